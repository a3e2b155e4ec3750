"""ctypes binding of tests/cpu_shim/index_plan_shim.cpp: the host decisions of the seek index (flate_amd/csrc/index_plan.h) as
the library computes them -- the point rule, point selection, clipping, the scratch slots, the passes, and the blob."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libindex_plan_shim.so")
HEADERS = ("index_plan.h",)
CONSTS = ("window", "spacing_default", "slack", "slot_align", "pass_bytes", "hdr_bytes", "stream_bytes", "point_bytes", "version", "in_spare")

_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "index_plan_shim.cpp")
        deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in HEADERS]
        if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        u32, u64, i, i32, p = C.c_uint32, C.c_uint64, C.c_int, C.c_int32, C.c_void_p
        for name, args, res in (("shim_idx_const", [i], u64), ("shim_idx_args_ok", [i, i], i), ("shim_idx_spacing", [u64], u64),
                                ("shim_idx_max_points", [u64, u64], u64), ("shim_idx_window_len", [u64], u32),
                                ("shim_idx_clip", [u64, u64, u64], u64), ("shim_idx_slot_bytes", [u64], u64),
                                ("shim_idx_point_rule", [p, u64, u64, p], u64), ("shim_idx_select", [p, u64, u64], u64),
                                ("shim_idx_plan_range", [u64, i32, p, u64, u32, u32, u64, u64, u64, p, p, u64], None),
                                ("shim_idx_merge", [p, u64, u64], u64),
                                ("shim_idx_passes", [p, u64, u64, p, p, p], u64),
                                ("shim_idx_blob", [u32, u64, u32, p, p, p, p, p, p, p], u64),
                                ("shim_idx_parse", [p, u64, p, p, u64, p, u64], i)):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = res
        _lib = L
    return _lib


def const(name):
    return int(lib().shim_idx_const(CONSTS.index(name)))


def _u64(a):
    return np.ascontiguousarray(np.array(list(a) + [0], np.uint64))


def point_rule(pos, spacing):
    a, which = _u64(pos), np.zeros(len(pos) + 1, np.uint64)
    n = lib().shim_idx_point_rule(a.ctypes.data, len(pos), spacing, which.ctypes.data)
    return [int(x) for x in which[:n]]


def select(out_pos, begin):
    a = _u64(out_pos)
    return int(lib().shim_idx_select(a.ctypes.data, len(out_pos), begin))


def clip(begin, length, size):
    return int(lib().shim_idx_clip(begin, length, size))


def slot_bytes(need):
    return int(lib().shim_idx_slot_bytes(need))


def plan_range(size, status, out_pos, begin, length, cap, n_streams=3, stream=1, in_bit=None, in_len=100):
    """dict(point, skip, len, status, decode) of one range of a stream with the points out_pos; with in_bit (the points' bits)
    also in_lo, in_hi: the bytes of the stream of in_len bytes that the decode can consume"""
    a, out = _u64(out_pos), np.zeros(7, np.uint64)
    b = None if in_bit is None else _u64(in_bit)
    lib().shim_idx_plan_range(size, status, a.ctypes.data, len(out_pos), n_streams, stream, begin, length, cap, out.ctypes.data,
                              None if b is None else b.ctypes.data, in_len)
    r = dict(point=int(out[0]), skip=int(out[1]), len=int(out[2]), status=int(out[3].astype(np.int64)), decode=int(out[4]))
    if in_bit is not None:
        r.update(in_lo=int(out[5]), in_hi=int(out[6]))
    return r


def merge(intervals, gap):
    """[(lo, hi)] merged where they touch or lie less than gap apart"""
    a = _u64(x for iv in intervals for x in iv)
    n = lib().shim_idx_merge(a.ctypes.data, len(intervals), gap)
    return [(int(a[2 * k]), int(a[2 * k + 1])) for k in range(n)]


def passes(slots, budget):
    """(pass boundaries, the ranges' places in their pass's scratch, the largest pass's scratch)"""
    a, first, off, most = _u64(slots), np.zeros(len(slots) + 2, np.uint64), np.zeros(len(slots) + 1, np.uint64), C.c_uint64()
    n = lib().shim_idx_passes(a.ctypes.data, len(slots), budget, first.ctypes.data, off.ctypes.data, C.addressof(most))
    return [int(x) for x in first[:n + 1]], [int(x) for x in off[:len(slots)]], int(most.value)


def blob(container, spacing, streams):
    """streams: [(in_len, size, status, [(in_bit, out_pos)])] -> the blob, its windows filled with a pattern"""
    in_len, size, npts = _u64(s[0] for s in streams), _u64(s[1] for s in streams), _u64(len(s[3]) for s in streams)
    status = np.ascontiguousarray(np.array([s[2] for s in streams] + [0], np.int32))
    bit, pos = _u64(b for s in streams for b, _ in s[3]), _u64(p for s in streams for _, p in s[3])
    args = (container, spacing, len(streams), in_len.ctypes.data, size.ctypes.data, status.ctypes.data, npts.ctypes.data, bit.ctypes.data,
            pos.ctypes.data)
    n = lib().shim_idx_blob(*args, None)
    out = np.zeros(n, np.uint8)
    lib().shim_idx_blob(*args, out.ctypes.data)
    return out.tobytes()


def parse(data, room_streams=1 << 12, room_points=1 << 16):
    """None when the blob is refused, else dict(container, spacing, win_bytes, win_at, streams=[(in_len, size, status, [(in_bit,
    out_pos, win_off)])])"""
    raw = np.frombuffer(bytes(data) + b"\0", np.uint8)
    head, rows, pts = np.zeros(6, np.uint64), np.zeros((room_streams, 5), np.uint64), np.zeros((room_points, 3), np.uint64)
    if not lib().shim_idx_parse(raw.ctypes.data, len(data), head.ctypes.data, rows.ctypes.data, room_streams, pts.ctypes.data, room_points):
        return None
    ns = int(head[2])
    assert ns <= room_streams and int(head[3]) <= room_points
    streams = []
    for r in rows[:ns]:
        p0, n = int(r[2]), int(r[3])
        streams.append((int(r[0]), int(r[1]), int(r[4].astype(np.int64)), [tuple(int(x) for x in q) for q in pts[p0:p0 + n]]))
    return dict(container=int(head[0]), spacing=int(head[1]), win_bytes=int(head[4]), win_at=int(head[5]), streams=streams)
