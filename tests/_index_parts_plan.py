"""ctypes binding of tests/cpu_shim/index_parts_plan_shim.cpp: the host decisions of the fresh seek index
(flate_amd/csrc/index_parts_plan.h) as the library computes them -- the points of a joined stream, the cut of a range into
parts, the part table of a call with its passes, and the version-2 blob."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libindex_parts_plan_shim.so")
HEADERS = ("index_parts_plan.h", "index_plan.h", "size_plan.h")
CONSTS = ("version", "max_parts")

_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "index_parts_plan_shim.cpp")
        deps = [src] + [os.path.join(ROOT, "flate_amd", "csrc", h) for h in HEADERS]
        if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        u32, u64, i, p = C.c_uint32, C.c_uint64, C.c_int, C.c_void_p
        for name, args, res in (("shim_idxp_const", [i], u64), ("shim_idxp_point_pieces", [u64, u32, u64, p], u64),
                                ("shim_idxp_points", [p, p, u64, u32, p], None),
                                ("shim_idxp_plan_call", [u32, p, p, p, p, p, p, u32, p, p, p, p, u64, p, p, p, u64, p], None),
                                ("shim_idxp_blob", [u32, u64, u32, p, p, p, p, p, p, p], u64),
                                ("shim_idxp_version", [p, u64], u32),
                                ("shim_idxp_parse", [p, u64, p, p, u64, p, u64], i)):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = res
        _lib = L
    return _lib


def const(name):
    return int(lib().shim_idxp_const(CONSTS.index(name)))


def _u64(a):
    return np.ascontiguousarray(np.array(list(a) + [0], np.uint64))


def point_pieces(n, piece, spacing):
    """the pieces of a joined stream of n bytes that are points"""
    cnt = int(lib().shim_idxp_point_pieces(n, piece, spacing, None))
    which = np.zeros(cnt + 1, np.uint64)
    assert int(lib().shim_idxp_point_pieces(n, piece, spacing, which.ctypes.data)) == cnt
    return [int(x) for x in which[:cnt]]


def points(which, place, piece):
    """[(in_bit, out_pos, win_off)] of the point pieces `which` that begin `place` bytes into their stream"""
    a, b, out = _u64(which), _u64(place), np.zeros((len(which) + 1, 3), np.uint64)
    lib().shim_idxp_points(a.ctypes.data, b.ctypes.data, len(which), piece, out.ctypes.data)
    return [tuple(int(x) for x in r) for r in out[:len(which)]]


def _tables(streams):
    in_len, size, npts = _u64(s[0] for s in streams), _u64(s[1] for s in streams), _u64(len(s[3]) for s in streams)
    status = np.ascontiguousarray(np.array([s[2] for s in streams] + [0], np.int32))
    bit, pos = _u64(b for s in streams for b, _ in s[3]), _u64(p for s in streams for _, p in s[3])
    return [in_len, size, status, npts, bit, pos]


def plan_call(streams, ranges, caps, budget, room_parts=1 << 16):
    """streams: [(in_len, size, status, [(in_bit, out_pos)])]; ranges: [(stream, begin, len)]; caps: the slots' sizes.
    None when the call has too many parts, else dict(ranges=[dict(part0, n_parts, len, status)], parts=[dict(point, skip,
    len, dst, in_lo, in_hi, range, direct, slot_off)], pass_first, scratch, n_direct, n_scratch)."""
    tabs = _tables(streams)
    n = len(ranges)
    rs = np.ascontiguousarray(np.array([r[0] for r in ranges] + [0], np.uint32))
    rb, rl = _u64(r[1] for r in ranges), _u64(r[2] for r in ranges)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(np.array(list(caps), np.uint64), out=off[1:])
    head, rows, parts = np.zeros(5, np.uint64), np.zeros((n + 1, 4), np.uint64), np.zeros((room_parts, 9), np.uint64)
    first = np.zeros(room_parts + 2, np.uint64)
    lib().shim_idxp_plan_call(len(streams), *[t.ctypes.data for t in tabs], n, rs.ctypes.data, rb.ctypes.data, rl.ctypes.data,
                              off.ctypes.data, budget, head.ctypes.data, rows.ctypes.data, parts.ctypes.data, room_parts,
                              first.ctypes.data)
    if int(head[0]) == (1 << 64) - 1:
        return None
    npart, npass = int(head[0]), int(head[1])
    assert npart <= room_parts
    keys = ("point", "skip", "len", "dst", "in_lo", "in_hi", "range", "direct", "slot_off")
    return dict(ranges=[dict(part0=int(r[0]), n_parts=int(r[1]), len=int(r[2]), status=int(r[3].astype(np.int64))) for r in rows[:n]],
                parts=[dict(zip(keys, (int(x) for x in q))) for q in parts[:npart]],
                pass_first=[int(x) for x in first[:npass + 1]] if npart else [0],
                scratch=int(head[2]), n_direct=int(head[3]), n_scratch=int(head[4]))


def blob(container, spacing, streams):
    """streams: [(in_len, size, status, [(in_bit, out_pos)])] -> the version-2 blob"""
    tabs = _tables(streams)
    args = (container, spacing, len(streams)) + tuple(t.ctypes.data for t in tabs)
    n = lib().shim_idxp_blob(*args, None)
    out = np.zeros(n, np.uint8)
    assert lib().shim_idxp_blob(*args, out.ctypes.data) == n
    return out.tobytes()


def version(data):
    raw = np.frombuffer(bytes(data) + b"\0", np.uint8)
    return int(lib().shim_idxp_version(raw.ctypes.data, len(data)))


def parse(data, room_streams=1 << 12, room_points=1 << 16):
    """None when the version-2 parser refuses the blob, else dict(container, spacing, win_bytes, streams=[(in_len, size,
    status, [(in_bit, out_pos, win_off)])])"""
    raw = np.frombuffer(bytes(data) + b"\0", np.uint8)
    head, rows, pts = np.zeros(5, np.uint64), np.zeros((room_streams, 5), np.uint64), np.zeros((room_points, 3), np.uint64)
    if not lib().shim_idxp_parse(raw.ctypes.data, len(data), head.ctypes.data, rows.ctypes.data, room_streams, pts.ctypes.data, room_points):
        return None
    ns = int(head[2])
    assert ns <= room_streams and int(head[3]) <= room_points
    streams = []
    for r in rows[:ns]:
        p0, n = int(r[2]), int(r[3])
        streams.append((int(r[0]), int(r[1]), int(r[4].astype(np.int64)), [tuple(int(x) for x in q) for q in pts[p0:p0 + n]]))
    return dict(container=int(head[0]), spacing=int(head[1]), win_bytes=int(head[4]), streams=streams)
