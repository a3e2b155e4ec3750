"""ctypes binding of tests/cpu_shim/inflate_plan_shim.cpp: the host decisions of the inflate entry points
(flate_amd/csrc/inflate_plan.h) as the library computes them -- the chunk table, the LDS ring, the pinned sub-batches, the
k_inflate_par rule, the span pool's bound, the copy-out plan, the rules of the resumable inflater's host feeds.  TEST
INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libinflate_plan_shim.so")
CSRC = os.path.join(ROOT, "flate_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("inflate_plan.h", "flate_layout.h", "flate_common.h")]
HOST_PASS_CHUNKS = 1024     # FLATE_HIP_HOST_PASS_CHUNKS default (flate_hip.hip, fl_knobs)
NONE, DENSE, PACKED = 0, 1, 2   # fl_copy_out_kind

_lib = None


def newer(target, deps):
    return os.path.exists(target) and os.path.getmtime(target) >= max(os.path.getmtime(d) for d in deps)


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "inflate_plan_shim.cpp")
        if not newer(SHIM_SO, [src] + DEPS):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        u32, u64, i64, i, p = C.c_uint32, C.c_uint64, C.c_int64, C.c_int, C.c_void_p
        L.shim_inflate_const.restype = u64
        L.shim_inflate_ring_large.argtypes = [i64, u32]
        L.shim_inflate_pin_io.argtypes = [i, i, u64, u64, u32, u64]
        L.shim_inflate_sub_batch.argtypes = [u32, u64]
        L.shim_inflate_sub_batch.restype = u32
        L.shim_inflate_par.argtypes = [p, p, p, u32, i64, i, p]
        L.shim_inflate_oversize.argtypes = [p, u32]
        L.shim_inflate_oversize.restype = u32
        L.shim_inflate_chunks.argtypes = [p, p, u32, u64, u64, p]
        L.shim_inflate_pool_release.argtypes = [u64]
        L.shim_copy_out_plan.argtypes = [p, p, u32, p]
        L.shim_inflater_slots_ok.argtypes = [p, p, p, u32]
        L.shim_inflater_rebase.argtypes = [p, p, u32, p, p]
        L.shim_inflater_copy_each.argtypes = [u32]
        _lib = L
    return _lib


def _u64(v):
    return np.ascontiguousarray(np.array(list(v), np.uint64))


def _u32(v):
    return np.ascontiguousarray(np.array(list(v), np.uint32))


def consts():
    """(small ring, large ring, the longest input of a stream)"""
    return tuple(int(lib().shim_inflate_const(k)) for k in range(3))


def ring_large(knob, n_streams):
    return bool(lib().shim_inflate_ring_large(knob, n_streams))


def pin_io(in_pinned, out_pinned, in_bytes, out_bytes, n_streams, host_pass_chunks=HOST_PASS_CHUNKS):
    return bool(lib().shim_inflate_pin_io(int(in_pinned), int(out_pinned), in_bytes, out_bytes, n_streams, host_pass_chunks))


def sub_batch(n_streams, host_pass_chunks=HOST_PASS_CHUNKS):
    return int(lib().shim_inflate_sub_batch(n_streams, host_pass_chunks))


def sub_batches(n_streams, host_pass_chunks=HOST_PASS_CHUNKS):
    """the sizes of the sub-batches as the driver's loop cuts them: sub streams each, the last what is left"""
    sub = sub_batch(n_streams, host_pass_chunks)
    return [min(sub, n_streams - c0) for c0 in range(0, n_streams, sub)]


def par(streams, knob=-1, flags=0):
    """streams: (in_len, out_cap) or (in_len, out_cap, skip) -> (use, min_bytes, n_big, taken)"""
    rows = [tuple(s) + (0,) * (3 - len(s)) for s in streams]
    a, b, c = _u32(r[0] for r in rows), _u64(r[1] for r in rows), _u32(r[2] for r in rows)
    out = np.zeros(3, np.uint64)
    use = lib().shim_inflate_par(a.ctypes.data, b.ctypes.data, c.ctypes.data, len(rows), knob, flags, out.ctypes.data)
    return bool(use), int(out[0]), int(out[1]), int(out[2])


def oversize(hin):
    a = _u64(hin)
    return int(lib().shim_inflate_oversize(a.ctypes.data, len(hin) - 1))


def chunks(hin, hout=None, in_shift=0, out_shift=0):
    """[(in_off, out_off, out_cap, in_len)] of the table, or None where it is refused; every other field must be 0"""
    n = len(hin) - 1
    a = _u64(hin)
    b = _u64(hout) if hout is not None else None
    rows = np.zeros((max(n, 1), 5), np.uint64)
    ok = lib().shim_inflate_chunks(a.ctypes.data, b.ctypes.data if b is not None else None, n, in_shift, out_shift, rows.ctypes.data)
    assert ok in (0, 1)
    if not ok:
        return None
    assert all(int(r[4]) == 1 for r in rows[:n])
    return [tuple(int(x) for x in r[:4]) for r in rows[:n]]


def pool_release(pool_bytes):
    return bool(lib().shim_inflate_pool_release(pool_bytes))


def copy_out(hout, out_len):
    """(kind, total, end)"""
    a, b = _u64(hout), _u64(list(out_len) + [0])
    out = np.zeros(2, np.uint64)
    kind = lib().shim_copy_out_plan(a.ctypes.data, b.ctypes.data, len(hout) - 1, out.ctypes.data)
    return kind, int(out[0]), int(out[1])


def inflater_slots_ok(in_off, out_off, final):
    a, b, c = _u64(in_off), _u64(out_off), np.ascontiguousarray(np.array(list(final), np.uint8))
    assert len(in_off) == len(out_off) == len(final) + 1
    return bool(lib().shim_inflater_slots_ok(a.ctypes.data, b.ctypes.data, c.ctypes.data, len(final)))


def inflater_rebase(in_off, out_off):
    """(hin, hout): the offsets the staged copies are read with"""
    a, b = _u64(in_off), _u64(out_off)
    hin, hout = np.zeros(len(in_off), np.uint64), np.zeros(len(out_off), np.uint64)
    assert lib().shim_inflater_rebase(a.ctypes.data, b.ctypes.data, len(in_off) - 1, hin.ctypes.data, hout.ctypes.data) == 1
    return [int(x) for x in hin], [int(x) for x in hout]


def inflater_copy_each(n_streams):
    return bool(lib().shim_inflater_copy_each(n_streams))
