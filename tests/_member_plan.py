"""ctypes binding of tests/cpu_shim/member_plan_shim.cpp: the rules by which flate_hip_decompress_members follows a
stream's chain of members (flate_amd/csrc/member_plan.h), compiled for the CPU.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(_ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libmember_plan_shim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "member_plan_shim.cpp")
        deps = [src, os.path.join(_ROOT, "flate_amd", "csrc", "member_plan.h")]
        if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        L.shim_member_miss_status.argtypes = [C.c_uint64]
        L.shim_member_stream_of.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
        L.shim_member_stream_of.restype = C.c_uint32
        L.shim_member_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64,
                                        C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
        L.shim_member_slots.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
        L.shim_member_scan_tiles.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
        L.shim_member_scan_cap.argtypes = [C.c_uint64, C.c_uint32]
        L.shim_member_scan_cap.restype = C.c_uint64
        L.shim_member_walk_offsets.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
        L.shim_member_walk_offsets.restype = C.c_uint64
        L.shim_member_count_ok.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64]
        L.shim_member_partition.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        _lib = L
    return _lib


OK, NO_FIRST, ORDER = 0, 1, 2   # fl_member_fault


def scan_tiles(base, lo, hi):
    """(rel0, n_tiles), or None where the scan would need more tiles than a grid has"""
    rel0, n_tiles = C.c_int64(0), C.c_uint64(0)
    ok = lib().shim_member_scan_tiles(base, lo, hi, C.byref(rel0), C.byref(n_tiles))
    return (rel0.value, n_tiles.value) if ok else None


def scan_cap(n_cand, n_streams):
    return int(lib().shim_member_scan_cap(n_cand, n_streams))


def walk_offsets(hin, container):
    """(toff[0..n], capacity)"""
    a = np.array(hin, np.uint64)
    toff = np.zeros(len(hin), np.uint64)
    cap = lib().shim_member_walk_offsets(a.ctypes.data, len(hin) - 1, container, toff.ctypes.data)
    return [int(x) for x in toff], int(cap)


def count_ok(M, n_streams, cap):
    return bool(lib().shim_member_count_ok(M, n_streams, cap))


def partition(doff, mstart, msize, vin, vout):
    """(fault, stream, min_, mout): the members' input offsets and slots (None, None where the table is refused)"""
    n, M = len(doff) - 1, doff[-1]
    d, s, z = np.array(doff, np.uint64), np.array(list(mstart) + [0], np.uint32), np.array(list(msize) + [0], np.uint64)
    vi, vo = np.array(vin, np.uint64), np.array(vout, np.uint64)
    min_, mout = np.zeros(M + 1, np.uint64), np.zeros(M + 1, np.uint64)
    stream = C.c_uint32(0)
    fault = lib().shim_member_partition(d.ctypes.data, s.ctypes.data, z.ctypes.data, vi.ctypes.data, vo.ctypes.data, n,
                                        min_.ctypes.data, mout.ctypes.data, C.byref(stream))
    if fault:
        return fault, stream.value, None, None
    return fault, stream.value, [int(x) for x in min_], [int(x) for x in mout]


def scan_tile():
    return lib().shim_member_scan_tile()


def lds_tile():
    return lib().shim_member_lds_tile()


def least_bytes(container):
    return lib().shim_member_least_bytes(container)


def stream_of(off, p):
    a = np.array(off, np.uint64)
    return lib().shim_member_stream_of(a.ctypes.data, len(off) - 1, p)


def chain(cands, start, end):
    """cands: [(position, status, consumed, size)] ascending -> ([(start relative to the stream, size)], status, on chain)"""
    n = len(cands)
    pos = np.array([c[0] for c in cands] + [0], np.uint64)
    st = np.array([c[1] for c in cands] + [0], np.int32)
    used = np.array([c[2] for c in cands] + [0], np.uint64)
    size = np.array([c[3] for c in cands] + [0], np.uint64)
    tab_start = np.zeros(n + 1, np.uint32)
    tab_size = np.zeros(n + 1, np.uint64)
    status, on = C.c_int32(-7), C.c_uint32(0)
    m = lib().shim_member_chain(pos.ctypes.data, st.ctypes.data, used.ctypes.data, size.ctypes.data, n, start, end,
                                tab_start.ctypes.data, tab_size.ctypes.data, C.byref(status), C.byref(on))
    return [(int(tab_start[k]), int(tab_size[k])) for k in range(m)], status.value, on.value


def slots(sizes, slot_start, slot_end):
    a = np.array(list(sizes) + [0], np.uint64)
    out = np.zeros(len(sizes) + 1, np.uint64)
    lib().shim_member_slots(a.ctypes.data, len(sizes), slot_start, slot_end, out.ctypes.data)
    return [int(x) for x in out[:len(sizes)]]
