"""ctypes binding of tests/cpu_shim/pass_plan_shim.cpp: the pass schedule of a chunk-path batch
(flate_amd/csrc/pass_plan.h) and the workspace bytes per chunk and per block, as the library computes them.
Used by the CPU tests of the schedule and by the GPU tests that size what a handle may hold."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libpass_plan_shim.so")
HOST_PASS_CHUNKS = 1024     # FLATE_HIP_HOST_PASS_CHUNKS default (flate_hip.hip, fl_knobs)
MAX_PASS_CHUNKS = 32768     # FLATE_HIP_MAX_PASS_CHUNKS default

_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "pass_plan_shim.cpp")
        deps = [src, os.path.join(ROOT, "include", "flate_hip.h")] + [
            os.path.join(ROOT, "flate_amd", "csrc", h)
            for h in ("pass_plan.h", "stream_tables.h", "flate_layout.h", "flate_common.h")]
        if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined", "-fno-sanitize-recover",
                            "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        L.shim_pass_schedule.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_int, C.POINTER(C.c_uint64)]
        L.shim_pass_schedule.restype = C.c_int
        L.shim_lz_chunk_bytes.argtypes = [C.c_int]
        L.shim_lz_chunk_bytes.restype = C.c_uint64
        L.shim_block_bytes.restype = C.c_uint64
        _lib = L
    return _lib


def schedule(n, host=HOST_PASS_CHUNKS, max_pass=MAX_PASS_CHUNKS, pinned=True, ramp=True, planned=False):
    """[(c0, nc, stream), ...] and the largest pass"""
    L = lib()
    largest = C.c_uint64(0)
    k = L.shim_pass_schedule(n, host, max_pass, int(pinned), int(ramp), int(planned), None, 0, C.byref(largest))
    buf = np.zeros(3 * max(k, 1), dtype=np.uint64)
    k2 = L.shim_pass_schedule(n, host, max_pass, int(pinned), int(ramp), int(planned), buf.ctypes.data, k,
                              C.byref(largest))
    assert k2 == k
    return [tuple(int(x) for x in buf[3 * i: 3 * i + 3]) for i in range(k)], int(largest.value)


def lz_chunk_bytes(level):
    """LZ workspace bytes per chunk of a pass (levels 8-9 keep four link arrays instead of one)"""
    return int(lib().shim_lz_chunk_bytes(int(level >= 8)))


def block_bytes():
    """plan + histograms + checksum words of one block slot"""
    return int(lib().shim_block_bytes())
