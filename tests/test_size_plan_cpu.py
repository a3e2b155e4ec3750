"""The host-side decisions of the size probe (flate_amd/csrc/size_plan.h) on the CPU: which streams are cut, where the scan
for block starts is aimed, and when the records of a stream's spans form a closed chain whose lengths may be summed.  The
shim (tests/cpu_shim/size_plan_shim.cpp) is built the way tests/_planner_shim.py builds its own.  No GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libsize_plan_shim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "size_plan_shim.cpp")
        deps = [src, os.path.join(ROOT, "flate_amd", "csrc", "size_plan.h")]
        if not os.path.exists(SHIM_SO) or os.path.getmtime(SHIM_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=undefined", "-fno-sanitize-recover",
                            "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        L.shim_size_eligible.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]
        L.shim_size_spacing.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.shim_size_targets.argtypes = [C.c_uint64, C.c_uint32, C.c_void_p, C.c_int]
        L.shim_size_follow_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def follow(spans):
    """spans: [(start_bit, end_bit, out_len, need_hist, status, final_seen, consumed)] -> (size, status, consumed) or None"""
    start = np.array([s[0] for s in spans], np.uint64)
    rec = np.array([[s[1], s[2], s[3], s[6], s[4], s[5]] for s in spans], np.uint64).reshape(-1)
    size, status, used = C.c_uint64(0), C.c_int32(-7), C.c_uint64(0)
    ok = lib().shim_size_follow_chain(start.ctypes.data, rec.ctypes.data, len(spans), C.byref(size), C.byref(status),
                                      C.byref(used))
    return (size.value, status.value, used.value) if ok else None


def span(start, end, out_len, need=0, status=0, final=0, consumed=0):
    return (start, end, out_len, need, status, final, consumed)


CLOSED = [span(0, 1000, 70000), span(1000, 2400, 5), span(2400, 3001, 123456, final=1, consumed=376)]


def test_a_chain_closes():
    assert follow(CLOSED) == (70000 + 5 + 123456, 0, 376)
    assert follow([span(0, 77, 0, final=1, consumed=10)]) == (0, 0, 10)
    # more than 4 GiB is summed in 64 bits
    big = [span(0, 10, 3 << 30), span(10, 20, 3 << 30, final=1, consumed=3)]
    assert follow(big) == (6 << 30, 0, 3)


def test_spans_that_start_inside_a_live_span_are_dead():
    """a position that parsed by accident inside span 0: nothing lands on it, its record is ignored whatever it says"""
    dead = span(500, 900, 9999, need=5, status=7)
    assert follow([CLOSED[0], dead, CLOSED[1], CLOSED[2]]) == follow(CLOSED)


def test_a_gap_does_not_close():
    for end in (999, 1001, 2401, 3001):
        assert follow([span(0, end, 70000), CLOSED[1], CLOSED[2]]) is None
    assert follow([CLOSED[0], span(1000, 2399, 5), CLOSED[2]]) is None


@pytest.mark.parametrize("where", [0, 1, 2])
def test_an_error_span_does_not_close(where):
    spans = list(CLOSED)
    s = spans[where]
    spans[where] = span(s[0], s[1], s[2], status=11, final=s[5], consumed=s[6])
    assert follow(spans) is None


def test_need_hist_at_the_edge():
    ok = [span(0, 1000, 300), span(1000, 2000, 40, need=300), span(2000, 3000, 7, need=340, final=1, consumed=375)]
    assert follow(ok) == (347, 0, 375)
    assert follow([ok[0], span(1000, 2000, 40, need=301), ok[2]]) is None
    assert follow([ok[0], ok[1], span(2000, 3000, 7, need=341, final=1, consumed=375)]) is None
    # the first span has nothing before it: any match that leaves it is InvalidMatch, for the whole-stream kernel to report
    assert follow([span(0, 100, 3, need=1, final=1, consumed=13)]) is None
    assert follow([span(0, 100, 4, need=0, final=1, consumed=13)]) == (4, 0, 13)


def test_no_bfinal_does_not_close():
    assert follow([span(0, 1000, 5), span(1000, 2000, 5)]) is None
    assert follow([span(0, 1000, 5)]) is None


def spacing(lens, n_cu):
    a = np.array(lens, np.uint64)
    p = np.zeros(len(lens), np.uint32)
    lib().shim_size_spacing(a.ctypes.data, len(lens), n_cu, p.ctypes.data)
    return [int(x) for x in p]


def targets(in_len, p):
    buf = np.zeros(2 * max(p, 1), np.uint64)
    k = lib().shim_size_targets(in_len, p, buf.ctypes.data, max(p, 1))
    return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(k)]


def test_spacing_respects_the_minimum_and_the_cap():
    L = lib()
    span_bytes, span_max, streams_max = L.shim_size_span_bytes(), L.shim_size_span_max(), L.shim_size_streams_max()
    rng = random.Random(11)
    batches = [[40 * 1024], [span_bytes - 1], [span_bytes], [2 * span_bytes - 1], [2 * span_bytes], [177 << 20],
               [0xfffffff0], [0xfffffff0] * streams_max, [1 << 20] * 128, [span_bytes] * streams_max,
               [1 << 30] + [span_bytes] * (streams_max - 1)]
    batches += [[rng.randrange(1, 1 << rng.randrange(10, 32)) for _ in range(rng.randrange(1, streams_max + 1))]
                for _ in range(200)]
    for lens in batches:
        for n_cu in (1, 8, 256, 304, 4096):
            pieces = spacing(lens, n_cu)
            assert sum(pieces) <= span_max, (lens[:4], n_cu)
            for n, p in zip(lens, pieces):
                assert p >= 1
                if p == 1:
                    assert targets(n, p) == []
                    continue
                assert n // p >= span_bytes, (n, p)
                t = targets(n, p)
                assert len(t) == p - 1
                edges = [0] + [f for f, _ in t] + [8 * n]
                assert all(b - a >= 8 * span_bytes for a, b in zip(edges, edges[1:])), (n, p)
                # the windows tile [first target, end of stream): no block start can be missed between two of them
                assert all(t[i][1] == t[i + 1][0] for i in range(len(t) - 1)) and t[-1][1] == 8 * n
    assert spacing([4 << 20], 256)[0] > 16  # a long stream alone is cut into many pieces
    assert spacing([40 * 1024], 256) == [2]


def eligible(lens, min_bytes, n_cu):
    a = np.array(lens, np.uint64)
    out = np.zeros(len(lens), np.uint32)
    k = lib().shim_size_eligible(a.ctypes.data, len(lens), min_bytes, n_cu, out.ctypes.data)
    return [int(x) for x in out[:k]]


def test_which_streams_are_cut():
    long_, short = 1 << 20, 20000
    assert eligible([short, long_, short, long_], 131072, 256) == [1, 3]
    assert eligible([long_] * 4, 0, 256) == []                      # FLATE_HIP_INFLATE_SPANS=0: never
    assert eligible([long_] * 256, 131072, 256) == list(range(256))
    assert eligible([long_] * 257, 131072, 256) == []               # the long streams fill the chip by themselves
    assert eligible([long_] * 9, 131072, 8) == []
    assert eligible([short] * 16385, 131072, 256) == []
    assert eligible([40000] * 300, 32768, 304) == []                # more than a call cuts
