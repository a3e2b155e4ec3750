"""The host-side decisions of the span inflater (flate_amd/csrc/span_plan.h) on the CPU: which streams are cut and where
the scan is aimed, the spans its answers make, the walk over a stream's span records, the work items of k_span_fix, and
the fold of their checksum parts against the footer.  The shim (tests/cpu_shim/span_plan_shim.cpp) is built the way
tests/test_size_plan_cpu.py builds its own, without a sanitizer; tests/host_cpp/test_span_plan.cpp runs the same functions
over random and hostile records under AddressSanitizer and UBSan as a program of its own.  No GPU.

Every expected value below is worked out by hand from the rule as span_plan.h states it, with 256 CUs, the default bound of
131072 bytes, one decode in symbols and FLATE_HIP_SPAN_TWIN unset unless a test says otherwise."""
import ctypes as C
import os
import random
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT

SHIM_DIR = os.path.join(ROOT, "tests", "cpu_shim")
SHIM_SO = os.path.join(SHIM_DIR, "libspan_plan_shim.so")
CSRC = os.path.join(ROOT, "flate_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("span_plan.h", "flate_layout.h", "flate_common.h")]
_lib = None

TAIL, NO_SPAN, ITEM, WAVES, PIECE = 32768, 0xffffffff, 65536, 4, 65536
NONE = (1 << 64) - 1  # what the scan answers for a target without a block start
N_CU, MIN_BYTES = 256, 131072
MIB = 1 << 20


def newer(target, deps):
    return os.path.exists(target) and os.path.getmtime(target) >= max(os.path.getmtime(d) for d in deps)


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(SHIM_DIR, "span_plan_shim.cpp")
        if not newer(SHIM_SO, [src] + DEPS):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", SHIM_SO, src], check=True)
        L = C.CDLL(SHIM_SO)
        L.shim_span_const.restype = C.c_uint32
        L.shim_span_pool_pieces.restype = C.c_uint64
        L.shim_span_pool_pieces.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
        L.shim_span_eligible.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_uint32, C.c_int, C.c_void_p,
                                         C.POINTER(C.c_int)]
        L.shim_span_targets.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                        C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
        L.shim_cut_positions.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p]
        L.shim_span_build.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        L.shim_span_follow_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int,
                                             C.c_void_p, C.c_void_p]
        L.shim_span_fix_items.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
        L.shim_span_verify.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
        _lib = L
    return _lib


def u32(v):
    return np.ascontiguousarray(np.array(list(v), np.uint32))


def u64(v):
    return np.ascontiguousarray(np.array(list(v), np.uint64))


def test_the_constants_are_the_ones_this_file_reasons_with():
    assert [lib().shim_span_const(i) for i in range(8)] == [TAIL, NO_SPAN, ITEM, WAVES, 32, 65536, 1024, PIECE]


# ---------------------------------------------------------------- which streams are cut

def eligible(lens, min_bytes=MIN_BYTES, flags=0, n_cu=N_CU, knob=-1):
    a, out, twin = u32(lens), np.zeros(len(lens) + 1, np.uint32), C.c_int(-1)
    k = lib().shim_span_eligible(a.ctypes.data, len(lens), min_bytes, flags, n_cu, knob, out.ctypes.data, C.byref(twin))
    return [int(x) for x in out[:k]], bool(twin.value)


BIG, MID, SHORT = MIB, 40000, 20000  # at least the bound / long (32768 or more) but below the bound / not long


def test_up_to_32_long_streams_are_cut_many_times_and_only_those_of_the_bound():
    lens = [BIG] * 15 + [MID, SHORT] + [BIG] * 15 + [MID, SHORT, SHORT]  # 32 long ones, 30 of them of 131072 bytes or more
    assert eligible(lens) == ([i for i, n in enumerate(lens) if n == BIG], False)
    assert eligible([BIG]) == ([0], False)
    assert eligible([131071, 131072]) == ([1], False)
    assert eligible([MID] * 5) == ([], False)           # long, but none reaches the bound
    assert eligible([32768] * 5, min_bytes=32768) == ([0, 1, 2, 3, 4], False)
    assert eligible([32767] * 5, min_bytes=1000) == ([0, 1, 2, 3, 4], False)  # (not long, yet taken: the bound decides)


def test_33_to_140_long_streams_are_cut_once_each_and_the_bound_drops_to_32768():
    lens = [BIG] * 30 + [MID] * 3 + [SHORT] * 4  # 33 long ones
    assert eligible(lens) == (list(range(33)), True)
    assert eligible(lens, min_bytes=20000) == (list(range(37)), True)  # min(20000, 32768): a lower bound stays
    assert eligible([32767, 32768] * 33) == (list(range(1, 66, 2)), True)
    assert eligible([BIG] * 140) == (list(range(140)), True)  # 140 * 20 = 2800 <= 256 * 11 = 2816


def test_more_long_streams_than_eleven_twentieths_of_the_cus_are_left_alone():
    assert eligible([BIG] * 141) == ([], False)  # 141 * 20 = 2820 > 2816
    assert eligible([BIG] * 141, n_cu=257) == (list(range(141)), True)  # 2820 <= 2827
    assert eligible([BIG] * 33, n_cu=59) == ([], False)   # 660 > 649
    assert eligible([BIG] * 33, n_cu=60) == (list(range(33)), True)


def test_twin_knob_0_means_never():
    assert eligible([BIG] * 33, knob=0) == ([], False)
    assert eligible([BIG] * 32, knob=0) == (list(range(32)), False)  # the first rule does not ask the knob
    assert eligible([BIG] * 33, knob=700) == (list(range(33)), True)


def test_more_than_256_eligible_streams_are_left_alone():
    assert eligible([2000] * 256, min_bytes=1000) == (list(range(256)), False)
    assert eligible([2000] * 257, min_bytes=1000) == ([], False)
    assert eligible([BIG] * 256, n_cu=512) == (list(range(256)), True)
    assert eligible([BIG] * 257, n_cu=512) == ([], True)


def test_never_with_the_strict_header_or_a_bound_of_0():
    assert eligible([BIG] * 4, flags=1) == ([], False)
    assert eligible([BIG] * 4, flags=3) == ([], False)
    assert eligible([BIG] * 4, flags=2) == ([0, 1, 2, 3], False)
    assert eligible([BIG] * 4, min_bytes=0) == ([], False)
    assert eligible([BIG] * 40, flags=1) == ([], False)


# ---------------------------------------------------------------- where the scan is aimed

def targets(chunks, elig=None, twin=False, knob=-1, sym=True, n_cu=N_CU):
    """chunks: [(in_len, out_cap)] -> ([(from_bit, limit_bit, stream)], pt_first)"""
    elig = list(range(len(chunks))) if elig is None else elig
    lens, caps, el = u32(c[0] for c in chunks), u64(c[1] for c in chunks), u32(elig)
    cap = 1100
    out, first = np.zeros(3 * cap, np.uint64), np.zeros(len(elig) + 1, np.uint32)
    n = lib().shim_span_targets(lens.ctypes.data, caps.ctypes.data, len(chunks), el.ctypes.data, len(elig), int(twin), knob, int(sym),
                                n_cu, out.ctypes.data, cap, first.ctypes.data)
    assert n <= cap
    return [tuple(int(x) for x in out[3 * i:3 * i + 3]) for i in range(n)], [int(x) for x in first]


def test_targets_of_one_stream():
    """weight = max(in_len, min(out_cap, 32 in_len)) = 4194304; rounds = max(1, (4194304 + 256 * 393216) / (256 * 786432)) = 1;
    want = min(1024, 1 * 256 - 8, max(2, 4194304 / (3 * 65536))) = min(1024, 248, 21) = 21; P = max(2, min(21, 1 MiB / 16384)) = 21;
    bits / P = 8388608 / 21 = 399457"""
    pts, first = targets([(MIB, 4 * MIB)])
    assert first == [0, 20] and len(pts) == 20
    assert pts == [(399457 * j, 399457 * (j + 1) if j < 20 else 8388608, 0) for j in range(1, 21)]
    assert pts[-1] == (7989140, 8388608, 0)
    assert targets([(MIB, 4 * MIB)], sym=False) == (pts, first)  # (which decode: the twin cut's business only)


def test_a_span_has_at_least_a_quarter_of_FL_SPAN_BYTES_and_a_stream_at_least_one_target():
    """weight = max(40000, min(4 MiB, 1280000)) = 1280000; want = min(1024, 248, max(2, 1280000 / 196608 = 6)) = 6;
    P = max(2, min(6, 40000 / 16384 = 2)) = 2"""
    assert targets([(40000, 4 * MIB)]) == ([(160000, 320000, 0)], [0, 1])
    # weight = 32768 (the room is smaller than the stream): want = max(2, 0) = 2, P = max(2, min(2, 2)) = 2
    assert targets([(32768, 100)]) == ([(131072, 262144, 0)], [0, 1])
    # in_len / 16384 = 1: still two pieces
    assert targets([(20000, 4 * MIB)]) == ([(80000, 160000, 0)], [0, 1])


def test_the_streams_share_the_spans_by_the_room_their_callers_gave_them():
    """weights 4194304 and max(1 MiB, min(1 MiB, 32 MiB)) = 1048576, together 5242880; rounds 1;
    want = min(1024, 248, 5242880 / 196608 = 26) = 26; P = 26 * 4194304 / 5242880 = 20 and 26 * 1048576 / 5242880 = 5;
    8388608 / 20 = 419430, 8388608 / 5 = 1677721.  The stream in between is not eligible."""
    pts, first = targets([(MIB, 4 * MIB), (SHORT, 1 << 30), (MIB, MIB)], elig=[0, 2])
    assert first == [0, 19, 23]
    assert pts[:19] == [(419430 * j, 419430 * (j + 1) if j < 19 else 8388608, 0) for j in range(1, 20)]
    assert pts[19:] == [(1677721, 3355442, 2), (3355442, 5033163, 2), (5033163, 6710884, 2), (6710884, 8388608, 2)]


def test_long_inputs_get_a_multiple_of_the_cus():
    """in_len 100 MiB with room for 512 MiB: weight 536870912; rounds = min(4, (536870912 + 100663296) / 201326592 = 3) = 3;
    want = min(1024, 3 * 256 - 8 = 760, 536870912 / 196608 = 2730) = 760; P = min(760, 104857600 / 16384 = 6400) = 760;
    bits / P = 838860800 / 760 = 1103764"""
    pts, first = targets([(100 * MIB, 512 * MIB)])
    assert first == [0, 759]
    assert pts[0] == (1103764, 2207528, 0) and pts[-1] == (1103764 * 759, 838860800, 0)
    # room for 32 bytes per compressed byte and more, 1 GiB of input: rounds 4, and FL_SPAN_MAX = 1024 caps 4 * 256 - 8 = 1016 ... no:
    # want = min(1024, 1016, ...) = 1016
    pts, first = targets([(1 << 30, 1 << 40)])
    assert first == [0, 1015]
    # few CUs: min(8, n_cu / 2) = 2 are left to what else runs: want = min(1024, 4 * 4 - 2 = 14, ...) = 14
    assert targets([(1 << 30, 1 << 40)], n_cu=4)[1] == [0, 13]


def test_the_twin_cut():
    """one target per stream, at bits / 1000 * f (the division comes first): 8388608 / 1000 = 8388.
    128 streams, symbols: f = 1250 * 128 / (256 + 128 / 4) + 10 = 160000 / 288 + 10 = 565; two runs: 2000 * 128 / 384 + 15 = 681.
    56 streams, symbols: 70000 / 270 + 10 = 269, two runs: 112000 / 312 + 15 = 373: both clamped up to 500."""
    def cut(n, **kw):
        pts, first = targets([(MIB, 4 * MIB)] * n, twin=True, **kw)
        assert first == list(range(n + 1))
        assert [p[2] for p in pts] == list(range(n)) and all(p[1] == 8388608 for p in pts)
        assert len({p[0] for p in pts}) == 1
        return pts[0][0]

    assert cut(128) == 8388 * 565 == 4739220 != 8388608 * 565 // 1000
    assert cut(128, sym=False) == 8388 * 681
    assert cut(56) == 8388 * 500 and cut(56, sym=False) == 8388 * 500
    assert cut(128, knob=700) == 8388 * 700 and cut(128, knob=700, sym=False) == 8388 * 700
    assert cut(128, knob=2000) == 8388 * 950
    assert cut(128, knob=2) == 8388 * 2
    assert cut(128, knob=1) == 8388 * 565  # (1 and below: no place named)
    # 256 streams on 64 CUs (no batch gets there: the rule is clamped all the same): 320000 / 128 + 10 -> 900
    assert cut(256, n_cu=64) == 8388 * 900
    # a stream of 999 bits' worth: bits / 1000 = 7
    pts, _ = targets([(999, 4 * MIB)] * 40, twin=True)
    assert pts[0][:2] == (7 * 500, 7992)


# ---------------------------------------------------------------- the spans the scan's answers make

def cut_positions(found, j0=0, j1=None, limit=NONE):
    f, out = u64(found), np.zeros(len(found) + 1, np.uint64)
    n = lib().shim_cut_positions(f.ctypes.data, j0, len(found) if j1 is None else j1, limit, out.ctypes.data)
    return [int(x) for x in out[:n]]


def test_cut_positions_are_distinct_and_ascending():
    found = [100, 100, NONE, 90, 250, 300, 8000, 120, 8000]
    # the inflater: no limit
    assert cut_positions(found) == [100, 250, 300, 8000]
    # the size probe: below the stream's last bit
    assert cut_positions(found, limit=8000) == [100, 250, 300]
    assert cut_positions(found, limit=8001) == [100, 250, 300, 8000]
    assert cut_positions(found, limit=300) == [100, 250]
    assert cut_positions(found, limit=100) == [90]  # (the first 100s are at the limit: nothing is kept before 90 comes)
    assert cut_positions(found, limit=90) == []
    # one stream's targets only
    assert cut_positions(found, 3, 6) == [90, 250, 300]
    assert cut_positions(found, 2, 3) == [] and cut_positions(found, 4, 4) == []
    # the stream's start is the first span's: never a cut
    assert cut_positions([0, 0, 17]) == [17]
    assert cut_positions([NONE] * 4) == []


def test_the_spans_of_a_batch():
    """three chunks, the middle one not eligible; chunk 0 has three targets (two name the same place), chunk 2 two (one found
    nothing)"""
    elig, pt_first, found = u32([0, 2]), u32([0, 3, 5]), u64([700, 700, 9000, NONE, 4400])
    out, cand, cand_off, sp_first = np.zeros(6 * 7, np.uint64), np.zeros(5, np.uint64), np.zeros(4, np.uint32), np.zeros(3, np.uint32)
    n = lib().shim_span_build(3, elig.ctypes.data, 2, pt_first.ctypes.data, found.ctypes.data, out.ctypes.data, cand.ctypes.data,
                              cand_off.ctypes.data, sp_first.ctypes.data)
    spans = [tuple(int(x) for x in out[6 * i:6 * i + 6]) for i in range(n)]
    #                 start stream first prev  live wp
    assert spans == [(0, 0, 1, NO_SPAN, 0, 0), (700, 0, 0, NO_SPAN, 0, 0), (9000, 0, 0, NO_SPAN, 0, 0),
                     (0, 2, 1, NO_SPAN, 0, 0), (4400, 2, 0, NO_SPAN, 0, 0)]
    assert list(sp_first) == [0, 3, 5]
    assert list(cand_off) == [0, 2, 2, 3] and list(cand[:3]) == [700, 9000, 4400]


def test_the_pool_holds_what_the_streams_can_and_two_pieces_a_span():
    lens, caps, el = u32([MIB, SHORT, 1000]), u64([4 * MIB + 5, 1 << 30, 1 << 30]), u32([0, 2])
    # min(4 MiB + 5, 32 MiB) + min(1 GiB, 32000) = 4226309 bytes -> 64 pieces, + 2 * 7 + 1
    pieces = lambda both: lib().shim_span_pool_pieces(lens.ctypes.data, caps.ctypes.data, 3, el.ctypes.data, 2, 7, both)
    assert pieces(0) == 64 + 14 + 1 and pieces(1) == 2 * (64 + 14 + 1)


# ---------------------------------------------------------------- the chain of a stream

def rec(end, out_len, status=0, final=0, hist=0, pieces=0):
    return (end, out_len, status, final, hist, pieces)


def follow(starts, recs, out_cap, both=False, a=0, b=None, live=None):
    """spans [a, b) of `starts` are one stream's (the first of them its first span).  Returns (ok, chain, total, end_bit,
    last, wp[], prev[], live[])"""
    n = len(starts)
    b = n if b is None else b
    live = [0] * n if live is None else live
    sp = u64(x for i in range(n) for x in (starts[i], 0, 1 if i == a else 0, NO_SPAN, live[i]))
    rc = u64(x for r in recs for x in r)
    chain, res = np.zeros(n + 1, np.uint32), np.zeros(4, np.uint64)
    ok = lib().shim_span_follow_chain(sp.ctypes.data, rc.ctypes.data, n, a, b, out_cap, int(both), chain.ctypes.data, res.ctypes.data)
    sp = sp.reshape(n, 5)
    return (bool(ok), [int(x) for x in chain[:int(res[3])]], int(res[0]), int(res[1]), int(res[2]),
            [int(x) for x in sp[:, 1]], [int(x) for x in sp[:, 3]], [int(x) for x in sp[:, 4]])


STARTS = [0, 1000, 2400]
CLOSED = [rec(1000, 70000), rec(2400, 5), rec(3001, 123456, final=1)]
TOTAL = 70000 + 5 + 123456


def test_a_chain_closes():
    ok, chain, total, end_bit, last, wp, prev, live = follow(STARTS, CLOSED, TOTAL)
    assert ok and chain == [0, 1, 2] and total == TOTAL and end_bit == 3001 and last == 2
    assert wp == [0, 70000, 70005] and prev == [NO_SPAN, 0, 1] and live == [1, 1, 1]
    # a stream that was never cut into more than its first span
    assert follow([0], [rec(77, 12, final=1)], 12)[:5] == (True, [0], 12, 77, 0)
    # an empty stream
    assert follow([0], [rec(10, 0, final=1)], 0)[:4] == (True, [0], 0, 10)
    # more than 4 GiB is summed in 64 bits
    assert follow([0, 10], [rec(10, 3 << 30), rec(20, 3 << 30, final=1)], 6 << 30)[:3] == (True, [0, 1], 6 << 30)


def test_span_numbers_are_those_of_the_whole_batch():
    """the stream's spans are 2 .. 4 of the batch's: chain and prev name them so, and the other stream is not touched"""
    starts, recs = [0, 555] + STARTS, [rec(1, 1, status=9)] * 2 + CLOSED
    ok, chain, total, end_bit, last, wp, prev, live = follow(starts, recs, TOTAL, a=2, live=[1, 0, 0, 0, 0])
    assert ok and chain == [2, 3, 4] and last == 4
    assert wp == [0, 0, 0, 70000, 70005] and prev == [NO_SPAN, NO_SPAN, NO_SPAN, 2, 3] and live == [1, 0, 1, 1, 1]
    ok, chain, *_, live = follow(starts + [9999], recs + [rec(1, 1)], TOTAL, a=2, b=5, live=[0, 1, 0, 0, 0, 1])
    assert ok and chain == [2, 3, 4] and live == [0, 1, 1, 1, 1, 1]


def test_a_span_that_starts_inside_a_live_one_is_dead():
    starts = [0, 500, 1000, 2400]
    recs = [CLOSED[0], rec(900, 9999, status=7, hist=1), CLOSED[1], CLOSED[2]]
    ok, chain, total, end_bit, last, wp, prev, live = follow(starts, recs, TOTAL)
    assert ok and chain == [0, 2, 3] and total == TOTAL and end_bit == 3001
    assert live == [1, 0, 1, 1] and prev[2] == 0 and prev[3] == 2 and wp[2] == 70000 and wp[3] == 70005


@pytest.mark.parametrize("end", [999, 1001, 2399, 2401, 3001, 0, NONE])
def test_a_gap_does_not_close(end):
    ok, chain, total, end_bit, last, wp, prev, live = follow(STARTS, [rec(end, 70000), CLOSED[1], CLOSED[2]], TOTAL, live=[0, 1, 1])
    assert not ok and chain == [0] and total == 70000 and last == 0
    assert live == [0, 0, 0]  # the whole stream, whatever it said before


@pytest.mark.parametrize("where", [0, 1, 2])
@pytest.mark.parametrize("status", [1, 11, 0xffffffff])
def test_a_status_anywhere_on_the_chain_does_not_close(where, status):
    recs = list(CLOSED)
    recs[where] = rec(*recs[where][:2], status=status, final=recs[where][3])
    ok, chain, total, end_bit, last, wp, prev, live = follow(STARTS, recs, TOTAL)
    assert not ok and chain == list(range(where)) and last == where and live == [0, 0, 0]
    assert total == sum(r[1] for r in CLOSED[:where])  # (the span with the status never joined)


def test_no_final_block_does_not_close():
    assert follow(STARTS, [CLOSED[0], CLOSED[1], rec(3001, 123456)], TOTAL)[:3] == (False, [0, 1, 2], TOTAL)
    assert follow([0], [rec(100, 5)], 5)[:2] == (False, [0])
    assert follow([0], [rec(100, 5)], 5)[7] == [0]


def test_one_byte_more_than_the_room_does_not_close():
    assert follow(STARTS, CLOSED, TOTAL)[0]
    ok, chain, total, *_, live = follow(STARTS, CLOSED, TOTAL - 1)
    assert not ok and chain == [0, 1, 2] and total == TOTAL and live == [0, 0, 0]
    # ... wherever on the chain the room ends
    assert follow(STARTS, CLOSED, 70004)[:3] == (False, [0, 1], 70005)
    assert follow(STARTS, CLOSED, 69999)[:3] == (False, [0], 70000)
    assert follow(STARTS, CLOSED, 1 << 62)[0]


def test_a_sum_that_wraps_does_not_close():
    recs = [CLOSED[0], rec(2400, (1 << 64) - 10), CLOSED[2]]  # 70000 + 2^64 - 10 = 69990 in 64 bits
    ok, chain, *_ = follow(STARTS, recs, TOTAL)
    assert not ok and chain == [0, 1]
    assert not follow([0], [rec(5, NONE, final=1)], NONE - 1)[0]
    assert follow([0], [rec(5, NONE, final=1)], NONE)[0]  # (no wrap: as much room as bytes)


def test_history_before_the_first_32_KiB_of_output_is_the_old_paths_when_run_b_is_in_run_as_launch():
    def recs(first_len, hist0=0):
        return [rec(1000, first_len, hist=hist0), rec(2400, 5, hist=1), rec(3001, 7, final=1)]

    assert follow(STARTS, recs(TAIL), 1 << 20, both=True)[:2] == (True, [0, 1, 2])
    ok, chain, total, end_bit, last, wp, prev, live = follow(STARTS, recs(TAIL - 1), 1 << 20, both=True)
    assert not ok and chain == [0] and last == 1 and total == TAIL - 1 and live == [0, 0, 0]
    # two launches: run B is given its place
    assert follow(STARTS, recs(TAIL - 1), 1 << 20, both=False)[:2] == (True, [0, 1, 2])
    assert follow(STARTS, recs(0), 1 << 20, both=False)[0]
    # the first span has no history to reach into (a copy that does is an error run A saw)
    assert follow(STARTS, recs(TAIL, hist0=1), 1 << 20, both=True)[0]
    # a span without such copies may start anywhere
    assert follow(STARTS, [rec(1000, 1), rec(2400, 5), rec(3001, 7, final=1)], 1 << 20, both=True)[0]
    # the rule looks at every span behind the first: the third one at 32767 bytes
    third = [rec(1000, TAIL - 6), rec(2400, 5), rec(3001, 7, hist=1, final=1)]
    assert not follow(STARTS, third, 1 << 20, both=True)[0]
    third[1] = rec(2400, 6)
    assert follow(STARTS, third, 1 << 20, both=True)[0]


def test_a_record_that_points_at_or_before_its_own_span_ends_the_walk():
    # at itself
    ok, chain, *_, last, wp, prev, live = follow(STARTS, [CLOSED[0], rec(1000, 5), CLOSED[2]], TOTAL)
    assert not ok and chain == [0, 1] and live == [0, 0, 0]
    # at a span before it (a dead one, and the stream's first)
    starts = [0, 500, 1000, 2400]
    back = [CLOSED[0], rec(1000, 1), rec(500, 5), CLOSED[2]]
    assert follow(starts, back, TOTAL)[:2] == (False, [0, 2])
    back[2] = rec(0, 5)
    assert follow(starts, back, TOTAL)[:2] == (False, [0, 2])
    # the first span at itself
    assert follow(STARTS, [rec(0, 5), CLOSED[1], CLOSED[2]], TOTAL)[:2] == (False, [0])
    # two spans that name each other
    assert follow(STARTS, [rec(2400, 5), rec(2400, 5), rec(1000, 5)], TOTAL)[:2] == (False, [0, 2])


# ---------------------------------------------------------------- the work items of k_span_fix

def fix_items(streams, both):
    """streams: [(out_off, out_cap, starts, recs)] -> dict"""
    n_el = len(streams)
    sp_first = [0]
    for s in streams:
        sp_first.append(sp_first[-1] + len(s[2]))
    nsp = sp_first[-1]
    sp = u64(x for s in streams for i, st in enumerate(s[2]) for x in (st, 0, 1 if i == 0 else 0, NO_SPAN, 0))
    rc = u64(x for s in streams for r in s[3] for x in r)
    cap = 256
    ok, items, item_first = np.zeros(n_el, np.int32), np.zeros(7 * cap, np.uint64), np.zeros(n_el + 1, np.uint32)
    chain_all, chain_off, chain_pos = np.zeros(nsp, np.uint32), np.zeros(n_el + 1, np.uint32), np.zeros(nsp, np.uint32)
    misc = np.zeros(3, np.uint64)
    offs, caps, firsts = u64(s[0] for s in streams), u64(s[1] for s in streams), u32(sp_first)
    lib().shim_span_fix_items(offs.ctypes.data, caps.ctypes.data, n_el,
                              firsts.ctypes.data, sp.ctypes.data, rc.ctypes.data, int(both), ok.ctypes.data, items.ctypes.data,
                              cap, item_first.ctypes.data, chain_all.ctypes.data, chain_off.ctypes.data, chain_pos.ctypes.data,
                              misc.ctypes.data)
    n_items = int(misc[0])
    assert n_items <= cap
    n_chain = int(chain_off[n_el])
    keys = ("dst", "span", "local", "len", "kind", "prev", "pad")
    return dict(ok=[int(x) for x in ok], items=[dict(zip(keys, (int(x) for x in items[7 * i:7 * i + 7]))) for i in range(n_items)],
                item_first=[int(x) for x in item_first], chain_all=[int(x) for x in chain_all[:n_chain]],
                chain_off=[int(x) for x in chain_off], chain_pos=[int(x) for x in chain_pos[:n_chain]], longest=int(misc[1]),
                uses_hist=bool(misc[2]), nsp=nsp)


# four spans of ITEM + 1, 0, ITEM and 5 bytes
FOUR_STARTS = [0, 800, 1600, 2400]


def four(hist=0):
    return [rec(800, ITEM + 1), rec(1600, 0), rec(2400, ITEM, hist=hist), rec(3000, 5, final=1)]


@pytest.mark.parametrize("both,hist,kind", [(False, 0, 1), (True, 0, 1), (False, 1, 2), (True, 1, 3)])
def test_items_of_one_stream(both, hist, kind):
    f = fix_items([(1000, 1 << 20, FOUR_STARTS, four(hist))], both)
    assert f["ok"] == [1] and f["uses_hist"] == bool(hist)
    assert f["chain_all"] == [0, 1, 2, 3] and f["chain_off"] == [0, 4] and f["chain_pos"] == [0, 1, 2, 3] and f["longest"] == 4
    it = f["items"]
    # ITEM + 1 bytes: two items and two empty ones; 0 bytes: none at all; ITEM bytes: one and three; 5 bytes: one and three
    assert f["item_first"] == [0, 12] and len(it) == 12
    assert [(i["span"], i["local"], i["len"]) for i in it] == [
        (0, 0, ITEM), (0, ITEM, 1), (0, 0, 0), (0, 0, 0),
        (2, 0, ITEM), (2, 0, 0), (2, 0, 0), (2, 0, 0),
        (3, 0, 5), (3, 0, 0), (3, 0, 0), (3, 0, 0)]
    # dst = out_off + wp + local; wp = the bytes of the spans before
    assert [i["dst"] for i in it if i["len"]] == [1000, 1000 + ITEM, 1000 + ITEM + 1, 1000 + 2 * ITEM + 1]
    # a first span's bytes are in place and final; the others: final in the pool (no span of the batch reaches into its history),
    # or run B's in place (two launches), or both in the pool (one launch) -- empty items as the span they fill
    assert [i["kind"] for i in it] == [0] * 4 + [kind] * 8
    assert [i["prev"] for i in it] == [NO_SPAN] * 4 + [1] * 4 + [2] * 4
    assert all(i["pad"] == (4 if both else 0) for i in it)


def test_items_of_a_batch():
    """three streams: the middle one's chain does not close (its copies into the history do not count, it gets no items);
    the third has two spans of 3 ITEM and ITEM - 1 bytes"""
    third = [rec(640, 3 * ITEM), rec(900, ITEM - 1, final=1)]
    f = fix_items([(1000, 1 << 20, FOUR_STARTS, four()),
                   (1 << 21, 1 << 20, [0, 100], [rec(100, 7, hist=1), rec(200, 7, status=3, hist=1)]),
                   (1 << 22, 1 << 20, [0, 640], third)], True)
    assert f["ok"] == [1, 0, 1] and not f["uses_hist"] and f["nsp"] == 8
    assert f["chain_all"] == [0, 1, 2, 3, 6, 7] and f["chain_off"] == [0, 4, 4, 6]
    assert f["chain_pos"] == [0, 1, 2, 3, 0, 1] and f["longest"] == 4
    assert f["item_first"] == [0, 12, 12, 20]
    tail = f["items"][12:]
    assert [(i["span"], i["local"], i["len"], i["kind"], i["prev"]) for i in tail] == [
        (6, 0, ITEM, 0, NO_SPAN), (6, ITEM, ITEM, 0, NO_SPAN), (6, 2 * ITEM, ITEM, 0, NO_SPAN), (6, 0, 0, 0, NO_SPAN),
        (7, 0, ITEM - 1, 1, 6), (7, 0, 0, 1, 6), (7, 0, 0, 1, 6), (7, 0, 0, 1, 6)]
    assert [i["dst"] - (1 << 22) for i in tail if i["len"]] == [0, ITEM, 2 * ITEM, 3 * ITEM]
    assert all(i["pad"] == 8 for i in f["items"])
    # one span anywhere on a live chain that reaches into its history: every span behind a first one has two versions
    third[1] = rec(900, ITEM - 1, final=1, hist=1)
    g = fix_items([(1000, 1 << 20, FOUR_STARTS, four()), (1 << 22, 1 << 20, [0, 640], third)], True)
    assert g["uses_hist"] and [i["kind"] for i in g["items"]] == [0] * 4 + [3] * 8 + [0] * 4 + [3] * 4
    # no chain closes: nothing to do
    h = fix_items([(0, 10, [0, 100], [rec(100, 7), rec(200, 7, final=1)])], False)
    assert h["ok"] == [0] and h["items"] == [] and h["item_first"] == [0, 0] and h["chain_all"] == [] and h["chain_off"] == [0, 0]


# ---------------------------------------------------------------- the checksum fold and the footer

def parts_of(data, span_lens, container):
    """What k_span_fix reports for the items of a stream whose spans make span_lens bytes: for every item its length and
    -- gzip -- the CRC-32 of its bytes, which the kernel puts together from its lanes' CRC-32s (each from 0xffffffff,
    inverted at the end, an empty lane's 0) times x^(8 * bytes behind the lane): the CRC-32 as zlib defines it, 0 for an
    empty item; -- zlib -- the sums A (of the bytes) and B (of the running A) from A = B = 0, mod 65521, as A | B << 16.
    zlib.adler32 starts at A = 1: it says A + 1 and B + len."""
    parts, at = [], 0
    for n in span_lens:
        k = 0
        for o in range(0, n, ITEM):
            piece = data[at + o:at + min(n, o + ITEM)]
            if container == 1:
                pc = zlib.crc32(piece)
            else:
                ad = zlib.adler32(piece)
                pc = ((ad & 0xffff) - 1) % 65521 | ((((ad >> 16) - len(piece)) % 65521) << 16)
            parts += [pc, len(piece)]
            k += 1
        while k % WAVES:
            parts += [0, 0]
            k += 1
        at += n
    assert at == len(data)
    return parts


def verify(span_lens, parts, container, foot, in_len, end_bit, total=None, r2=None, uses_hist=False):
    nsp = len(span_lens)
    ra = [rec(100 * (i + 1), n) for i, n in enumerate(span_lens)]
    rb = ra if r2 is None else r2
    res = np.zeros(3, np.uint64)
    p = u32(parts)
    f = np.frombuffer(bytes(foot).ljust(8, b"\0"), np.uint8).copy()
    chain, first = u32(range(nsp)), u32([1] + [0] * (nsp - 1))
    a6, b6 = u64(x for r in ra for x in r), u64(x for r in rb for x in r)
    ok = lib().shim_span_verify(chain.ctypes.data, nsp, sum(span_lens) if total is None else total, end_bit, first.ctypes.data,
                                a6.ctypes.data, b6.ctypes.data, nsp, int(uses_hist), p.ctypes.data, len(parts) // 2, container,
                                f.ctypes.data, in_len, res.ctypes.data)
    return bool(ok), int(res[0]), int(res[1]), int(res[2])


def test_the_adler_parts_are_the_sums_from_zero():
    """the reading of zlib.adler32 that parts_of relies on, against the sums themselves"""
    piece = random.Random(5).randbytes(ITEM)
    v = np.frombuffer(piece, np.uint8).astype(np.uint64)
    a, b = int(v.sum()) % 65521, int((v * np.arange(ITEM, 0, -1, dtype=np.uint64)).sum()) % 65521
    assert parts_of(piece, [ITEM], 2)[:2] == [a | (b << 16), ITEM]


DATA = random.Random(2024).randbytes(3 * ITEM + 1)
# (the stream's last item has 1 byte, ITEM bytes, something in between; one span, or two that split an item)
SPLITS = [(DATA, [3 * ITEM + 1]), (DATA[:3 * ITEM], [3 * ITEM]), (DATA, [ITEM + 100, 2 * ITEM - 99]), (DATA[:-9], [1, 3 * ITEM - 9]),
          (DATA[:ITEM], [0, ITEM, 0])]
END_BYTE = 5000  # the final block ends in this byte of the stream


@pytest.mark.parametrize("data,span_lens", SPLITS)
def test_the_gzip_footer(data, span_lens):
    parts = parts_of(data, span_lens, 1)
    foot = struct.pack("<II", zlib.crc32(data), len(data))
    for end_bit in (8 * END_BYTE - 7, 8 * END_BYTE - 3, 8 * END_BYTE):
        assert verify(span_lens, parts, 1, foot, END_BYTE + 8, end_bit) == (True, END_BYTE + 8, zlib.crc32(data), NO_SPAN)
    assert verify(span_lens, parts, 1, foot, END_BYTE + 100, 8 * END_BYTE)[:2] == (True, END_BYTE + 8)  # (bytes behind the member)
    # the footer ends one byte behind the stream
    assert verify(span_lens, parts, 1, foot, END_BYTE + 7, 8 * END_BYTE)[0] is False
    assert verify(span_lens, parts, 1, foot, END_BYTE + 8, 8 * END_BYTE + 1)[0] is False
    # one bit of the footer
    for bit in (0, 7, 13, 31, 32, 40, 63):
        bad = bytearray(foot)
        bad[bit // 8] ^= 1 << (bit % 8)
        assert verify(span_lens, parts, 1, bad, END_BYTE + 8, 8 * END_BYTE)[0] is False, bit
    # ISIZE
    assert verify(span_lens, parts, 1, struct.pack("<II", zlib.crc32(data), len(data) + 1), END_BYTE + 8, 8 * END_BYTE)[0] is False
    assert verify(span_lens, parts, 1, foot, END_BYTE + 8, 8 * END_BYTE, total=len(data) + (1 << 32))[0] is True  # (ISIZE is mod 2^32)
    # one bit of one part
    bad = list(parts)
    bad[0] ^= 0x400
    assert verify(span_lens, bad, 1, foot, END_BYTE + 8, 8 * END_BYTE)[0] is False
    # two items the other way round (random bytes: no two items are alike)
    full = [q for q in range(0, len(parts), 2) if parts[q + 1]]
    if len(full) > 1:
        bad, (i, j) = list(parts), full[:2]
        bad[i:i + 2], bad[j:j + 2] = parts[j:j + 2], parts[i:i + 2]
        assert verify(span_lens, bad, 1, foot, END_BYTE + 8, 8 * END_BYTE)[0] is False


@pytest.mark.parametrize("data,span_lens", SPLITS)
def test_the_zlib_footer(data, span_lens):
    parts = parts_of(data, span_lens, 2)
    foot = struct.pack(">I", zlib.adler32(data))
    assert verify(span_lens, parts, 2, foot, END_BYTE + 4, 8 * END_BYTE - 3) == (True, END_BYTE + 4, 0, NO_SPAN)
    assert verify(span_lens, parts, 2, foot, END_BYTE + 3, 8 * END_BYTE)[0] is False
    for bit in (0, 9, 16, 31):
        bad = bytearray(foot)
        bad[bit // 8] ^= 1 << (bit % 8)
        assert verify(span_lens, parts, 2, bad, END_BYTE + 4, 8 * END_BYTE)[0] is False, bit
    # the little-endian reading is not taken
    if foot != foot[::-1]:
        assert verify(span_lens, parts, 2, foot[::-1], END_BYTE + 4, 8 * END_BYTE)[0] is False
    # the total enters the second sum
    assert verify(span_lens, parts, 2, foot, END_BYTE + 4, 8 * END_BYTE, total=len(data) + 1)[0] is False
    assert verify(span_lens, parts, 2, foot, END_BYTE + 4, 8 * END_BYTE, total=len(data) + 65521)[0] is True


def test_adler_at_its_largest_sums():
    """0xff bytes: A and B pass 65521 many times within an item, and between the items"""
    data = b"\xff" * (3 * ITEM + 1)
    parts = parts_of(data, [2 * ITEM, ITEM + 1], 2)
    assert verify([2 * ITEM, ITEM + 1], parts, 2, struct.pack(">I", zlib.adler32(data)), 104, 800)[0] is True


def test_a_raw_stream_has_no_footer():
    assert verify([5], [], 0, b"", 700, 8 * 700 - 2) == (True, 700, 0, NO_SPAN)
    assert verify([5], [], 0, b"", 699, 8 * 700 - 2)[0] is False


def test_run_b_must_say_what_run_a_said():
    data, span_lens = DATA, [ITEM, ITEM, ITEM + 1]
    parts = parts_of(data, span_lens, 1)
    foot = struct.pack("<II", zlib.crc32(data), len(data))
    ra = [rec(100 * (i + 1), n) for i, n in enumerate(span_lens)]
    args = (span_lens, parts, 1, foot, END_BYTE + 8, 8 * END_BYTE)
    for where, other in [(1, rec(200, ITEM + 1)), (1, rec(201, ITEM)), (2, rec(300, ITEM + 1, status=5)), (2, rec(300, 0))]:
        rb = list(ra)
        rb[where] = other
        # (the fold is not reached: crc 0)
        assert verify(*args, r2=rb, uses_hist=True) == (False, END_BYTE + 8, 0, where)
        # no span reached into its history: there was no run B to compare
        assert verify(*args, r2=rb, uses_hist=False)[0] is True
    # what only run A knows, and the first span, whose run A was final
    rb = [rec(1, 1, status=9)] + [rec(r[0], r[1], final=1, hist=1, pieces=9) for r in ra[1:]]
    assert verify(*args, r2=rb, uses_hist=True)[0] is True


# ---------------------------------------------------------------- random and hostile records under the sanitizers

def test_random_and_hostile_records_under_the_sanitizers():
    """tests/host_cpp/test_span_plan.cpp: a program of its own, built with AddressSanitizer and UBSan, that walks, plans and
    verifies a few thousand random record sets (end_bit anywhere, lengths up to 2^64 - 1, any status).  It checks that
    every call returns and every index it hands out is inside its array; what the calls decide is this file's business."""
    src = os.path.join(ROOT, "tests", "host_cpp", "test_span_plan.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_span_plan")
    if not newer(exe, [src] + DEPS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-o", exe, src],
                       check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
