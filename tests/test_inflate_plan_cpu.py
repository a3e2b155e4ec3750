"""The host decisions of the inflate entry points (flate_amd/csrc/inflate_plan.h) on the CPU: the chunk table, which LDS
ring a launch gets, when a pinned host call runs in sub-batches and how large they are, when k_inflate_par runs, when the
span pool is given back, how a host caller's output comes home, and the rules of the resumable inflater's host feeds.  The shim (tests/cpu_shim/inflate_plan_shim.cpp) is
built the way tests/test_span_plan_cpu.py builds its own, without a sanitizer; tests/host_cpp/test_inflate_plan.cpp runs the
same functions over random and hostile inputs under AddressSanitizer and UBSan (tests/test_host_cpp.py).  No GPU.

Every expected value below is worked out by hand from the rule as inflate_plan.h states it."""
import pytest

import _inflate_plan as P

SMALL, LARGE, MAX_IN = 2048, 32768, 0xfffffff0
MIB = 1 << 20


def test_the_constants_are_the_ones_this_file_reasons_with():
    assert P.consts() == (SMALL, LARGE, MAX_IN)


# ---------------------------------------------------------------- the LDS ring

@pytest.mark.parametrize("knob, n, large", [
    (-1, 1024, True), (-1, 1025, False),            # unset: up to 4 * 256 streams get the large ring
    (0, 1024, False), (0, 1025, False),             # a knob below the large ring's size: the small one, whatever the count
    (SMALL, 1024, False), (SMALL, 1025, False),
    (LARGE, 1024, True), (LARGE, 1025, True),       # from the large ring's size on: the large one
    (LARGE - 1, 1, False), (-1, 1, True), (-1, 0xffffffff, False),
])
def test_ring(knob, n, large):
    assert P.ring_large(knob, n) is large


# ---------------------------------------------------------------- pinned overlap

def test_pin_io_every_condition_at_its_edge():
    in_bytes, n = 1000, 4097
    at_most = 8 * in_bytes + MIB    # 1056576
    assert P.pin_io(True, True, in_bytes, at_most, n) is True
    assert P.pin_io(False, True, in_bytes, at_most, n) is False
    assert P.pin_io(True, False, in_bytes, at_most, n) is False
    assert P.pin_io(True, True, in_bytes, at_most + 1, n) is False
    assert P.pin_io(True, True, in_bytes + 1, at_most + 1, n) is True      # eight bytes of room more
    assert P.pin_io(True, True, in_bytes, at_most, 4096) is False          # 4 * 1024: not above it
    assert P.pin_io(True, True, 0, MIB, n) is True                         # nothing goes in: the slack alone
    assert P.pin_io(True, True, 0, MIB + 1, n) is False
    # FLATE_HIP_HOST_PASS_CHUNKS=2
    assert P.pin_io(True, True, in_bytes, at_most, 8, 2) is False
    assert P.pin_io(True, True, in_bytes, at_most, 9, 2) is True


@pytest.mark.parametrize("n, knob, sizes", [
    (4097, 1024, [4097]),                       # 4097 // 3072 = 1 sub-batch (never 4096 + 1)
    (6145, 1024, [3073, 3072]),                 # 6145 // 3072 = 2: ceil(6145 / 2) = 3073
    (6146, 1024, [3073, 3073]),
    (16385, 1024, [3277] * 5),                  # 16385 // 3072 = 5: ceil(16385 / 5) = 3277, 5 * 3277 = 16385
    (9, 2, [9]),                                # 9 // 6 = 1
    (20, 2, [7, 7, 6]),                         # 20 // 6 = 3: ceil(20 / 3) = 7
])
def test_sub_batches(n, knob, sizes):
    got = P.sub_batches(n, knob)
    assert got == sizes
    assert sum(got) == n and min(got) > 0 and len(set(got[:-1])) <= 1 and got[-1] <= got[0]


def test_sub_batch_below_one_target():
    assert P.sub_batches(5, 1024) == [5]        # (the rule is asked only above 4 passes; it still answers)
    assert P.sub_batches(1, 1) == [1]


# ---------------------------------------------------------------- k_inflate_par

def test_par_knob():
    big = [(40000, 0)]
    assert P.par(big) == (True, 32768, 1, 1)
    assert P.par(big, knob=0) == (False, 0, 1, 0)                 # 0: never
    assert P.par(big, knob=40001) == (False, 40001, 0, 0)         # the knob is the minimum size
    assert P.par(big, knob=40000) == (True, 40000, 1, 1)
    assert P.par([(32767, 0)]) == (False, 32768, 0, 0)
    assert P.par([(32768, 0)]) == (True, 32768, 1, 1)


def test_par_count_of_long_streams():
    small = [(100, 1000)] * 3
    assert P.par([(32768, 0)] * 2048 + small) == (True, 32768, 2048, 2051)   # taken: every stream of the launch
    assert P.par([(32768, 0)] * 2049 + small) == (False, 32768, 2049, 0)
    assert P.par(small) == (False, 32768, 0, 0)


def test_par_long_by_its_slot_alone():
    assert P.par([(100, 16 * 32768)]) == (True, 32768, 1, 1)
    assert P.par([(100, 16 * 32768 - 1)]) == (False, 32768, 0, 0)
    assert P.par([(100, 16 * 1000)], knob=1000) == (True, 1000, 1, 1)


def test_par_flag_bit_and_skipped_streams():
    big = [(40000, 0)]
    assert P.par(big, flags=1) == (False, 32768, 1, 0)            # the strict header: never
    assert P.par(big, flags=2) == (True, 32768, 1, 1)
    # what the spans finished is skipped: counted as long (the rule looks at sizes), not as taken
    assert P.par([(40000, 0, 1), (40000, 0, 0), (10, 0, 0)]) == (True, 32768, 2, 2)


# ---------------------------------------------------------------- the chunk table

def test_chunk_table_with_shifts_and_an_empty_stream():
    hin, hout = [100, 150, 150, 400], [1000, 1010, 1010, 5000]
    assert P.chunks(hin, hout, 100, 1000) == [(0, 0, 10, 50), (50, 10, 0, 0), (50, 10, 3990, 250)]
    assert P.chunks(hin, hout) == [(100, 1000, 10, 50), (150, 1010, 0, 0), (150, 1010, 3990, 250)]
    # no slots (the size probe, the index walk)
    assert P.chunks(hin, None, 100) == [(0, 0, 0, 50), (50, 0, 0, 0), (50, 0, 0, 250)]
    assert P.chunks([7]) == []


def test_chunk_table_at_the_length_limit():
    assert P.chunks([0, MAX_IN], [0, 1]) == [(0, 0, 1, MAX_IN)]
    assert P.chunks([0, MAX_IN + 1], [0, 1]) is None
    assert P.oversize([0, MAX_IN]) == 1                          # none: n
    assert P.oversize([0, MAX_IN + 1]) == 0
    hin = [5, 5, 10, 10 + MAX_IN, 11 + 2 * MAX_IN, 12 + 2 * MAX_IN]
    assert P.oversize(hin) == 3                                  # the first that is too long
    assert P.chunks(hin) is None
    assert P.chunks(hin[:4], None, 5) == [(0, 0, 0, 0), (0, 0, 0, 5), (5, 0, 0, MAX_IN)]


# ---------------------------------------------------------------- the span pool

def test_span_pool_release():
    assert [P.pool_release(b) for b in (0, 2 << 30, (2 << 30) + 1)] == [False, False, True]


# ---------------------------------------------------------------- copy-out

def test_copy_out_nothing():
    assert P.copy_out([100, 200, 300], [0, 0]) == (P.NONE, 0, 0)
    assert P.copy_out([5, 5], [0]) == (P.NONE, 0, 0)               # no slots at all


def test_copy_out_dense_from_half_the_span():
    hout = [100, 200, 300, 400]                                     # a span of 300 bytes
    assert P.copy_out(hout, [50, 50, 50]) == (P.DENSE, 150, 350)    # exactly half: as it is, up to the last produced byte
    assert P.copy_out(hout, [50, 50, 49]) == (P.PACKED, 149, 0)     # one byte under
    assert P.copy_out(hout, [100, 100, 100]) == (P.DENSE, 300, 400)


def test_copy_out_end_from_a_middle_slot():
    # the last slot produced nothing: the copy ends with the middle one's bytes
    assert P.copy_out([0, 100, 200, 210], [5, 100, 0]) == (P.DENSE, 105, 200)
    assert P.copy_out([0, 100, 200, 210], [100, 5, 0]) == (P.DENSE, 105, 105)


# ---------------------------------------------------------------- the resumable inflater's host feeds

def test_inflater_slot_of_a_stream_is_empty_or_holds_the_longest_match():
    piece = [10, 15]                                                # five bytes go in
    assert P.inflater_slots_ok(piece, [0, 0], [0]) is True          # no room: allowed, nothing comes out
    assert P.inflater_slots_ok(piece, [0, 1], [0]) is False
    assert P.inflater_slots_ok(piece, [0, 257], [0]) is False
    assert P.inflater_slots_ok(piece, [0, 258], [0]) is True
    assert P.inflater_slots_ok(piece, [40, 40 + 257], [1]) is False
    assert P.inflater_slots_ok(piece, [40, 40 + 258], [1]) is True
    # an empty piece is a feed all the same when it is final or has a slot
    assert P.inflater_slots_ok([10, 10], [0, 1], [0]) is False
    assert P.inflater_slots_ok([10, 10], [0, 0], [1]) is True
    # a skipped stream (empty piece, not final, empty slot) among others: exempt, and the others are still checked
    assert P.inflater_slots_ok([10, 10, 15], [0, 0, 300], [0, 0]) is True
    assert P.inflater_slots_ok([10, 10, 15], [0, 0, 257], [0, 0]) is False
    assert P.inflater_slots_ok([10, 15, 15], [0, 257, 257], [0, 0]) is False


def test_inflater_offsets_must_ascend():
    assert P.inflater_slots_ok([10, 9], [0, 300], [0]) is False
    assert P.inflater_slots_ok([10, 15, 20], [0, 300, 299], [0, 0]) is False
    assert P.inflater_slots_ok([7], [9], []) is True


def test_inflater_copy_home_choice():
    assert [P.inflater_copy_each(n) for n in (1, 16, 17, 0xffffffff)] == [True, True, False, False]


def test_inflater_rebased_tables():
    assert P.inflater_rebase([100, 150, 150, 400], [1000, 1258, 1258, 5000]) == ([0, 50, 50, 300], [0, 258, 258, 4000])
    assert P.inflater_rebase([0, 5], [0, 300]) == ([0, 5], [0, 300])
    assert P.inflater_rebase([1 << 40], [7]) == ([0], [0])
