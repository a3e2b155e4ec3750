"""The rules by which flate_hip_decompress_members follows a stream's chain of members (flate_amd/csrc/member_plan.h), on
the CPU: hand-made candidate tables -- positions with the probe's (status, consumed, size) -- against a restatement of
the loop a caller writes.  The shim (tests/cpu_shim/member_plan_shim.cpp) compiles the text the kernels run.  No GPU."""
import random

import pytest

import _member_plan as M


def loop(cands, start, end):
    """the caller's loop over a stream whose bytes read 1f 8b 08 exactly at the candidates' positions:
    ([(member start relative to the stream, size)] with the failing remainder last, status, members decoded)"""
    at, table, by_pos = start, [], {c[0]: c for c in cands}
    while True:
        if at not in by_pos:  # fl_inf_header: 10 bytes are read before the magic is compared
            return table + [(at - start, 0)], (1 if end - at < 10 else 2), len(table)
        _, status, used, size = by_pos[at]
        table.append((at - start, size))
        if status != 0:
            return table, status, len(table) - 1
        at += used
        if at == end:
            return table, 0, len(table)


def check(cands, start, end):
    table, status, members = loop(cands, start, end)
    got_table, got_status, on = M.chain(cands, start, end)
    assert got_status == status
    assert [t[0] for t in got_table] == [t[0] for t in table]
    # (the size of a failing last entry is not looked at: its slot is the rest)
    assert got_table[:members] == table[:members]
    assert on == len([t for t in table if start + t[0] in {c[0] for c in cands}])
    return got_table, got_status


def test_constants():
    assert M.scan_tile() % 1024 == 0 and M.scan_tile() >= 1024
    assert M.lds_tile() >= 64
    assert [M.least_bytes(c) for c in (0, 1, 2)] == [2, 20, 8]
    assert [M.lib().shim_member_miss_status(k) for k in (0, 3, 9, 10, 11, 1000)] == [1, 1, 1, 2, 2, 2]


def test_chain_skips_false_candidates():
    # members at 100, 150, 230; false candidates at 120 (refused) and 160 (probes clean, ends inside the third member)
    cands = [(100, 0, 50, 7), (120, 7, 3, 0), (150, 0, 80, 9), (160, 0, 30, 5), (230, 0, 70, 11)]
    table, status = check(cands, 100, 300)
    assert status == 0 and table == [(0, 7), (50, 9), (130, 11)]


@pytest.mark.parametrize("left", [9, 10])
def test_chain_lands_on_a_non_candidate(left):
    end = 1000
    cands = [(0, 0, 400, 1), (400, 0, end - left - 400, 2), (end - left + 1, 0, 5, 3)]
    table, status = check(cands, 0, end)
    assert status == (1 if left == 9 else 2)
    assert table == [(0, 1), (400, 2), (end - left, 0)]


def test_error_in_the_middle():
    cands = [(10, 0, 30, 4), (40, 11, 17, 99), (70, 0, 30, 4)]
    table, status = check(cands, 10, 100)
    assert status == 11 and [t[0] for t in table] == [0, 30]


def test_zero_candidates():
    assert check([], 5, 5) == ([(0, 0)], 1)      # an empty stream: EndOfStream
    assert check([], 5, 14) == ([(0, 0)], 1)
    assert check([], 5, 15) == ([(0, 0)], 2)
    # candidates, but none at the stream's first byte
    assert check([(6, 0, 20, 1)], 5, 26) == ([(0, 0)], 2)


def test_successor_exactly_at_the_stream_end():
    cands = [(0, 0, 64, 10), (64, 0, 36, 20)]
    assert check(cands, 0, 100) == ([(0, 10), (64, 20)], 0)
    # ... and one byte short of it: a remainder of one byte
    assert check(cands, 0, 101) == ([(0, 10), (64, 20), (100, 0)], 1)


@pytest.mark.parametrize("members", [70, 5000])
def test_long_chains(members):
    """70 members are more than a wave's lanes, 5000 are past one tile of successors; between any two members lie false
    candidates, so that the chain's indices run away from its count"""
    assert members < M.lds_tile() or members > 2 * M.lds_tile()
    rng = random.Random(members)
    cands, at = [], 0
    for k in range(members):
        used = rng.randrange(20, 90)
        cands.append((at, 0, used, k + 1))
        for f in sorted(rng.sample(range(at + 1, at + used), rng.randrange(0, 3))):
            cands.append((f, rng.choice([0, 0, 7, 11]), rng.randrange(1, 40), 12345))
        at += used
    table, status = check(cands, 0, at)
    assert status == 0 and len(table) == members and [t[1] for t in table] == list(range(1, members + 1))
    # the same chain cut short by an error at its last member
    last = max(i for i, c in enumerate(cands) if c[3] == members)
    cands[last] = (cands[last][0], 13, 0, 0)
    table, status = check(cands, 0, at)
    assert status == 13 and len(table) == members


def test_a_stream_inside_a_batch():
    """positions are absolute: a stream that starts at 1000 sees only its own candidates"""
    cands = [(1000, 0, 40, 1), (1040, 0, 60, 2)]
    assert check(cands, 1000, 1100) == ([(0, 1), (40, 2)], 0)
    assert M.stream_of([0, 10, 10, 30], 0) == 0
    assert M.stream_of([0, 10, 10, 30], 9) == 0
    assert M.stream_of([0, 10, 10, 30], 10) == 2     # the empty stream holds no byte
    assert M.stream_of([0, 10, 10, 30], 29) == 2
    assert M.stream_of([7, 8], 7) == 0


def test_slots():
    assert M.slots([10, 0, 5], 100, 200) == [100, 110, 110]
    assert M.slots([10, 95, 5], 100, 200) == [100, 110, 200]   # clamped to the stream's slot
    assert M.slots([3 << 32, 1], 0, 1 << 40) == [0, 3 << 32]
    assert M.slots([7], 50, 50) == [50]
