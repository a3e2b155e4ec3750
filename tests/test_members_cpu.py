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


# ---------------------------------------------------------------- the host's side of the call (member_plan.h)

TILE = 16384


@pytest.mark.parametrize("residue", range(16))
def test_scan_tiles_at_every_residue_of_the_address(residue):
    """a lane reads 16 bytes at a multiple of 16: the first tile starts up to 15 bytes before the first input byte"""
    assert M.scan_tile() == TILE
    base = 0x7f0000001000 + residue
    for lo in (0, 3, 100):
        back = (base + lo) & 15
        rel0 = lo - back                                  # negative where lo < back
        for k in (1, 2):
            assert M.scan_tiles(base, lo, rel0 + k * TILE - 1) == (rel0, k)
            assert M.scan_tiles(base, lo, rel0 + k * TILE) == (rel0, k)
            assert M.scan_tiles(base, lo, rel0 + k * TILE + 1) == (rel0, k + 1)
        assert M.scan_tiles(base, lo, lo + 1) == (rel0, 1)


def test_scan_tiles_bound():
    most = 0x7fffffff
    assert M.scan_tiles(0x1000, 0, most * TILE) == (0, most)
    assert M.scan_tiles(0x1000, 0, most * TILE + 1) is None
    assert M.scan_tiles(0x1001, 16, most * TILE + 1) == (15, most)     # (the tiles start at 15)
    assert M.scan_tiles(0x1001, 16, most * TILE + 16) is None


@pytest.mark.parametrize("container, least, toff", [
    (0, 2, [0, 52, 54, 76]),      # 100 / 2 + 2, 0 / 2 + 2, 41 / 2 + 2
    (1, 20, [0, 7, 9, 13]),       # 100 / 20 + 2, 2, 41 / 20 + 2
    (2, 8, [0, 14, 16, 23]),      # 100 / 8 + 2, 2, 41 / 8 + 2
])
def test_table_capacities(container, least, toff):
    assert M.least_bytes(container) == least
    # walk: a table per stream, side by side; the offsets of the streams in the caller's buffer do not matter
    assert M.walk_offsets([0, 100, 100, 141], container) == (toff, toff[-1])
    assert M.walk_offsets([1000, 1100, 1100, 1141], container) == (toff, toff[-1])
    # ... a stream of k smallest members and some bytes more holds them and the failing remainder
    for k in (1, 7, 1000):
        assert M.walk_offsets([0, k * least + least - 1], container)[1] == k + 2
    # scan: every candidate on at most one chain, one entry more per stream
    assert M.scan_cap(0, 3) == 3 and M.scan_cap(10, 3) == 13 and M.scan_cap(1 << 22, 0xffffffff) == (1 << 22) + 0xffffffff


def test_member_count_that_came_back():
    assert M.count_ok(2, 2, 10) and M.count_ok(10, 2, 10)
    assert not M.count_ok(1, 2, 10)                       # a stream without an entry
    assert not M.count_ok(11, 2, 10)                      # more than the tables hold
    assert M.count_ok(0xfffffff0, 1, 1 << 40) and not M.count_ok(0xfffffff1, 1, 1 << 40)


VIN, VOUT = [0, 100, 250], [1000, 2000, 2600]


def test_partition_of_a_good_table():
    fault, _, min_, mout = M.partition([0, 2, 3], [0, 40, 0], [300, 9999, 50], VIN, VOUT)
    assert fault == M.OK
    assert min_ == [0, 40, 100, 250]
    assert mout == [1000, 1300, 2000, 2600]
    # a member may start at its stream's end (an empty remainder), and a member's size is clamped to the stream's slot
    fault, _, min_, mout = M.partition([0, 3, 4], [0, 40, 100, 0], [999, 999, 0, 1], VIN, VOUT)
    assert fault == M.OK and min_ == [0, 40, 100, 100, 250] and mout == [1000, 1999, 2000, 2000, 2600]


@pytest.mark.parametrize("doff, mstart, fault, stream", [
    ([0, 2, 2], [0, 40], 1, 1),                 # a stream with 0 members (the last one: nothing behind the table is read)
    ([0, 0, 2], [0, 40], 1, 0),
    ([0, 2, 3], [0, 40, 5], 1, 1),              # a first start that is not 0
    ([0, 2, 3], [1, 40, 0], 1, 0),
    ([0, 3, 4], [0, 40, 39, 0], 2, 0),          # a start that goes backwards
    ([0, 1, 4], [0, 0, 20, 19], 2, 1),
    ([0, 2, 3], [0, 101, 0], 2, 0),             # a start beyond the stream (100 bytes)
    ([0, 1, 3], [0, 0, 151], 2, 1),
    ([0, 3, 3], [0, 40, 39], 2, 0),             # two bad streams: the first is named
    ([0, 2, 4], [0, 101, 7, 8], 2, 0),
])
def test_partition_refuses_hostile_tables(doff, mstart, fault, stream):
    assert (M.NO_FIRST, M.ORDER) == (1, 2)
    assert M.partition(doff, mstart, [10] * len(mstart), VIN, VOUT)[:2] == (fault, stream)


def test_slots():
    assert M.slots([10, 0, 5], 100, 200) == [100, 110, 110]
    assert M.slots([10, 95, 5], 100, 200) == [100, 110, 200]   # clamped to the stream's slot
    assert M.slots([3 << 32, 1], 0, 1 << 40) == [0, 3 << 32]
    assert M.slots([7], 50, 50) == [50]
