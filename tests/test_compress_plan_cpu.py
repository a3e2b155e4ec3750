"""CPU tests of compress_impl's host decisions (flate_amd/csrc/pass_plan.h, through tests/cpu_shim/compress_plan_shim.cpp):
the chunk table with its length limits, the walk that cuts a batch into chunk-path and whole-stream passes, the block
tables of a pass (the simple compressors' flush pieces among them), when a call takes two compute streams and how large
its slices are, and which rows of a pass's slots go home by the rectangle copy.  Every expectation is written out by hand
or comes from a model in plain Python; the tests need offsets only, no data."""
import itertools

import numpy as np
import pytest

import _compress_plan as CP
import _pass_plan as P
from test_pass_plan_cpu import CONFIGS, limit, model

B = CP.FL_BLOCK_BYTES


# ---------------------------------------------------------------- the chunk table

@pytest.mark.parametrize("mode", [1, 6])
@pytest.mark.parametrize("flush", [None, True, False])
def test_chunk_table_fields_and_shifts(mode, flush):
    lens = [0, 1, 65535, 65536]
    caps = [64, 0, 70000, 3]
    hin = [1000 + sum(lens[:i]) for i in range(len(lens) + 1)]
    hout = [5000 + sum(caps[:i]) for i in range(len(caps) + 1)]
    for in_shift, out_shift in [(0, 0), (1000, 5000), (7, 4999)]:
        ok, c = CP.chunk_table(hin, hout, in_shift, out_shift, mode, flush)
        assert ok
        assert [int(x) for x in c["in_off"]] == [h - in_shift for h in hin[:-1]]
        assert [int(x) for x in c["out_off"]] == [h - out_shift for h in hout[:-1]]
        assert [int(x) for x in c["out_cap"]] == caps
        assert [int(x) for x in c["in_len"]] == lens
        assert [int(x) for x in c["unfinished"]] == [1 if flush is False else 0] * 4   # only flush without finish
        for name in ("pos_off", "skip", "piece0", "n_piece", "flush_off", "n_flush", "zone_off", "n_slides", "pad_"):
            assert not c[name].any(), name


@pytest.mark.parametrize("mode,most", [(1, 0xfffffff0), (0, 0xfffffff0), (6, 0xfff00000), (4, 0xfff00000), (9, 0xfff00000)])
def test_chunk_table_length_limits(mode, most):
    """stream positions are 32-bit: exactly at the limit passes, one past it fails, wherever the long input stands"""
    for at in (0, 1, 2):
        for extra, want in ((0, True), (1, False)):
            lens = [5, 5, 5]
            lens[at] = most + extra
            hin = [3 + sum(lens[:i]) for i in range(4)]
            ok, c = CP.chunk_table(hin, [0, 10, 20, 30], 3, 0, mode)
            assert ok is want, (mode, at, extra)
            if ok:
                assert [int(x) for x in c["in_len"]] == lens
    # the levels' limit is the lower one: what they refuse the simple modes take
    assert CP.chunk_table([0, 0xfff00001], [0, 8], mode=1)[0] is True
    assert CP.chunk_table([0, 0xfff00001], [0, 8], mode=6)[0] is False
    # offsets that do not grow are a length beyond every limit
    assert CP.chunk_table([10, 5], [0, 8], mode=1)[0] is False


# ---------------------------------------------------------------- the next pass

def model_sizes(n, host, max_pass, pinned, ramp, planned):
    """test_pass_plan_cpu.model's rule with its runs of whole sub-batches counted, not walked (limits of 1 and 5 chunks
    make thousands of passes): with H = L + L // 2, a pinned pass that starts with `left` >= H chunks takes L, so
    (left - H) // L + 1 passes do; what is left then goes in passes of min(max_pass, left)"""
    pin = pinned and not planned
    L = min(host, max_pass) if pin else max_pass
    if not pin:
        return [L] * (n // L) + ([n % L] if n % L else [])
    sizes, c0 = [], 0
    if ramp and n >= 3 * L:
        for k in range(2):
            sizes.append(min(L, max(64, L >> (2 - k))))
            c0 += sizes[-1]
    H, left = L + L // 2, n - c0
    m = 0 if left < H else (left - H) // L + 1
    sizes += [L] * m
    c0 += m * L
    while c0 < n:
        sizes.append(min(max_pass, n - c0))
        c0 += sizes[-1]
    return sizes


def test_the_counted_model_is_the_walked_one():
    for host, max_pass in CONFIGS:
        for pinned, ramp, planned in COMBOS:
            for n in (1, 2, 63, 64, 100, 191, 192, 193, 500, 1535, 1536, 2559, 3071, 3072, 3073, 4097, 5000):
                assert model_sizes(n, host, max_pass, pinned, ramp, planned) == \
                    [nc for _, nc, _ in model(n, host, max_pass, pinned, ramp, planned)], (n, host, max_pass, pinned, ramp, planned)


COMBOS = [(True, True, False), (True, False, False), (False, True, False), (False, True, True), (True, True, True)]


@pytest.mark.parametrize("host,max_pass", CONFIGS)
@pytest.mark.parametrize("pinned,ramp,planned", COMBOS)
def test_all_chunk_walk_is_the_schedule_for_every_n_up_to_5000(host, max_pass, pinned, ramp, planned):
    """without a chunk table (fl_pass_schedule's case) and with a table of short inputs, at levels and simple modes"""
    kw = dict(host=host, max_pass=max_pass, pinned=pinned, ramp=ramp, planned=planned)
    short = np.full(5000, 65535, dtype=np.uint32)
    for n in range(1, 5001):
        want = np.array(model_sizes(n, host, max_pass, pinned, ramp, planned), dtype=np.uint64)
        for got in (CP.walk(None, n, raw=True, **kw), CP.walk(short[:n], raw=True, mode=6 if n & 1 else 1, **kw)):
            assert np.array_equal(got[:, 1], want), (n, kw)
            assert np.array_equal(got[:, 0], np.cumsum(want) - want) and not got[:, 2].any()
    for n in (1, 1535, 2559, 3072, 4097):
        sched, _ = P.schedule(n, host, max_pass, pinned, ramp, planned)
        assert [(c0, nc) for c0, nc, _ in sched] == [(c0, nc) for c0, nc, _ in CP.walk(None, n, **kw)]


def test_mixed_batches_alternate_kinds_at_the_seam():
    lens = [100, 65535, 65536, 70000, 65535]   # short short | long long | short: 65535 is the last chunk-path length
    for mode in range(4, 10):
        assert CP.walk(lens, mode=mode, pinned=False) == [(0, 2, 0), (2, 2, 1), (4, 1, 0)]
    for mode in (0, 1):   # the simple modes know one kind
        assert CP.walk(lens, mode=mode, pinned=False) == [(0, 5, 0)]
    assert CP.walk([65536, 1, 65536], mode=6, pinned=False) == [(0, 1, 1), (1, 1, 0), (2, 1, 1)]
    # the chunk limit cuts inside a run of one kind, never across kinds
    assert CP.walk([1, 1, 1, 70000, 1], mode=6, pinned=False, max_pass=2) == [(0, 2, 0), (2, 1, 0), (3, 1, 1), (4, 1, 0)]


def test_flush_points_force_the_whole_stream_kind_at_the_levels_only():
    for mode in range(4, 10):
        assert CP.walk([100], mode=mode, pinned=False, flush=True) == [(0, 1, 1)]
        assert CP.walk([0], mode=mode, pinned=False, flush=True) == [(0, 1, 1)]
    for mode in (0, 1):
        assert CP.walk([100], mode=mode, pinned=False, flush=True) == [(0, 1, 0)]
        assert CP.walk([200000], mode=mode, pinned=False, flush=True) == [(0, 1, 0)]


def test_whole_stream_passes_end_at_the_byte_limit():
    two = [100000, 100000]
    assert CP.walk(two, pinned=False, stream_bytes=200000) == [(0, 2, 1)]           # exactly the limit: one pass
    assert CP.walk(two, pinned=False, stream_bytes=199999) == [(0, 1, 1), (1, 1, 1)]
    assert CP.walk(two, pinned=False, stream_bytes=150000) == [(0, 1, 1), (1, 1, 1)]
    # a pass always takes its first stream, however long
    assert CP.walk([300000], pinned=False, stream_bytes=150000) == [(0, 1, 1)]
    assert CP.walk([300000, 70000, 70000, 300000], pinned=False, stream_bytes=150000) == [(0, 1, 1), (1, 2, 1), (3, 1, 1)]
    # the chunk limit does not bind whole-stream passes
    assert CP.walk([70000] * 5, pinned=False, max_pass=2) == [(0, 5, 1)]


def test_pass_index_counts_across_kinds_for_the_ramp():
    """pinned, 1024 a sub-batch, 4001 chunks (>= 3 x 1024: the ramp is on): the long first input is pass 0, so the chunk
    pass behind it is pass 1 -- half a sub-batch, not a quarter -- and pass 2 is past the ramp"""
    lens = [70000] + [1000] * 4000
    assert CP.walk(lens, pinned=True, ramp=True) == [(0, 1, 1), (1, 512, 0), (513, 1024, 0), (1537, 1024, 0), (2561, 1440, 0)]
    assert CP.walk(lens, pinned=True, ramp=False) == [(0, 1, 1), (1, 1024, 0), (1025, 1024, 0), (2049, 1024, 0), (3073, 928, 0)]
    # two long ones first: both ramp slots are used up
    lens = [70000, 1000, 70000] + [1000] * 4000
    assert CP.walk(lens, pinned=True)[:4] == [(0, 1, 1), (1, 1, 0), (2, 1, 1), (3, 1024, 0)]


# ---------------------------------------------------------------- the tables of a pass

def test_level_6_tables_two_blocks_a_chunk():
    c = CP.chunks_of([0, 100, 65535])
    nb, blk, sb, st = CP.pass_tables(c, mode=6)
    assert nb == 6 and blk == [0, 0, 1, 1, 2, 2] and sb == [] and st == (0, 0, 0, 0)
    assert [int(x) for x in c["n_blocks"]] == [2, 2, 2]
    assert [int(x) for x in c["first_block"]] == [0, 2, 4]
    assert [int(x) for x in c["pos_off"]] == [0, CP.FL_CHUNK_STRIDE, 2 * CP.FL_CHUNK_STRIDE]


@pytest.mark.parametrize("mode", [0, 1])
def test_simple_mode_tables_a_block_per_full_buffer_and_one_more(mode):
    c = CP.chunks_of([0, B - 1, B, 2 * B])
    nb, blk, sb, _ = CP.pass_tables(c, mode=mode)
    assert [int(x) for x in c["n_blocks"]] == [1, 1, 2, 3]
    assert [int(x) for x in c["first_block"]] == [0, 1, 2, 4]
    assert nb == 7 and blk == [0, 1, 2, 2, 3, 3, 3] and sb == []
    assert [int(x) for x in c["pos_off"]] == [i * CP.FL_CHUNK_STRIDE for i in range(4)]


FLUSH_CASES = [
    # (n, flush points, finish, the fl_sblock list: (start, len, flags) -- 1 final, 2 the empty stored block of a flush)
    (100, [], True, [(0, 100, 1)]),
    (0, [], True, [(0, 0, 1)]),
    (B, [], True, [(0, B, 0), (B, 0, 1)]),                                   # a full buffer goes out, finish writes an empty block
    (100, [0], True, [(0, 0, 0), (0, 0, 2), (0, 100, 1)]),                   # one point at 0
    (100, [50, 50], True, [(0, 50, 0), (0, 0, 2), (50, 0, 0), (0, 0, 2), (50, 50, 1)]),   # the same point twice
    (100, [100], True, [(0, 100, 0), (0, 0, 2), (100, 0, 1)]),               # a point at n
    (2 * B + 10, [2 * B], True, [(0, B, 0), (B, B, 0), (2 * B, 0, 0), (0, 0, 2), (2 * B, 10, 1)]),  # at a multiple of the buffer
    (100, [100], False, [(0, 100, 0), (0, 0, 2)]),                           # no finish: the stream ends with the marker
    (100, [30, 100], False, [(0, 30, 0), (0, 0, 2), (30, 70, 0), (0, 0, 2)]),
]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,points,finish,want", FLUSH_CASES)
def test_simple_mode_flush_pieces_by_hand(mode, n, points, finish, want):
    c = CP.chunks_of([n])
    nb, blk, sb, st = CP.pass_tables(c, mode=mode, flush=points, finish=finish)
    assert sb == want
    assert nb == len(want) and blk == [0] * len(want) and st == (0, 0, 0, 0)
    assert int(c["n_blocks"][0]) == len(want) and int(c["pos_off"][0]) == 0 and int(c["first_block"][0]) == 0


def test_whole_stream_pass_goes_through_the_stream_tables():
    """(end - start) / 32768 + 1 blocks a piece, one more behind a flush; positions rounded up to a segment and one more"""
    c = CP.chunks_of([70000, 65536])
    nb, blk, sb, st = CP.pass_tables(c, stream=True, mode=6)
    assert [int(x) for x in c["n_blocks"]] == [3, 3] and [int(x) for x in c["first_block"]] == [0, 3]
    assert nb == 6 and blk == [0, 0, 0, 1, 1, 1] and sb == []
    assert st[1] == 2 and st[3] == 0   # a piece a stream, no flush points
    assert [int(x) for x in c["pos_off"]] == [0, 3 * CP.FL_SEG + CP.FL_SEG]
    c = CP.chunks_of([100])
    nb, blk, _, st = CP.pass_tables(c, stream=True, mode=6, flush=[40], finish=True)
    assert nb == 3 and blk == [0, 0, 0] and st[1] == 2 and st[3] == 1   # [0, 40) + marker, [40, 100)
    assert int(c["n_flush"][0]) == 1 and int(c["n_piece"][0]) == 2


@pytest.mark.parametrize("mode", [0, 1, 6])
def test_blk_chunk_first_block_and_the_pinned_total(mode):
    """blk_chunk has nb entries in chunk order, first_block is the running sum, and what the pinned path reserves for the
    whole batch is the sum over its passes"""
    rng = np.random.default_rng(5 + mode)
    lens = [int(x) for x in rng.choice([0, 1, B - 1, B, B + 1, 2 * B, 3 * B + 7], size=300)]
    if mode >= 4:
        lens = [min(x, B) for x in lens]
    per = [2 if mode >= 4 else x // B + 1 for x in lens]
    assert CP.batch_blocks(lens, mode) == sum(per)
    passes = CP.walk(lens, host=64, mode=mode, pinned=True, ramp=False)
    assert len(passes) > 2
    total = 0
    for c0, nc, stream in passes:
        assert not stream
        c = CP.chunks_of(lens[c0:c0 + nc])
        nb, blk, _, _ = CP.pass_tables(c, mode=mode)
        assert nb == len(blk) == sum(per[c0:c0 + nc])
        assert blk == [i for i in range(nc) for _ in range(per[c0 + i])]
        assert [int(x) for x in c["first_block"]] == [sum(per[c0:c0 + i]) for i in range(nc)]
        total += nb
    assert total == CP.batch_blocks(lens, mode)
    assert CP.batch_blocks([0, B - 1, B, 2 * B], 1) == 7 and CP.batch_blocks([0, B - 1, B, 2 * B], 0) == 7
    assert CP.batch_blocks([0, 5, B], 6) == 6


# ---------------------------------------------------------------- two compute streams

def test_two_stream_truth_table():
    """more than one pass (a pinned batch above the sub-batch size, or a plan of two passes), levels only, no flush points,
    FLATE_HIP_ONE_COMPUTE_STREAM unset, every input on the chunk path"""
    host = 4
    for planned, more, mode, flush, one, long_one in itertools.product([False, True], [False, True], [1, 6], [False, True],
                                                                       [False, True], [False, True]):
        n = host + 1 if more or planned else host   # (a planned call's chunk count does not matter: its passes do)
        lens = [100] * n
        if long_one:
            lens[n // 2] = 65536
        want = more and mode == 6 and not flush and not one and not long_one
        got = CP.two_eligible(lens, pinned_passes=not planned, planned_passes=(2 if more else 1) if planned else 0,
                              mode=mode, flush=flush, one_stream=one, host=host)
        assert got is want, (planned, more, mode, flush, one, long_one)
    short = [100] * 10
    assert CP.two_eligible(short, True, 0, 6, host=4) is True
    assert CP.two_eligible(short, True, 0, 9, host=4) is True and CP.two_eligible(short, True, 0, 4, host=4) is True
    assert CP.two_eligible(short, True, 0, 6, host=10) is False          # one sub-batch
    assert CP.two_eligible(short, True, 0, 6, host=4, max_pass=3) is True    # (the sub-batch is never above max_pass_chunks)
    assert CP.two_eligible(short, False, 0, 6, host=4) is False          # a device batch that is not planned
    assert CP.two_eligible(short, False, 3, 6) is True
    assert CP.two_eligible([65535] * 10, True, 0, 6, host=4) is True     # 65535 is still the chunk path
    assert CP.two_eligible([65535] * 9 + [65536], True, 0, 6, host=4) is False


def test_two_stream_slices_of_a_plan():
    on, sched, nc, nb = CP.two_from_plan([(1024, 2048), (300, 600), (1500, 3000)])
    assert on and sched == [(0, 1024, 0), (1024, 300, 1), (1324, 1500, 0)] and (nc, nb) == (1500, 3000)
    # the largest pass by chunks and the largest by blocks need not be one pass
    on, sched, nc, nb = CP.two_from_plan([(10, 50), (20, 40)])
    assert on and sched == [(0, 10, 0), (10, 20, 1)] and (nc, nb) == (20, 50)
    assert CP.two_from_plan([(1024, 2048)])[0] is False     # fewer than two passes: off
    assert CP.two_from_plan([])[0] is False


def test_two_stream_slices_of_a_schedule():
    on, sched, nc, nb = CP.two_from_schedule(2559)          # 1024 + the merged tail at its largest
    assert on and sched == [(0, 1024, 0), (1024, 1535, 1)] and (nc, nb) == (1535, 3070)
    on, sched, nc, nb = CP.two_from_schedule(3072)
    assert on and [s[1] for s in sched] == [256, 512, 1024, 1280] and [s[2] for s in sched] == [0, 1, 0, 1]
    assert (nc, nb) == (1280, 2560)
    # above the sub-batch size but one merged pass: a second slice would never be used
    for n in (1025, 1535):
        on, sched, nc, nb = CP.two_from_schedule(n)
        assert not on and sched == [(0, n, 0)]
    assert CP.two_from_schedule(1536)[0] is True
    assert CP.two_from_schedule(7, host=4)[:2] == (True, [(0, 4, 0), (4, 3, 1)])


# ---------------------------------------------------------------- the rectangle copy's rows

def slots(pitches, base=0):
    out = [base]
    for p in pitches:
        out.append(out[-1] + p)
    return out


def test_rect_rows():
    assert CP.rect_rows(slots([8224]), 1) == (0, 0, 0)                       # one slot: nothing to compare
    assert CP.rect_rows(slots([8224] * 63), 1) == (0, 8224, 4112)            # 63 rows: off
    assert CP.rect_rows(slots([8224] * 64), 1) == (64, 8224, 4112)
    assert CP.rect_rows(slots([8224] * 64, base=12345), 1) == (64, 8224, 4112)
    assert CP.rect_rows(slots([8224] * 64 + [8000]), 1) == (64, 8224, 4112)  # the uniform run, the rest by the copy kernel
    assert CP.rect_rows(slots([8224] * 64 + [8000] + [8224] * 100), 1) == (64, 8224, 4112)
    assert CP.rect_rows(slots([8224] + [8000] * 200), 1) == (0, 8224, 4112)  # another pitch at row 1: a run of one
    assert CP.rect_rows(slots([8190] * 64), 1) == (0, 8190, 4080)            # half = 4095 & ~15 = 4080 < 4096
    assert CP.rect_rows(slots([8192] * 64), 1) == (64, 8192, 4096)           # exactly 4096
    assert CP.rect_rows(slots([8222] * 64), 1) == (64, 8222, 4096)           # 4111 & ~15
    for knob in (-1, 0):                                                    # off unless FLATE_HIP_RECT=1
        assert CP.rect_rows(slots([8224] * 64), knob) == (0, 8224, 4112)
        assert CP.rect_rows(slots([8224] * 500), knob) == (0, 8224, 4112)
