"""The host decisions of a whole-stream pass (flate_amd/csrc/stream_plan.h), on the CPU: every expected value below is
worked out by hand from the rules the header states -- a window is 64 KiB of its stream from position 32768 j, a
stream of N >= 65536 bytes slides (N - 65536) // 32768 + 1 times and has one window more than slides, a workgroup walks
a group of G windows -- never by asking the header twice."""
import pytest

import _stream_plan as P

NONE = 0xffffffff      # fl_swin.prev of a stream's first group; G of a pass whose groups are whole streams
MIB = 1 << 20


def stream_of(nwin):
    """a stream length with `nwin` windows"""
    return 1000 if nwin == 1 else 65536 + (nwin - 2) * 32768


# ---------------------------------------------------------------------------------------------------- the window table
# N -> per window (in_len, bytes behind the window that the lazy calls look at)
WINDOWS = {
    1: [(1, 0)],
    65535: [(65535, 0)],
    65536: [(65536, 0), (32768, 0)],
    65537: [(65536, 1), (32769, 0)],
    98304: [(65536, 264), (65536, 0), (32768, 0)],
    98305: [(65536, 264), (65536, 1), (32769, 0)],
    131072 + 263: [(65536, 264), (65536, 264), (65536, 263), (33031, 0)],
    131072 + 264: [(65536, 264), (65536, 264), (65536, 264), (33032, 0)],
    131072 + 265: [(65536, 264), (65536, 264), (65536, 264), (33033, 0)],   # capped at 264
}


@pytest.mark.parametrize("n", sorted(WINDOWS))
def test_window_table_of_one_stream(n):
    wins, groups, meta = P.windows([(4096, n, 0, 0)], n_cu=1)
    want = WINDOWS[n]
    assert P.n_slides(n) + 1 == len(want) == meta["nw"] == len(wins)
    for j, (w, (in_len, look)) in enumerate(zip(wins, want)):
        # (in_off, in_len, pad_: bit 0 "a window", bits 8.. the lookahead, piece0: the window's position in its stream)
        assert w == (4096 + 32768 * j, in_len, 1 | look << 8, 32768 * j, 0, 0), (j, w)
        assert w[0] - 4096 + in_len + look <= n
    assert meta["bytes"] == n
    # one CU and one stream: the stream is one group
    assert groups == [(0, 0, len(want), 0, NONE)] and not meta["grouped"] and meta["G"] == NONE


def test_window_table_copies_the_flush_fields_and_numbers_windows_through_the_pass():
    wins, groups, meta = P.windows([(1000, 98305, 7, 3), (200000, 1, 10, 0), (300000, 65537, 10, 2)], n_cu=2)
    assert [w[0] for w in wins] == [1000, 1000 + 32768, 1000 + 65536, 200000, 300000, 300000 + 32768]
    assert [w[3] for w in wins] == [0, 32768, 65536, 0, 0, 32768]
    assert [w[4:] for w in wins] == [(7, 3)] * 3 + [(10, 0)] + [(10, 2)] * 2
    assert [w[2] >> 8 for w in wins] == [264, 1, 0, 0, 1, 0] and all(w[2] & 0xff == 1 for w in wins)
    assert meta["bytes"] == 98305 + 1 + 65537 and meta["nw"] == 6
    assert groups == [(0, 0, 3, 0, NONE), (1, 3, 1, 0, NONE), (2, 4, 2, 0, NONE)]   # 3 streams >= 2 slots


# ---------------------------------------------------------------------------------------------------------- the groups
def test_as_many_streams_as_slots_one_group_per_stream():
    wins, groups, meta = P.windows([98304] * 4, n_cu=4)
    assert meta["slots"] == 4 and meta["G"] == NONE and not meta["grouped"] and meta["max_win"] == 3
    assert groups == [(i, 3 * i, 3, 0, NONE) for i in range(4)]


@pytest.mark.parametrize("total_win,G", [(7, 1), (8, 1), (9, 2), (25, 4)])   # slots - 1, slots, slots + 1, 3 * slots + 1
def test_one_stream_is_cut_into_as_many_groups_as_the_chip_holds(total_win, G):
    wins, groups, meta = P.windows([stream_of(total_win)], n_cu=8)
    assert meta["nw"] == total_win and meta["slots"] == 8 and meta["G"] == G   # max(1, ceil(total_win / slots))
    ng = -(-total_win // G)
    assert len(groups) == ng <= 8 and meta["grouped"] and meta["max_win"] == G
    for k, g in enumerate(groups):
        last = total_win - G * k
        assert g == (0, G * k, min(G, last), G * k, NONE if k == 0 else k - 1)
    assert groups[-1][2] == (total_win % G or G)    # the last group of a stream may be short: 9 = 4 x 2 + 1, 25 = 6 x 4 + 1


def test_prev_chains_restart_with_every_stream():
    wins, groups, meta = P.windows([stream_of(5), stream_of(4)], n_cu=8)   # 9 windows on 8 slots: G = 2
    assert meta["G"] == 2 and meta["grouped"] and meta["max_win"] == 2
    assert groups == [(0, 0, 2, 0, NONE), (0, 2, 2, 2, 0), (0, 4, 1, 4, 1), (1, 5, 2, 0, NONE), (1, 7, 2, 2, 3)]


def test_the_group_knob_overrides_g_whatever_the_number_of_streams():
    wins, groups, meta = P.windows([stream_of(5)] * 4, n_cu=4, group_knob=3)     # 4 streams on 4 slots: whole streams, but for the knob
    assert meta["G"] == 3 and meta["grouped"]
    assert groups == [g for i in range(4) for g in ((i, 5 * i, 3, 0, NONE), (i, 5 * i + 3, 2, 3, 2 * i))]
    wins, groups, meta = P.windows([stream_of(9)], n_cu=8, group_knob=1)         # (by the rule: 2)
    assert meta["G"] == 1 and len(groups) == 9 and all(g[2] == 1 for g in groups)
    wins, groups, meta = P.windows([stream_of(9)], n_cu=8, group_knob=100)
    assert groups == [(0, 0, 9, 0, NONE)] and not meta["grouped"]


def test_slots_double_from_the_chain_budget_of_the_deep_walk():
    L = P.lib()
    assert L.shim_bulk_min_chain() == 1024       # level 8's chain budget (level_args): levels 8 and 9 walk deep
    assert not L.shim_stream_deep_walk(1023) and L.shim_stream_deep_walk(1024) and L.shim_stream_deep_walk(4096)
    assert not L.shim_stream_deep_walk(256)      # level 7
    _, g6, m6 = P.windows([stream_of(17)], n_cu=8)
    _, g9, m9 = P.windows([stream_of(17)], n_cu=8, deep_walk=True)
    assert (m6["slots"], m6["G"], len(g6)) == (8, 3, 6)       # ceil(17 / 8) = 3: 5 x 3 + 2
    assert (m9["slots"], m9["G"], len(g9)) == (16, 2, 9)      # ceil(17 / 16) = 2: 8 x 2 + 1


@pytest.mark.parametrize("n_cu,deep,G,ng", [(1, False, NONE, 1),       # 1 stream is not fewer than 1 slot: the whole stream
                                             (1, True, 500, 2),         # 2 slots
                                             (256, False, 4, 250), (256, True, 2, 500),
                                             (304, False, 4, 250),      # ceil(1000 / 304) = 4
                                             (304, True, 2, 500)])      # ceil(1000 / 608) = 2
def test_groups_by_the_number_of_compute_units(n_cu, deep, G, ng):
    _, groups, meta = P.windows([stream_of(1000)], n_cu=n_cu, deep_walk=deep)
    assert meta["slots"] == n_cu * (2 if deep else 1) and meta["G"] == G and len(groups) == ng
    assert sum(g[2] for g in groups) == 1000 and meta["grouped"] == (ng > 1)


def test_608_windows_fill_the_608_slots_of_304_units_one_more_doubles_g():
    assert P.windows([stream_of(608)], n_cu=304, deep_walk=True)[2]["G"] == 1
    assert P.windows([stream_of(609)], n_cu=304, deep_walk=True)[2]["G"] == 2


# -------------------------------------------------------------------------------------------------------- the estimate
def test_eligibility_for_the_windows():
    ok = P.lib().shim_stream_windows_allowed
    # flush points with a deep chain: refused whatever the knob
    assert [ok(1, 1, k, 5) for k in (-1, 0, 1)] == [0, 0, 0]
    assert ok(1, 0, -1, 5) and ok(1, 0, 1, 5)          # flush points at levels 4-7: allowed
    assert ok(0, 1, -1, 5) and ok(0, 1, 1, 5)          # a deep chain without flush points: allowed
    assert not ok(0, 0, 0, 5) and not ok(0, 1, 0, 5)   # the knob at 0: never
    assert not ok(0, 0, -1, 0) and not ok(0, 0, 1, 0)  # no segment (an empty stream): nothing to walk


# 256 compute units.  est_new = rounds x max_win x win_ms (+ rounds x win_ms + 0.1 when grouped), win_ms 0.28 (deep: 1.5);
# est_old = MiB x 0.061 + 0.8 (deep: MiB x 0.11 + 1.3)
ESTIMATES = [
    # one 1 MiB stream, level 6: 32 windows as 32 groups of one in one round: 0.28 + 0.28 + 0.1 against 0.061 + 0.8 -- windows
    ("1 MiB, level 6", [MIB], False, True, 0.66, 0.861),
    # one 16 MiB stream, level 9: 512 windows on 512 slots, G = 1: 1.5 + 1.5 + 0.1 against 16 x 0.11 + 1.3 -- tiles, by 0.04 ms
    ("16 MiB, level 9", [16 * MIB], True, False, 3.1, 3.06),
    # one 100 MiB stream, level 9: 3200 windows, G = ceil(3200 / 512) = 7, 458 groups in one round:
    # 7 x 1.5 + 1.5 + 0.1 against 100 x 0.11 + 1.3 -- windows, by 0.2 ms
    ("100 MiB, level 9", [100 * MIB], True, True, 12.1, 12.3),
    # 256 streams of 1 MiB, level 6: a workgroup per stream, 32 windows each, no fix: 32 x 0.28 against 256 x 0.061 + 0.8 -- windows
    ("256 x 1 MiB, level 6", [MIB] * 256, False, True, 8.96, 16.416),
    # ... level 9: 512 slots, G = 8192 / 512 = 16, two groups a stream: 16 x 1.5 + 1.5 + 0.1 against 256 x 0.11 + 1.3 -- windows
    ("256 x 1 MiB, level 9", [MIB] * 256, True, True, 25.6, 29.46),
    # 2560 streams of 1000 bytes, level 6: ten rounds of one window, 2.8, against 2560000 / 2^20 x 0.061 + 0.8 = 0.949 -- tiles
    ("2560 x 1000 bytes, level 6", [1000] * 2560, False, False, 2.8, 2560000 / MIB * 0.061 + 0.8),
]


@pytest.mark.parametrize("name,streams,deep,windows,est_new,est_old", ESTIMATES, ids=[e[0] for e in ESTIMATES])
def test_estimate_with_the_knob_unset(name, streams, deep, windows, est_new, est_old):
    got = P.estimate(streams, n_cu=256, deep_walk=deep)
    assert got[0] == windows == (est_new < est_old)
    assert got[1] == pytest.approx(est_new, rel=1e-12) and got[2] == pytest.approx(est_old, rel=1e-12)
    # the knob at 1: the windows whatever the estimate says (at 0 the pass is not eligible: test_eligibility_for_the_windows)
    assert P.estimate(streams, n_cu=256, deep_walk=deep, windows_knob=1)[0]


def test_tile_limit_cuts_the_windows_whatever_the_knob():
    for knob in (-1, 1):
        assert P.estimate([MIB], n_cu=256, windows_knob=knob, tile_limit=32)[0]          # 32 windows
        assert not P.estimate([MIB], n_cu=256, windows_knob=knob, tile_limit=31)[0]
        assert P.estimate([MIB + 32768], n_cu=256, windows_knob=knob, tile_limit=33)[0]  # 33 windows
        assert not P.estimate([MIB + 32768], n_cu=256, windows_knob=knob, tile_limit=32)[0]


def test_round_cap_of_small_passes_of_few_streams():
    cap = lambda streams, **kw: P.estimate(streams, n_cu=256, **kw)[3]
    assert cap([64 * MIB - 1]) == 24 and cap([64 * MIB]) == 0
    assert cap([32 * MIB - 1, 32 * MIB]) == 24 and cap([32 * MIB, 32 * MIB]) == 0   # the pass's bytes, not a stream's
    assert cap([1000] * 255) == 24 and cap([1000] * 256) == 0                       # nc == slots - 1 / slots
    assert cap([1000] * 511, deep_walk=True) == 24 and cap([1000] * 512, deep_walk=True) == 0
    assert cap([64 * MIB - 1], windows_knob=1) == 24                                # (not the estimate's business)


# ----------------------------------------------------------------------------------------------------- the fix verdict
def test_fix_verdict():
    assert P.lib().shim_stream_fix_max() == 3
    v = P.fix_verdict
    for ng in (1, 8, 80):
        assert v(0, 0, ng) == v(1, 0, ng) == v(2, 0, ng) == P.SETTLED
        # bit 31: a window's stitch did not settle -- given up at once, behind the first launch too
        assert v(P.FIX_FIRST, 0x80000000, ng) == v(0, 0x80000000, ng) == v(0, 0x80000001, ng) == P.GIVE_UP
        # the first launch looks at nothing else: the fix launches follow
        assert v(P.FIX_FIRST, 0, ng) == v(P.FIX_FIRST, 1, ng) == v(P.FIX_FIRST, 0x7fffffff, ng) == P.AGAIN
    # more than ng / 8 + 1 groups moved: periodic data
    assert v(0, 11, 80) == P.AGAIN and v(0, 12, 80) == P.GIVE_UP     # 80 / 8 + 1 = 11 against 80 / 8 + 2
    assert v(0, 1, 1) == P.AGAIN and v(0, 2, 1) == P.GIVE_UP         # 1 / 8 + 1 = 1
    assert v(0, 2, 8) == P.AGAIN and v(0, 3, 8) == P.GIVE_UP         # 8 / 8 + 1 = 2
    # FL_STREAM_FIX_MAX launches and still moving: the fix launch number FL_STREAM_FIX_MAX - 1 is the last
    assert v(3 - 2, 1, 80) == P.AGAIN and v(3 - 1, 1, 80) == P.GIVE_UP
    assert v(3 - 1, 0, 80) == P.SETTLED


# ---------------------------------------------------------------------------------------------------------- the stitch
def test_stitch_direct_up_to_four_groups_of_segments():
    assert P.stitch_plan([3, 256, 0]) == (256, True, [], [])
    max_seg, direct, groups, group0 = P.stitch_plan([3, 257, 0])
    assert (max_seg, direct) == (257, False)
    assert groups == [(0, 0)] + [(1, g) for g in range(5)] and group0 == [0, 1, 6]


def test_stitch_group_tables_of_mixed_pieces():
    # pieces of 0 (flush called twice: no segment, no group), 1, 64, 65 and 257 segments: 0 + 1 + 1 + 2 + 5 groups of up to 64
    max_seg, direct, groups, group0 = P.stitch_plan([0, 1, 64, 65, 257])
    assert (max_seg, direct) == (257, False)
    assert group0 == [0, 0, 1, 2, 4]
    assert groups == [(1, 0), (2, 0), (3, 0), (3, 1), (4, 0), (4, 1), (4, 2), (4, 3), (4, 4)]
    # an empty piece in the middle and at the end
    assert P.stitch_plan([300, 0, 0, 2, 0])[2:] == ([(0, g) for g in range(5)] + [(3, 0)], [0, 5, 5, 5, 6])


# ------------------------------------------------------------------------------------------------------- the workspace
def test_wexit_layout():
    # 2 words a window | a word a group | a word a group | the dirty word (and three to spare)
    assert P.wexit_offsets(3, 2) == {"wexit": 0, "gexit": 6, "gentry": 8, "dirty": 10, "words": 14}
    assert P.wexit_offsets(1, 1) == {"wexit": 0, "gexit": 2, "gentry": 3, "dirty": 4, "words": 8}
    big = P.wexit_offsets(0xffffffff, 0xffffffff)     # no 32-bit wrap
    assert big["dirty"] == 4 * 0xffffffff and big["words"] == big["dirty"] + 4


# One stream of 100000 bytes without flush points: positions rounded up to 4 x 32768 and one segment more (163840), tiles at
# 0, 32768 and 65536, segments at 0 .. 98304, one piece, two slides (a zone each), 100000 // 32768 + 1 = 4 block slots.
# Records: fl_tile 16 bytes, fl_seg 8, fl_piece 32, fl_chunk 80, fl_swin 32, fl_sgroup 8.
PASS = dict(npos=163840, ntiles=3, nfpts=0, nzones=2, nseg=4, npc=1, nb=4)


def test_workspace_of_every_pass():
    got, tpl = P.workspace(P.COMMON, **PASS)
    assert tpl == 3
    assert got == [("tiles", 48), ("segs", 8 * 5), ("pieces", 32), ("fpts", 4), ("zones", 12), ("nsorted", 12), ("cflag", 12),
                   ("S", 3 * 65536 * 2), ("desc", 655360), ("tokens", 655360), ("marks", 20480), ("entry", 20), ("segtok", 20),
                   ("tokbase", 20), ("bound", 32), ("ntok", 4)]
    # the tiles run in launches of at most the tile limit: the sort scratch is one launch's
    got, tpl = P.workspace(P.COMMON, tile_limit=2, **PASS)
    assert tpl == 2 and dict(got)["nsorted"] == 8 and dict(got)["cflag"] == 8 and dict(got)["S"] == 2 * 65536 * 2
    assert dict(got)["tiles"] == 48


def test_workspace_of_the_windows():
    # three windows in three groups: 2 x 3 + 3 + 3 + 4 = 16 words of exits
    assert P.workspace(P.WINDOWS, a=3, b=3, **PASS)[0] == [("wchunks", 240), ("swins", 96), ("S", 3 * 131072), ("cflag", 12),
                                                           ("wexit", 64)]
    # levels 8-9: four link arrays a window, asked for on their own (a device may refuse them)
    assert P.workspace(P.WINDOWS, a=3, b=3, deep_walk=True, **PASS)[0] == [("wchunks", 240), ("swins", 96), ("cflag", 12), ("wexit", 64)]
    assert P.lib().shim_stream_links_bytes(3) == 3 * 4 * 131072
    assert P.lib().shim_stream_links_bytes(32768) == 16 << 30      # a 1 GiB stream: 16 GiB


def test_workspace_of_the_tiles_and_the_grouped_stitch():
    assert P.workspace(P.TILES, **PASS)[0] == [("NC", 3 * 65536 * 4), ("rec", 163840 * 8 + 64), ("jmp", 327680),
                                               ("exitmap", 5 * 512 * 2)]
    assert P.lib().shim_stream_rec_bytes(163840) == 1310720
    assert P.workspace(P.TILES, tile_limit=1, **PASS)[0][0] == ("NC", 65536 * 4)
    # nine groups over five pieces
    assert P.workspace(P.STITCH, a=9, b=5)[0] == [("sgroups", 80), ("sgroup0", 20), ("gmap", 10 * 512 * 2), ("gentry", 40)]
