"""The planted flush inputs of tests/_planted_flush.py do what their names say (CPU only): fed the case's writes and flushes, the
oracle's streaming compressor shows every token the construction predicts -- the match cut at the flush point, the literals where
a piece is shorter than 4 bytes or the source is one of the three positions in front of a flush point, M(4, ..) at a flush point
inside a run, the literals of a candidate that a slide dropped --, every finished stream inflates to its input under zlib and every
unfinished one ends in the sync marker.  On uniform bytes the block log shows the blocks that can no longer be stored (has_input
== 0) exactly for the flush points the reference's window bookkeeping gives them to.  The presence of every (kind, boundary)
class and of every flush pattern, the phases the events start at and the size of the list are asserted too: a later thinning cannot
empty one.  A case that stops sitting on its edge fails here instead of passing silently on the GPU
(tests/test_gpu_flush_geometry.py)."""
import functools
import zlib

import pytest

import _oracle as O
import _planted as P
import _planted_flush as PF
from _adversarial import LV

LEVELS = (4, 5, 6, 7, 8, 9)

# Cases whose event the oracle does not show as planted, or whose oracle stream does not inflate (quirk Q1): {level: names}.  At most
# 2 % of a (kind, level) class; the GPU test runs them for parity all the same.
FLUSH_DROPPED = {}


def oracle_stream(case, level, container=O.RAW, log=True):
    """(bytes, token log, block log) of the oracle's Deflate object fed the case's calls"""
    d = O.Deflate(container, level, log_tokens=log)
    prev = 0
    for f in case.flushes:
        d.write(case.data[prev:f])
        d.flush()
        prev = f
    if case.finish:
        d.write(case.data[prev:])
        d.finish()
    res = d.output(), (d.tokens() if log else None), (d.blocks() if log else None)
    d.close()
    return res


@functools.lru_cache(None)
def _verdicts(level):
    """per case: (name, kind, the first `want` the token log misses | None, why the stream is not the input's | None), and the
    count of null-input blocks per noise flush point"""
    rows, nulls = [], {}
    for c in PF.flush_cases(level):
        out, tok, blocks = oracle_stream(c, level)
        why = None
        if c.finish:
            try:
                if zlib.decompress(out, -15) != c.data:
                    why = "inflates to something else"
            except zlib.error as e:
                why = str(e)
        else:
            d = zlib.decompressobj(-15)
            if not out.endswith(b"\x00\x00\xff\xff"):
                why = "no sync marker at the end"
            elif d.decompress(out) != c.data or d.eof:
                why = "the prefix does not inflate to the data written"
        rows.append((c.name, c.kind, P.missed(c, tok), why))
        if c.kind == "noise":
            nulls[c.F] = sum(1 for b in blocks if b[2] == 0 and b[0] == 32768)
    return rows, nulls


@pytest.mark.parametrize("level", LEVELS)
def test_flush_cases_meet_their_intent(level):
    rows, _ = _verdicts(level)
    dropped = set(FLUSH_DROPPED.get(level, ()))
    assert dropped <= {r[0] for r in rows}
    bad, per_class = [], {}
    for name, kind, miss, why in rows:
        k = per_class.setdefault(kind, [0, 0])
        k[0] += 1
        if name in dropped:
            k[1] += 1
        elif miss is not None or why is not None:
            bad.append((name, miss, why))
    assert not bad, (level, len(bad), len(rows), bad[:5])
    for kind, (n, d) in per_class.items():
        assert d <= 0.02 * n, (level, kind, n, d)


@pytest.mark.parametrize("level", LEVELS)
def test_every_class_and_pattern_is_present(level):
    lazy = LV[level][1]
    cases = PF.flush_cases(level)
    assert len(cases) <= PF.MAX_FLUSH
    assert len({c.name for c in cases}) == len(cases)
    have = {(c.kind, c.bound) for c in cases}
    want = {("straddle", b) for b in PF.BOUNDS + ("N",)}
    want |= {(kind, b) for kind in ("source", "run") for b in PF.BOUNDS}  # (B = N: these would end behind the stream)
    want |= {("far", b) for b in PF.BOUNDS if b != 14400}                 # (a - 32768 < 0)
    want |= {("noise", b) for b in (32768, 65274, 65536, 98042, 98304)}
    if lazy >= 5:
        want |= {("ladder", b) for b in PF.BOUNDS}
    assert have == want, (level, have ^ want)
    # every parameter of every kind
    labels = {c.name.split("/")[1].split("@")[0] for c in cases}
    for L in PF.STRADDLE_L:
        for D in PF.STRADDLE_D:
            assert any(s.startswith("straddle_L%d_D%d_" % (L, D)) for s in labels), (L, D)
        for k in PF._k_values(L):
            assert any(s.startswith("straddle_L%d_" % L) and s.endswith("_k%d" % k) for s in labels), (L, k)
    for j in PF.SOURCE_J:
        for where in ("near", "D32768", "D32769"):
            assert "source_j%+d_%s" % (j, where) in labels, (j, where)
    for R in PF.RUN_R:
        for start in ("half", "F-2"):
            assert "run_%d_%s" % (R, start) in labels
    for D in P.FAR_D:
        for off in (0, 1):
            assert "far_D%d_a%+d" % (D, off) in labels
    for s in PF.LADDER_STEPS:
        ds = {int(x.rsplit("_d", 1)[1]) for x in labels if x.startswith("ladder_%d_" % s)}
        if s + 4 > lazy:
            assert not ds  # (its last step is no longer evaluated lazily at this level)
        else:
            assert min(ds) == -(s + 2) and max(ds) == 1 and 0 in ds and -1 in ds, (s, sorted(ds))
    assert {c.F for c in cases if c.kind == "noise"} == set(PF.NOISE_F)
    # every flush pattern, at every boundary (B = N: those without a flush point behind the stream's end)
    for b in PF.BOUNDS:
        assert {PF.pattern_of(c) for c in cases if c.bound == b} == set(PF.PATTERNS), b
    assert {PF.pattern_of(c) for c in cases if c.bound == "N"} >= {"F", "FF", "F-4,F", "unfinished"}
    for kind in ("straddle", "source"):
        for b in PF.BOUNDS + (("N",) if kind == "straddle" else ()):
            mine = [c for c in cases if c.kind == kind and c.bound == b]
            plain = sum(1 for c in mine if PF.pattern_of(c) == "F")
            assert len(mine) - plain == (plain + 2) // 3, (kind, b, plain, len(mine))  # a third, rounded up
    for c in cases:
        assert c.flushes == PF._flushes_of(PF.pattern_of(c), c.F) and c.finish == (PF.pattern_of(c) != "unfinished")
        assert len(c.data) == (c.F if not c.finish else PF._len_of(c.bound) if c.bound != "N" else PF.STREAM_LEN), c.name
        assert list(c.flushes) == sorted(c.flushes) and 0 <= c.flushes[0] and c.flushes[-1] <= len(c.data), c.name
    # source: delta = -4 .. +4 by ones at every boundary
    for b in PF.BOUNDS:
        assert {c.F - b for c in cases if c.kind == "source" and c.bound == b} == set(range(-4, 5)), b


@pytest.mark.parametrize("level", LEVELS)
def test_flush_points_and_events_meet_every_phase(level):
    """F takes every place from 4 below to 4 above a window start (the `wabs` / `w0` comparisons of the kernels), and the events
    that k_lz_parse<true> enters a segment with -- straddle, ladder -- start at every offset of a 24-byte segment"""
    cases = PF.flush_cases(level)
    for w0 in (32768, 65536, 98304):
        assert {c.F - w0 for c in cases if abs(c.F - w0) <= 4} == set(range(-4, 5)), w0
    assert {c.a % 24 for c in cases if c.kind in ("straddle", "ladder")} == set(range(24))
    # the zone edges of the first two slides, and the stream's end
    fs = {c.F for c in cases}
    for full in (65536, 98304):
        assert {full - 262 + d for d in range(-4, 5)} <= fs and {full + d for d in range(-4, 5)} <= fs
    assert {PF.STREAM_LEN - e for e in range(5)} <= {c.F for c in cases if c.bound == "N"}


def test_some_cases_have_their_candidate_dropped_by_a_slide():
    """the rule of the module docstring is exercised: cases whose whole event is literals although its distance is within
    32768 (the slide dropped the source), and cases whose match starts only behind the window's fill"""
    cases = [c for c in PF.flush_cases(9) if c.kind in ("straddle", "source") and "D32768" in c.name and c.want]
    zone = [c for c in cases if any(z <= c.a <= z + 262 for z in PF.zones(len(c.data), c.flushes))]
    assert len(zone) >= 6, len(zone)
    assert any(all(w[1] == ("L",) for w in c.want) for c in zone)
    assert any(c.want[0][1] == ("L",) and any(w[1][0] == "M" for w in c.want) for c in zone)


@pytest.mark.parametrize("level", LEVELS)
def test_noise_blocks_lose_their_input_where_the_flush_point_says(level):
    """140000 uniform bytes: a full block of 32768 tokens is handed to the block writer without its input (the Zig `null`: it
    cannot be stored) exactly when the flush point lies one byte before the first window start or inside the first slide's zone"""
    _, nulls = _verdicts(level)
    for F in PF.NOISE_F:
        if F == 32767 or 65274 <= F <= 65535:
            assert nulls[F] >= 1, (level, F, nulls)
        elif F in (32768, 32769, 65273, 65536, 65537):
            assert nulls[F] == 0, (level, F, nulls)


def test_the_rules_on_hand_made_examples():
    """the probes the rules were read from, as the rules give them (stream of 140000 bytes, one flush point)"""
    n = 140000
    # a match over a flush point: both pieces, or literals where a piece is shorter than 4
    assert PF._sim_copy(14400 - 10, 33, 1000, n, (14400,)) == ((14390, ("M", 1000, 10)), (14400, ("M", 1000, 23)))
    assert PF._sim_copy(14400 - 3, 33, 1000, n, (14400,)) == tuple((14397 + i, ("L",)) for i in range(3)) + ((14400, ("M", 1000, 30)),)
    assert PF._sim_copy(14400 - 30, 33, 1000, n, (14400,)) == ((14370, ("M", 1000, 30)),) + tuple((14400 + i, ("L",)) for i in range(3))
    # the source one byte in front of the flush point: one literal, then the match one byte shorter
    assert PF._sim_copy(17400, 20, 3001, n, (14400,)) == ((17400, ("L",)), (17401, ("M", 3001, 19)))
    assert PF._sim_copy(17400, 20, 3004, n, (14400,)) == ((17400, ("M", 3004, 20)),)
    # a run from F - 300: distance 4 at F
    run = dict(PF._sim_run(14100, 700, n, (14400,)))
    assert run[14100] == ("L",) and run[14101] == ("M", 1, 258) and run[14359] == ("M", 1, 41) and run[14400] == ("M", 4, 258)
    assert run[14658] == ("M", 1, 142)
    # F = 98404: a 258-byte match at distance 32768 from F - 257 is literals up to 98304, from F - 100 a match behind the fill
    far = PF._sim_copy(98404 - 257, 258, 32768, n, (98404,))
    assert far[:158] == tuple((98147 + i, ("L",)) for i in range(158)) and far[158:] == ((98305, ("M", 32768, 99)), (98404, ("L",)))
    assert PF._sim_copy(98404 - 100, 258, 32768, n, (98404,)) == ((98304, ("L",)), (98305, ("M", 32768, 99)), (98404, ("M", 32768, 158)))
    # several flush points
    assert PF._sim_copy(14400, 33, 1000, n, (14400, 14401, 14402, 14403)) == tuple((14400 + i, ("L",)) for i in range(3)) + ((14403, ("M", 1000, 30)),)
    assert PF._sim_copy(14390, 33, 1000, n, (14396, 14400)) == ((14390, ("M", 1000, 6)), (14396, ("M", 1000, 4)), (14400, ("M", 1000, 23)))
    # a flush point inside the 262 bytes before the window fills moves the zone
    assert PF.zones(n, ()) == [65274, 98042, 130810] and PF.zones(n, (65400, 98303)) == [65400, 98303, 130810]
    assert PF.zones(n, (65274, 65536)) == [65274, 98042, 130810] and PF.zones(65535, (65400,)) == []


@pytest.mark.parametrize("level", [4, 6, 9])
def test_object_cases_meet_their_intent(level):
    """the streams of the Compressor-object test: three flush points, the event behind the third"""
    cases = PF.object_cases()
    assert {c.F for c in cases} == set(PF.OBJECT_F) and all(c.flushes == PF.OBJECT_BEFORE + (c.F,) for c in cases)
    assert {(c.kind, c.F) for c in cases} == {(k, F) for k in ("far", "straddle", "ladder") for F in PF.OBJECT_F}
    # (parity only: the far candidate whose source is the last position a slide dropped -- what a + 1 does depends on `lazy`)
    assert {(c.a, c.name.split("/")[2][:10]) for c in cases if not c.want} == {(229376, "far_D32768"), (262144, "far_D32768")}
    bad = []
    for c in cases:
        assert len(c.data) == PF.OBJECT_LEN, c.name
        out, tok, _ = oracle_stream(c, level)
        m = P.missed(c, tok) if c.min_lazy <= LV[level][1] else None
        if m is not None or zlib.decompress(out, -15) != c.data:
            bad.append((c.name, m))
    assert not bad, (level, bad[:5])
