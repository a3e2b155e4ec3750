"""The planted inputs of tests/_planted.py do what their names say (CPU only): in the oracle's token list the planted match
starts exactly at `a` with its distance and length, the candidate one past the distance limit is not taken, a ladder of
improving matches gives literals and then the 258-byte match, a run gives a literal and a match at distance 1.  A case that
stops sitting on its edge fails here instead of passing silently on the GPU (tests/test_gpu_tokenizer_geometry.py).  The sizes
of the lists and the presence of every (event kind, boundary) class are asserted too: a later thinning cannot empty one."""
import pytest

import _oracle as O
import _planted as P
from _adversarial import LV

LEVELS = (4, 5, 6, 7, 8, 9)

# Stream cases whose event the oracle does not show as planted (at most 2 % of an (event, level) class; the GPU test runs them for
# parity all the same): {level: names}.
STREAM_DROPPED = {}


def _classes(cases):
    return {(c.kind, c.bound) for c in cases}


@pytest.mark.parametrize("level", LEVELS)
def test_junk_chunks_meet_their_intent(level):
    cases = P.chunk_cases(level, "junk")
    assert len(cases) <= P.MAX_JUNK
    bad = []
    for c in cases:
        assert c.want, c.name
        m = P.missed(c, O.tokenize(c.data, level))
        if m is not None:
            bad.append((c.name, c.a) + m)
    assert not bad, (level, len(bad), len(cases), bad[:5])


@pytest.mark.parametrize("level", LEVELS)
def test_stream_cases_meet_their_intent(level):
    cases = P.stream_cases(level)
    assert len(cases) <= P.MAX_STREAMS
    dropped = set(STREAM_DROPPED.get(level, ()))
    assert dropped <= {c.name for c in cases}
    bad, per_class = [], {}
    for c in cases:
        assert len(c.data) == P.STREAM_LEN and c.want, c.name
        k = per_class.setdefault(c.kind, [0, 0])
        k[0] += 1
        if c.name in dropped:
            k[1] += 1
            continue
        m = P.missed(c, O.tokenize(c.data, level))
        if m is not None:
            bad.append((c.name, c.a) + m)
    assert not bad, (level, len(bad), len(cases), bad[:5])
    for kind, (n, d) in per_class.items():
        assert d <= 0.02 * n, (level, kind, n, d)


@pytest.mark.parametrize("level", LEVELS)
def test_every_event_class_is_present(level):
    lazy = LV[level][1]
    for bg, cap in (("junk", P.MAX_JUNK), ("text", P.MAX_TEXT)):
        cases = P.chunk_cases(level, bg)
        assert len(cases) <= cap
        assert len({c.name for c in cases}) == len(cases)
        have = _classes(cases)
        for kind in ("match", "ladder", "far", "run"):
            if kind == "ladder" and lazy < min(P.LADDER_STEPS) + 4:
                assert not any(c.kind == "ladder" for c in cases)  # level 4: the lazy evaluation stops at 4 bytes
                continue
            for bound in P.BOUNDS + ("N",):
                if kind == "far" and bound == 14400:
                    continue  # (a - 32768 < 0)
                assert (kind, bound) in have, (level, bg, kind, bound)
        # every parameter of every kind, and every chunk length
        labels = {c.name.split("/")[1].split("@")[0] for c in cases}
        want = {"match_L%d_D%d" % (L, D) for L in P.MATCH_L for D in P.MATCH_D} | {"far_D%d" % D for D in P.FAR_D}
        want |= {"run_%d" % R for R in P.RUN_R} | {"ladder_%d" % s for s in P.LADDER_STEPS if s + 4 <= lazy}
        assert labels == want, (level, bg, labels ^ want)
        sizes = {len(c.data) for c in cases}
        assert sizes == ({P.N_FULL} | set(P.N_EDGE) if bg == "junk" else {P.N_FULL}), (level, bg, sizes)
        if bg == "junk":
            for n in P.N_EDGE:
                for kind in ("match", "far", "run") + (("ladder",) if lazy >= 5 else ()):
                    for bound in (49152, "N"):
                        # (around the seam itself B = 49152 and B = N are the same place: either has the event)
                        assert any(c.kind == kind and len(c.data) == n and (c.bound == bound or n <= 49153) for c in cases), (level, kind, n, bound)
    streams = P.stream_cases(level)
    assert len(streams) <= P.MAX_STREAMS
    have = _classes(streams)
    for kind in ("match", "far") + (("ladder",) if lazy >= 5 else ()):
        for bound in P.STREAM_BOUNDS:
            assert (kind, bound) in have, (level, kind, bound)


def test_periodic_and_tiny_lists():
    per = P.periodic_cases()
    assert {(c.kind, c.bound) for c in per} == {("periodic", b) for b in P.BOUNDS + ("N",)}
    assert {c.name.split("/")[1].split("@")[0] for c in per} == {"periodic_p%d" % p for p in P.PERIODS}
    tiny = P.tiny_cases()
    assert [len(c.data) for c in tiny] == list(range(4, 201))
    for c in tiny:
        L = max(4, len(c.data) // 3)
        assert c.a == len(c.data) - L
        if 2 * L <= len(c.data):  # (shorter ones: the copy lies over its own source)
            assert c.data[-L:] == c.data[:L]


def test_sweeps_meet_every_entry_phase():
    """a sweep's step is coprime to the segment sizes, and over the three inner boundaries of the full chunk the events start at
    every offset of a 24-, 48- and 64-byte segment; so they do around the seam alone for the segments that meet there (48 bytes
    below it, 24 above) and around 51456 alone for those of sub-pass B and of k_lz_walk (24, 64)"""
    import math
    for s in P.STEPS:
        assert math.gcd(s, 48) == 1 and math.gcd(s, 64) == 1
    for level in LEVELS:
        cases = [c for c in P.chunk_cases(level) if len(c.data) == P.N_FULL and c.bound != "N"]
        for seg in (24, 48, 64):
            assert len({c.a % seg for c in cases}) == seg, (level, seg)
        for bound, segs in ((49152, (24, 48)), (51456, (24, 64))):
            for seg in segs:
                assert len({c.a % seg for c in cases if c.bound == bound}) == seg, (level, bound, seg)


def test_the_guard_of_copy_breaks_a_chance_agreement():
    import numpy as np
    rng = np.random.default_rng(1)
    buf = np.full(100, 200, np.uint8)
    buf[50:60] = np.arange(10)
    P.copy(rng, buf, 20, 50, 10)
    assert bytes(buf[20:30]) == bytes(range(10)) and buf[19] != buf[49] and buf[30] != buf[60]
