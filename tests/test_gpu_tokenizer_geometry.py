"""GPU parity of the tokenizers on inputs placed against their own geometry (tests/_planted.py): one planted match, ladder of lazily
improving matches, candidate on / one past the distance limit, or run, at every entry phase of a segment around a segment start
(14400, 51456), the seam of the two sub-passes (49152) and the chunk's end, at chunk lengths on either side of the seam and of the
seam + 256; the same events around the interior and the seam of a stream's second window.  k_lz_parse (levels 4..7), k_lz_walk
(levels 8..9, and 4..7 in the walkall build), k_lz_parse<true> / k_lz_walk<true> (streams): the bytes are the oracle's.
tests/test_planted_cpu.py shows, without a GPU, that every input holds the event its name says."""
import os

import numpy as np
import pytest

import _oracle as O
import _planted as P
from gpu_util import engine

pytestmark = pytest.mark.gpu


def _first_difference(eng, case, level):
    """the case alone (debug_tokens of a batch of one: the index does not depend on how a large batch is cut into passes):
    its name, `a`, the first token that differs from the oracle's and that token's position in the input"""
    outs, st = eng.compress_many([case.data], O.RAW, level)
    got = eng.debug_tokens(0)
    want = O.tokenize(case.data, level)
    m = min(len(got), len(want))
    bad = np.nonzero(got[:m] != want[:m])[0]
    first = int(bad[0]) if bad.size else m
    starts, _ = P.token_starts(want)
    return {"case": case.name, "a": case.a, "level": level, "status alone": st, "token": first,
            "position": int(starts[first]) if first < len(want) else len(case.data),
            "got": O.tok_decode(got[first]) if first < len(got) else None,
            "want": O.tok_decode(want[first]) if first < len(want) else None,
            "alone": "same bytes as the oracle" if outs[0] == O.compress(case.data, O.RAW, level) else "differs too"}


def _check_parity(eng, cases, level):
    outs, st = eng.compress_many([c.data for c in cases], O.RAW, level)
    assert st == [0] * len(cases), (level, [(c.name, s) for c, s in zip(cases, st) if s][:5])
    bad = [i for i, (c, got) in enumerate(zip(cases, outs)) if got != O.compress(c.data, O.RAW, level)]
    if bad:
        raise AssertionError("%d of %d differ from the oracle: %s; the first of them alone: %s" % (
            len(bad), len(cases), [cases[i].name for i in bad[:20]], _first_difference(eng, cases[bad[0]], level)))


@pytest.mark.parametrize("level,background", [(lv, bg) for lv in (4, 5, 6, 7, 8, 9) for bg in ("junk", "text")],
                         ids=lambda v: str(v))
def test_planted_chunks(level, background):
    _check_parity(engine(), P.chunk_cases(level, background), level)


@pytest.mark.parametrize("level", [4, 6, 7, 9])
def test_planted_periodic_and_tiny(level):
    _check_parity(engine(), list(P.periodic_cases()) + list(P.tiny_cases()), level)


@pytest.mark.parametrize("windows", ["", "1"])
@pytest.mark.parametrize("level", [4, 5, 6, 7, 8, 9])
def test_planted_streams(level, windows, monkeypatch):
    if windows:
        monkeypatch.setenv("FLATE_HIP_STREAM_WINDOWS", windows)
    eng = engine()
    if not (windows == "1" and level <= 7):
        _check_parity(eng, P.stream_cases(level), level)
        return
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        _check_parity(eng, P.stream_cases(level), level)
        prof = eng.profile_read()
    finally:
        eng.profile_enable(False)
    # the seam under test is the one that ran
    assert "k_lz_parse" in prof and "k_lz_sort" not in prof and "k_lz_match" not in prof, prof


def test_planted_chunks_on_the_variant_builds():
    # the build with -DFL_BULK_MIN_CHAIN=1 sends levels 4-7 through k_lz_links / k_lz_walk (64-byte segments): the junk lists of
    # levels 4 and 6 there (its own process: the library is chosen at import)
    import subprocess
    import sys
    engine()  # (skips without a GPU, as the child's tests would)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "flate_amd", "lib", "var", "libflate_hip_walkall.so")
    assert os.path.exists(lib), "build() makes it (`make variants` in flate_amd/csrc)"
    env = dict(os.environ, FLATE_HIP_LIB=lib)
    me = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", me + "::test_planted_chunks[4-junk]",
                        me + "::test_planted_chunks[6-junk]"], env=env, capture_output=True, text=True, cwd=root)
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
