"""GPU parity of sync flush on inputs placed against the flush handling's own geometry (tests/_planted_flush.py): a match, the
source of a match, a run, a ladder of lazily improving matches or a candidate on / one past the distance limit planted ON a flush
point F, with F on and around every window start, slide zone, sub-pass seam and the stream's end, one flush point or several,
finished or not; uniform bytes whose blocks lose their input by where F lies.  k_lz_chain<true> / k_lz_parse<true> (levels 4..7),
the sort / match tiles (levels 8..9, and 4..7 with FLATE_HIP_STREAM_WINDOWS=0): the bytes are the oracle's streaming compressor's,
fed the same writes and flushes.  The Compressor object, which drops the history a flush can no longer depend on, is held to the
oracle on events that reach back exactly as far as a window does.  tests/test_planted_flush_cpu.py shows, without a GPU, that every
input holds the event its name says.

Wall time on one MI355X, the oracle's share included: test_planted_flush_streams 0.75 .. 0.94 s per parameter (249 .. 294 streams;
2.9 s for the first, which makes the engine), test_compressor_object_... 0.48 .. 0.54 s per mode (48 streams, four calls each),
test_planted_flush_containers 0.23 s.

What the list notices.  Builds with ONE decision made wrong on purpose (tried, not kept) fail test_planted_flush_streams in:
  * k_lz_chain<true>, `valid`: `>= 4u` -> `>= 3u` (F - 3 enters the table): [4..7-], 20 cases -- source_j-3_near@14400-1
    (M(3003, 20) for three literals and M(3003, 17)), @49152-2, @73728-2, @98304-2 (also as `FF`), source_j-3_D32768@98042-1, and
    the 14 run_*_half cases;
  * k_lz_parse<true>, the `maxlen` clamp removed: [4..7-], 42 .. 46 cases -- straddles with k >= 4 at every boundary
    (straddle_L5_D1000_k4@14400+25 first: M(1000, 5) at F - 4 for M(1000, 4); straddle_L258_D1000_k4@32768+0,
    straddle_L258_D32768_k5@49152+0, straddle_L258_D1000_k257@65274+0, straddle_L5_D32768_k4@98304+11 among the first 20);
  * k_lz_parse<true>, `has_fl`'s horizon `+ 65536 + 300` -> `+ 65536 - 300`: [4..7-], 12 .. 13 cases, all with F in the last 300
    bytes of a window -- straddle_L33_D1000_k29@65274-11, straddle_L258_D1000_k257@65274+0 and @98042+0 (also as `F-4,F`),
    straddle_L33_D1000_k30@98304-11, run_700_half@65274+0, run_259_half@65536-9, ladder_6_d-5@65274+11;
  * the tiles' `maxlen` clamp removed (kernels_lz.h): [8-], [9-], [4..7-0], 54 cases, the same straddles first;
  * the tiles' horizon `w0 + Mpos + 2 + FL_MAX_MATCH` without its last term: [8-], [9-], [4..7-0], 2 cases --
    run_700_half@65536+14 and run_700_half@98304+11 (M(1, 258) over F for M(1, 91): the match starts in the tile before F's)."""
import io
import zlib

import numpy as np
import pytest

import _oracle as O
import _planted as P
import _planted_flush as PF
from gpu_util import engine
from test_planted_flush_cpu import oracle_stream

pytestmark = pytest.mark.gpu

WBITS = {O.RAW: -15, O.GZIP: 31, O.ZLIB: 15}


def _inflates(case, stream, container=O.RAW):
    try:
        if case.finish:
            return zlib.decompress(stream, WBITS[container]) == case.data
        return zlib.decompressobj(WBITS[container]).decompress(stream) == case.data
    except zlib.error:
        return False


def _first_difference(eng, case, level):
    """the case again (debug_tokens shows the last call): its name, F, `a`, the first token that differs from the oracle's token
    log and that token's position in the input"""
    got_bytes, st = eng.compress_flush(case.data, case.flushes, case.finish, O.RAW, level)
    got = eng.debug_tokens(0)
    want_bytes, want, _ = oracle_stream(case, level)
    m = min(len(got), len(want))
    bad = np.nonzero(got[:m] != want[:m])[0]
    first = int(bad[0]) if bad.size else m
    starts, _ = P.token_starts(want)
    return {"case": case.name, "F": case.F, "a": case.a, "flushes": case.flushes, "finish": case.finish, "level": level,
            "status": st, "bytes": (len(got_bytes), len(want_bytes)), "tokens": (len(got), len(want)), "token": first,
            "position": int(starts[first]) if first < len(want) else len(case.data),
            "got": O.tok_decode(got[first]) if first < len(got) else None,
            "want": O.tok_decode(want[first]) if first < len(want) else None}


# (levels 8-9 with flush points run the tiles whatever the knob says)
@pytest.mark.parametrize("level,windows", [(lv, "") for lv in (4, 5, 6, 7, 8, 9)] + [(lv, "0") for lv in (4, 5, 6, 7)])
def test_planted_flush_streams(level, windows, monkeypatch):
    if windows:
        monkeypatch.setenv("FLATE_HIP_STREAM_WINDOWS", windows)
    eng = engine()
    cases = PF.flush_cases(level)
    profiled = level <= 7
    bad, wrong_kernels = [], []
    try:
        for c in cases:
            want, _, _ = oracle_stream(c, level, log=False)
            if profiled:
                eng.profile_enable(True)
                eng.profile_reset()
            got, st = eng.compress_flush(c.data, c.flushes, c.finish, O.RAW, level)
            if profiled:
                prof = eng.profile_read()
                # the seam under test is the one that ran (a run is periodic data, which the windows may hand to the tiles)
                if windows == "0":
                    if "k_lz_match" not in prof:
                        wrong_kernels.append((c.name, sorted(prof)))
                elif c.kind != "run" and ("k_lz_parse" not in prof or "k_lz_match" in prof):
                    wrong_kernels.append((c.name, sorted(prof)))
            if got != want or st != (0 if _inflates(c, want) else 102):
                bad.append((c, st))
    finally:
        eng.profile_enable(False)
    if bad:
        raise AssertionError("%d of %d differ from the oracle: %s; the first of them: %s" % (
            len(bad), len(cases), [(c.name, st) for c, st in bad[:20]], _first_difference(eng, bad[0][0], level)))
    assert not wrong_kernels, (level, windows, len(wrong_kernels), wrong_kernels[:5])


def test_planted_flush_containers():
    """every 7th case of level 6 through gzip and zlib: header, the same deflate bytes, the footer over all pieces"""
    eng = engine()
    bad = []
    for c in PF.flush_cases(6)[::7]:
        for container in (O.GZIP, O.ZLIB):
            got, st = eng.compress_flush(c.data, c.flushes, c.finish, container, 6)
            want, _, _ = oracle_stream(c, 6, container, log=False)
            if st != 0 or got != want or not _inflates(c, got, container):
                bad.append((c.name, container, st, len(got), len(want)))
    assert not bad, (len(bad), bad[:20])


@pytest.mark.parametrize("mode", [4, 6, 9])
def test_compressor_object_drops_history_in_front_of_planted_events(mode):
    """api._Compressor compresses only the tail it kept: by the third flush point it has dropped the stream's first 32 KiB or more
    and re-based the rest.  The bytes behind that flush point must still be the oracle's when they hold a candidate at distance
    exactly 32768 (and one past it), a 258-byte match from that distance over the flush point, or a lazy chain on it"""
    engine()
    from flate_amd import api
    bad = []
    for c in PF.object_cases():
        w = io.BytesIO()
        comp = api._Compressor(O.RAW, mode, w)
        d = O.Deflate(O.RAW, mode)
        prev = 0
        for f in c.flushes:
            comp.write(c.data[prev:f])
            d.write(c.data[prev:f])
            if f == c.flushes[-1]:
                assert comp._base > 0, (c.name, comp._base)  # the history was in fact dropped
            comp.flush()
            d.flush()
            if w.getvalue() != d.output():
                bad.append((c.name, "flush at %d" % f, comp._base, len(w.getvalue()), len(d.output())))
            prev = f
        comp.write(c.data[prev:])
        d.write(c.data[prev:])
        comp.finish()
        d.finish()
        if w.getvalue() != d.output():
            bad.append((c.name, "finish", comp._base, len(w.getvalue()), len(d.output())))
        elif zlib.decompress(w.getvalue(), -15) != c.data:
            bad.append((c.name, "does not inflate to the input"))
        d.close()
    assert not bad, (mode, len(bad), bad[:20])
