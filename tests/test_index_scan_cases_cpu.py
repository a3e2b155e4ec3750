"""tests/_index_scan_cases.py against stdlib zlib: the streams inflate to what the cases say, the expected points are fresh and
the dropped kept marks are not, and no family has gone empty."""
import zlib

import pytest

import _index_cases as IC
import _index_scan_cases as SC


def _inflate(c):
    d = zlib.decompressobj(SC.WBITS[c.container])
    got = d.decompress(c.stream)
    assert d.eof and d.unused_data == b""
    return got


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_holds_against_zlib(name):
    c = SC.BY_NAME[name]
    assert _inflate(c) == c.full
    hb = 8 * IC.HEADER_BYTES[c.container]
    assert c.points[0] == (hb, 0)
    # every mark is a block start behind an empty stored block: the bytes in front of it say so, and what follows it
    # inflates against the 32 KiB in front of it
    for bit, pos in c.marks:
        assert bit % 8 == 0 and c.stream[bit // 8 - 4:bit // 8] == b"\x00\x00\xff\xff", (name, bit)
        assert IC.shift_and_reinflate(c.stream, bit, pos, c.full), (name, bit, pos)
    assert [p for _, p in c.marks] == sorted(p for _, p in c.marks)
    kept = [c.marks[k] for k in SC.kept_marks(c.marks, c.spacing)]
    assert len(kept) <= len(c.full) // c.spacing
    # every expected point passes the no-dictionary probe, every dropped kept mark fails it
    for m in kept:
        assert SC.fresh_by_zlib(c.stream, m[0], m[1], c.full) == (m in c.points), (name, m)
    assert c.points[1:] == [m for m in kept if m in c.points]
    for a, b in zip(c.points, c.points[1:]):
        assert a[0] < b[0] and a[1] < b[1], name


def test_freshness_is_the_definition_on_the_planted_cases():
    """the zlib probe agrees with the definition where the tokens are known: fresh iff no match at p >= c has p - distance < c
    -- checked on the cases whose single interesting match is planted, through the asserts of _index_scan_cases itself, and
    here through the outcomes they recorded"""
    edges = ["near_k1", "near_k2", "near_k258", "far_dynamic", "far_fixed", "two_first", "two_second", "unkept"]
    for e in edges:
        assert SC.OUTCOMES.get(e) == {True, False}, (e, SC.OUTCOMES.get(e))


def test_no_family_is_empty():
    z = [c for c in SC.CASES if c.name.startswith("Z_")]
    assert len(z) == 18 and sorted(set(c.container for c in z)) == [0, 1, 2]
    for c in z:
        assert len(c.marks) >= 10
        if c.spacing == 1:
            kept = SC.kept_marks(c.marks, 1)
            fresh = len(c.points) - 1
            assert fresh >= 3 and len(kept) - fresh >= 3, (c.name, fresh, len(kept))
        else:
            assert len(SC.kept_marks(c.marks, c.spacing)) < len(c.marks)
    p = [c for c in SC.CASES if c.name.startswith("P_")]
    assert len(p) >= 40
    assert any(len(c.full) == 0 for c in p) and any(c.marks and c.marks[-1][1] == len(c.full) for c in p)
    assert sorted(set(c.container for c in p)) == [0, 1, 2]


def test_the_span_case():
    c = SC.span_case()
    assert _inflate(c) == c.full and 32768 <= len(c.stream) < 2 * 32768
    kept = SC.kept_marks(c.marks, 1)
    assert len(kept) == len(c.marks) == 74
    fresh = [m for m in c.marks if m in c.points]
    assert len(c.points) == 1 + len(fresh)
    assert (40000 in [p for _, p in fresh]) and (110000 in [p for _, p in fresh])
    # in front of every possible cut a mark that is not fresh lies within 32 KiB: no two stale marks are further apart
    stale = [p for b, p in c.marks if (b, p) not in c.points]
    assert stale[0] < 32768 and all(b - a < 32768 for a, b in zip(stale, stale[1:])) and len(c.full) - stale[-1] < 32768
