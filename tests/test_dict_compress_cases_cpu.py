"""CPU checks of tests/_dict_compress_cases.py, the yardstick of flate_hip_compress_batch_dict: every expectation is a
stream stdlib zlib inflates to the record with the dictionary's tail (raw) or the whole dictionary (zlib) as zdict, the
planted cases exercise what they are planted for, and flate_hip_compress_bound + 4 bytes hold every stream."""
import zlib as pyzlib

import pytest

import _dict_compress_cases as dc
import _oracle as O


def inflate(z, container, d):
    o = pyzlib.decompressobj(-15, zdict=dc.tail(d)) if container == O.RAW else pyzlib.decompressobj(15, zdict=d)
    out = o.decompress(z)
    assert o.eof and not o.unused_data
    return out


def covered(tokens):
    return sum(1 if t[0] == "L" else t[2] for t in map(O.tok_decode, tokens))


@pytest.mark.parametrize("level", dc.LEVELS)
def test_every_expectation_inflates_with_stdlib_zlib(level):
    for c in dc.CASES:
        for container in dc.CONTAINERS:
            z = dc.expected(c.zdict, c.rec, level, container)
            assert inflate(z, container, c.zdict) == c.rec, (c.name, container)
        assert covered(dc.expected_tokens(c.zdict, c.rec, level)) == len(c.rec), c.name
        z = dc.expected(c.zdict, c.rec, level, O.ZLIB)
        assert z[:2] == b"\x78\xbb" and int.from_bytes(z[:2], "big") % 31 == 0
        assert z[2:6] == pyzlib.adler32(c.zdict).to_bytes(4, "big") and z[-4:] == pyzlib.adler32(c.rec).to_bytes(4, "big")
        assert z[6:-4] == dc.expected(c.zdict, c.rec, level, O.RAW)


def test_the_shapes_are_all_there():
    lens = {len(c.zdict) for c in dc.CASES if c.name.startswith("shape_")}
    assert lens == set(dc.DICT_LENS)
    assert {len(c.rec) for c in dc.CASES} >= set(dc.SMALL_N)
    ends = {min(len(c.zdict), dc.WINDOW) + len(c.rec) for c in dc.CASES}
    assert ends >= set(dc.ENDS)
    big = dc.BY_NAME["shape_d40000_n%d" % dc.SMALL_N[19 % 5]]
    assert dc.expected(big.zdict, big.rec, 6, O.ZLIB)[2:6] == pyzlib.adler32(big.zdict).to_bytes(4, "big")  # DICTID: all of it
    assert dc.expected(big.zdict, big.rec, 6, O.RAW) == dc.expected(big.zdict[-dc.WINDOW:], big.rec, 6, O.RAW)  # history: the tail


@pytest.mark.parametrize("level", dc.LEVELS)
def test_empty_dictionary_is_the_plain_stream_with_fdict(level):
    for c in dc.CASES:
        if len(c.zdict) == 0:
            assert dc.expected(c.zdict, c.rec, level, O.RAW) == O.compress(c.rec, O.RAW, level), c.name
            z = dc.expected(c.zdict, c.rec, level, O.ZLIB)
            assert z[:6] == b"\x78\xbb\x00\x00\x00\x01" and z[6:] == O.compress(c.rec, O.ZLIB, level)[2:], c.name


@pytest.mark.parametrize("level", dc.LEVELS)
def test_the_three_positions_before_the_seam_are_no_candidates(level):
    """(c): the 8-byte string that starts 4 bytes before the seam is found whole (distance 24), the one that starts 1, 2
    or 3 bytes before it only from the record's first byte on: the exclusion is what the case exercises"""
    for k in (1, 2, 3, 4):
        c = dc.BY_NAME["straddle_k%d" % k]
        m = [t for t in map(O.tok_decode, dc.expected_tokens(c.zdict, c.rec, level)) if t[0] == "M"]
        assert m == ([("M", 24, 8)] if k == 4 else [("M", 20 + k, 8 - k)]), (k, m)


@pytest.mark.parametrize("level", dc.LEVELS)
def test_planted_matches_reach_into_the_dictionary(level):
    def toks(name):
        c = dc.BY_NAME[name]
        return list(map(O.tok_decode, dc.expected_tokens(c.zdict, c.rec, level)))
    # (a) position 0 of T is the chain's null: the record's first byte is a literal, the rest comes from distance 32768
    assert toks("far_prefix_258")[:2] == [("L", dc.BY_NAME["far_prefix_258"].rec[0]), ("M", 32768, 257)]
    assert ("M", 32768, 258) in toks("far_prefix_from_1")
    assert toks("far_prefix_long_dict")[1] == ("M", 32768, 257)
    # (b) the source begins 8 bytes before the seam and runs on into the record
    t = toks("source_runs_past_seam")
    assert t[:12] == [("L", b) for b in dc.BY_NAME["source_runs_past_seam"].rec[:12]] and t[12] == ("M", 20, 40)
    # ... a run from the dictionary's last bytes: from D - 5 it is found (distance 4), from D - 1 alone it is not
    assert toks("run_from_five_bytes")[0] == ("M", 4, 258)
    assert toks("run_from_last_byte")[:2] == [("L", ord("z")), ("M", 1, 258)]
    # (d)
    assert toks("same_byte_both")[0][0] == "M"
    assert toks("same_byte_dict_other_byte_rec")[:2] == [("L", ord("b")), ("M", 1, 258)]  # (nothing of it is in T)
    # (e) the matches at the record's first three positions each lose to the next position's
    t = toks("lazy_chain_at_start")
    if level == 4:  # (lazy = 4: the first position's 4-byte match goes out at once)
        assert t[0][0] == "M" and t[0][2] == 4
    else:
        assert [x[0] for x in t[:4]] == ["L", "L", "L", "M"] and t[3][2] == 13
    # (f) compared, not assumed: text against noise is the plain stream, and so is noise against noise
    for name in ("no_match_noise", "no_match_text"):
        c = dc.BY_NAME[name]
        assert all(x[0] == "L" or x[1] <= covered_before(toks(name), i) for i, x in enumerate(toks(name)))
        assert dc.expected(c.zdict, c.rec, level, O.RAW) == O.compress(c.rec, O.RAW, level), name


def covered_before(tokens, i):
    return sum(1 if t[0] == "L" else t[2] for t in tokens[:i])


def test_records_compress_against_their_dictionary():
    """the shape the call is made for: 200 bytes cut out of a 32 KiB dictionary are one match -- a block header, a length
    and a distance code, the end of the block: 16 bytes at the very most -- where they are over 100 bytes alone"""
    d = dc.TEXT[20000:20000 + dc.WINDOW]
    for level in dc.LEVELS:
        for at in (0, 5000, 32000):
            rec = d[at:at + 200]
            assert len(dc.expected(d, rec, level, O.RAW)) <= 16 < 100 < len(O.compress(rec, O.RAW, level))


@pytest.mark.parametrize("level", dc.LEVELS)
def test_slot_of_compress_bound_plus_4_holds_every_stream(level):
    from flate_amd import _capi
    bound = _capi.lib().flate_hip_compress_bound
    for n in dc.BOUND_N:
        rec = dc.noise(1000 + n, n)
        for d in (b"", dc.noise(7, 4095), dc.noise(8, dc.WINDOW)):
            if len(d) + n > dc.MAX_STREAM:
                continue
            for container in dc.CONTAINERS:
                z = dc.expected(d, rec, level, container)
                assert len(z) <= bound(n, container, level) + 4, (n, len(d), container, len(z))
    for c in dc.CASES:
        for container in dc.CONTAINERS:
            assert len(dc.expected(c.zdict, c.rec, level, container)) <= bound(len(c.rec), container, level) + 4, c.name


def test_mixed_batch_has_every_kind():
    recs, dicts, of = dc.mixed_batch()
    assert set(of) == {0, 1, 2, None} and dicts[2] == b""
    assert any(o is None and len(r) > 65535 for r, o in zip(recs, of)) and any(o is None and len(r) <= 65535 for r, o in zip(recs, of))
    assert all(o is None or min(len(dicts[o]), dc.WINDOW) + len(r) <= dc.MAX_STREAM for r, o in zip(recs, of))
