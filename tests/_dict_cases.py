"""Streams that were compressed against a preset dictionary (test infrastructure), with what they must decode to.

`CASES`: list of Case(name, container, stream, zdict, status, out, consumed).  container 0 = raw, 2 = zlib; zdict None = the
stream is given no dictionary; status = the engine's status for the stream; out = the bytes delivered (for a failing stream: the
bytes in front of the failure); consumed = input bytes used (None: not pinned, the stream fails).

Family Z: streams stdlib zlib made, zlib.compressobj(level, DEFLATED, wbits, 9, 0, zdict), records and dictionaries cut from
          synth.text.  Dictionary lengths straddle near_max of both LDS rings (1788, 32508), both ring sizes and the 32 KiB window.
Family S: synthesized raw streams no encoder emits (_deflate_synth.Stream with its history pre-seeded with the dictionary), each
          once as a fixed block (the decoders' symbol-at-a-time path) and once as a dynamic block whose codes fit the lookup
          tables (the fast rounds).
Family H: zlib headers around a Family Z stream: DICTID right and wrong, FDICT without a dictionary, a dictionary without FDICT,
          cuts inside the header, a wrong footer.

The independent reference is stdlib zlib: tests/test_dict_cases_cpu.py checks every case against zlib.decompressobj(wbits, zdict).
"""
import collections
import os
import random
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from _deflate_synth import Stream, spread  # noqa: E402
from _inflate_edge_cases import fixed_lit, fixed_match  # noqa: E402
from flate_amd import synth  # noqa: E402

Case = collections.namedtuple("Case", "name container stream zdict status out consumed")
CASES = []
TEXT = bytes(synth.text(1, 1 << 18))

LEVELS = (1, 6, 9)
RECORD_LENS = (0, 1, 3, 200, 4096, 70000)
DICT_LENS = (1, 2, 257, 1788, 1789, 2047, 2048, 2049, 32508, 32509, 32767, 32768, 32769, 40000)
# A 1-byte dictionary is reachable only by a record that starts with that byte three times, a 2-byte one only by a record that
# starts x y x: the records of these two start at the first places in the text where that happens (the dictionaries are the
# text's first bytes, "h" and "hk").  zlib 1.2.11 still emits no match into them -- it does not even for b"h" * 200 against
# b"h" -- so no zlib-made RAW stream needs a dictionary of fewer than 3 bytes; NEEDS_DICT_MIN says from where on they do.
# Matches into 1- and 2-byte dictionaries are in Family S.
_TINY = {1: TEXT.find(TEXT[:1] * 3), 2: TEXT.find(TEXT[:2] + TEXT[:1])}
assert _TINY[1] > 0 and _TINY[2] > 0
NEEDS_DICT_MIN = 3


def record(dlen, rlen):
    """a slice of the text whose start lies in the part of the dictionary text[:dlen] that a match can reach"""
    if dlen in _TINY:
        return TEXT[_TINY[dlen]:_TINY[dlen] + rlen]
    lo = max(0, dlen - 32768)
    off = lo + (dlen - lo - rlen) // 2 if rlen <= dlen - lo else lo
    return TEXT[off:off + rlen]


def deflate(data, level, wbits, zdict):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, 0, zdict)
    return c.compress(data) + c.flush()


def _add(name, container, stream, zdict, status, out, consumed="len"):
    CASES.append(Case(name, container, bytes(stream), None if zdict is None else bytes(zdict), status, bytes(out),
                      (len(stream) if status == 0 else None) if consumed == "len" else consumed))


# ---- Family Z ------------------------------------------------------------------------------------------------------------
def _family_z():
    for level in LEVELS:
        for wbits in (-15, 15):
            for dlen in DICT_LENS:
                for rlen in RECORD_LENS:
                    d, r = TEXT[:dlen], record(dlen, rlen)
                    assert len(r) == rlen
                    _add("Z_l%d_w%d_d%d_r%d" % (level, wbits, dlen, rlen), 0 if wbits < 0 else 2, deflate(r, level, wbits, d), d, 0, r)
            # the empty dictionary, with a record that needs none
            r = TEXT[5000:5200]
            _add("Z_l%d_w%d_d0_r200" % (level, wbits), 0 if wbits < 0 else 2, deflate(r, level, wbits, b""), b"", 0, r)


# ---- Family S ------------------------------------------------------------------------------------------------------------
def _codes():
    """a literal/length code of at most 10 bits over every symbol and a distance code of at most 8 over every symbol: all of it in
    the decoders' lookup tables"""
    rng = random.Random(7)
    return spread(rng, 286, list(range(286)), 10, 0), spread(rng, 30, list(range(30)), 8, 0)


LL, DL = _codes()
assert max(LL) <= 10 and max(DL) <= 8


def _filler(rng, n):
    """tokens that write n bytes: 300 random literals, then matches of that far back (period 300: longer than a match)"""
    toks = [("L", rng.randrange(256)) for _ in range(min(n, 300))]
    n -= len(toks)
    while n >= 3:
        k = min(n, 258)
        if n - k in (1, 2):
            k -= 3
        toks.append(("M", k, 300))
        n -= k
    return toks + [("L", rng.randrange(256)) for _ in range(n)]


def _emit_fixed(s, toks, final):
    """Stream.fixed, which also writes a match that reaches too far back: the stream is invalid from there on"""
    s.w.bits(final, 1)
    s.w.bits(1, 2)
    for t in toks:
        if t[0] == "L":
            fixed_lit(s.w, t[1])
            if s.valid:
                s.hist.append(t[1])
        else:
            fixed_match(s.w, t[1], t[2])
            if t[2] > len(s.hist):
                s.valid = False
            if s.valid:
                hist = s.hist
                for _ in range(t[1]):
                    hist.append(hist[-t[2]])
    fixed_lit(s.w, 256)


def _synth(name, dlen, parts, status=0, seed=3):
    """parts: ("L", byte) | ("M", length, distance) | ("FILL", n) | ("STORED", n).  Written once with the tokens in fixed blocks and
    once in dynamic blocks; a stored block is a block of its own in both."""
    zdict = TEXT[1000:1000 + dlen]
    for form in ("fixed", "dyn"):
        rng = random.Random(seed)
        s = Stream(seed)
        s.hist = bytearray(zdict)
        groups, cur = [], []
        for p in parts:
            if p[0] == "STORED":
                if cur:
                    groups.append(cur)
                groups.append(p)
                cur = []
            elif p[0] == "FILL":
                cur += _filler(rng, p[1])
            else:
                cur.append(p)
        tail = [("L", rng.randrange(256)) for _ in range(6 if form == "fixed" else 64)]  # (dyn: the rounds want 192 bits ahead)
        groups.append(cur + tail)
        good = bytearray()
        for gi, g in enumerate(groups):
            final = 1 if gi == len(groups) - 1 else 0
            if g[0] == "STORED":
                s.stored(bytes(rng.randrange(256) for _ in range(g[1])), final)
            elif form == "fixed":
                _emit_fixed(s, g, final)
            else:
                s.header(final, LL, DL)
                for t in g:  # (token by token: the bytes in front of an invalid match are the case's expectation)
                    keep = None if s.valid else bytearray(s.hist)
                    s.tokens(LL, DL, [t], eob=False)
                    if keep is not None:
                        s.hist = keep
                s.tokens(LL, DL, [], eob=True)
        stream = s.w.done()
        good = bytes(s.hist[len(zdict):])
        assert (status == 0) == s.valid, name
        _add("S_%s_%s" % (name, form), 0, stream, zdict, status, good)


def _family_s():
    few = [("L", 65), ("L", 66), ("L", 67)]
    # at output position 0
    _synth("p0_dist1_len258", 1000, [("M", 258, 1)])
    _synth("p0_dist_hist", 1000, [("M", 258, 1000)])
    _synth("p0_dict_of_1_byte", 1, [("M", 258, 1)])
    _synth("p0_dict_of_2_bytes", 2, [("M", 258, 2)])
    _synth("p0_dict_of_2_bytes_dist3", 2, [("M", 258, 3)], status=11)
    _synth("p0_dist_hist_plus1", 1000, [("M", 258, 1001)], status=11)
    _synth("p3_dist_hist_plus4", 1000, few + [("M", 258, 1004)], status=11)
    _synth("p3_dist_hist_plus3", 1000, few + [("M", 258, 1003)])
    # the source starts in the dictionary and ends in the output: near, far for the small ring, far for the large ring
    _synth("straddle_near", 1000, [("FILL", 5), ("M", 258, 8)])
    _synth("straddle_far_small", 4000, [("FILL", 2000), ("M", 258, 2100)])
    _synth("straddle_far_large", 32768, [("FILL", 32600), ("M", 258, 32700)])
    # distance 32768
    _synth("d32768_wp1_dict32767", 32767, [("L", 90), ("M", 258, 32768)])
    _synth("d32768_wp1_dict32766", 32766, [("L", 90), ("M", 258, 32768)], status=11)
    _synth("d32768_wp32767", 1000, [("FILL", 32767), ("M", 258, 32768)])
    _synth("d32768_wp32768", 1000, [("FILL", 32768), ("M", 258, 32768)])
    _synth("d32768_wp0_dict32768", 32768, [("M", 258, 32768)])
    _synth("d32768_wp0_dict40000", 40000, [("M", 258, 32768)])
    # stored blocks in front of a match
    _synth("stored10_dist15", 1000, few + [("STORED", 10), ("M", 258, 15)])
    _synth("stored3000_dist3100", 4000, few + [("STORED", 3000), ("M", 258, 3100)])
    # two matches into the dictionary in one round, the second reading the first's bytes
    _synth("two_in_a_round", 1000, few + [("M", 20, 500), ("M", 20, 10)])
    # a round with more than 260 bytes of dictionary copies
    _synth("round_over_260", 1000, few + [("M", 258, 600), ("M", 258, 700), ("M", 100, 900), ("M", 30, 950)])
    _synth("round_over_260_far", 4000, few + [("M", 258, 3600), ("M", 258, 3700), ("M", 100, 3900)])


# ---- Family H ------------------------------------------------------------------------------------------------------------
def _family_h():
    d = TEXT[:2048]
    r = record(2048, 200)
    z = deflate(r, 6, 15, d)
    assert z[1] & 0x20 and z[2:6] == zlib.adler32(d).to_bytes(4, "big")
    _add("H_right_id", 2, z, d, 0, r)
    for k in range(4):
        bad = bytearray(z)
        bad[2 + k] ^= 0x10
        _add("H_id_byte%d_flipped" % k, 2, bad, d, 107, b"")
    _add("H_fdict_no_dictionary", 2, z, None, 106, b"")
    plain = zlib.compress(r, 6)
    assert not plain[1] & 0x20
    _add("H_no_fdict_with_dictionary", 2, plain, d, 0, r)
    # FDICT clear, a dictionary supplied, and the first match reaches in front of the stream's first byte: the dictionary is
    # not this stream's history
    s = Stream(1)
    s.hist = bytearray(d)
    s.fixed([("L", 97), ("L", 98), ("L", 99), ("M", 10, 8), ("L", 100)], 1)
    body = s.w.done()
    _add("H_no_fdict_match_before_start", 2, bytes([0x78, 0x9C]) + body + zlib.adler32(bytes(s.hist[len(d):])).to_bytes(4, "big"),
         d, 11, b"abc")
    for cut in (2, 3, 4, 5):
        _add("H_cut_after_%d" % cut, 2, z[:cut], d, 1, b"")
    bad = bytearray(z)
    bad[-1] ^= 1
    _add("H_footer_bit", 2, bad, d, 6, r)


_family_z()
_family_s()
_family_h()
NAMES = [c.name for c in CASES]
assert len(set(NAMES)) == len(NAMES)
BY_NAME = {c.name: c for c in CASES}
SMALL = [c for c in CASES if len(c.stream) <= 12000]  # the resumable inflater is fed these at every early split point


def zlib_inflate(c):
    """what stdlib zlib makes of a case: its output, or None when it refuses the stream"""
    wbits = -15 if c.container == 0 else 15
    try:
        o = zlib.decompressobj(wbits, c.zdict) if c.zdict is not None else zlib.decompressobj(wbits)
        out = o.decompress(c.stream)
        if not o.eof:
            return None
        return out
    except zlib.error:
        return None
