"""Streams for the seek index (flate_hip_index_build / flate_hip_decompress_ranges; test infrastructure), with what they decode
to and where their blocks start.

`CASES`: list of Case(name, container, stream, full, spacing, status, block_starts, block_pos, ranges).  container 0 = raw,
1 = gzip, 2 = zlib; full = the bytes the stream must decode to; status = what the build's decode says (a stream whose status is
not 0 has no points); block_starts = [(bit, pos)] of every block in stream order, bit counted from the stream's first byte with
the container's header included, or None where the bits are not known; block_pos = the positions alone (always known);
ranges = [(begin, len)].

Family S: synthesized streams (_deflate_synth.Stream over the bit writer of _inflate_edge_cases.py, and the streams of
          _deflate_synth.random_streams written again block by block): every block start is known by construction.
Family Z: streams stdlib zlib made, compressobj.flush(Z_BLOCK / Z_SYNC_FLUSH / Z_FULL_FLUSH) at known input cuts.  Every segment
          is shorter than 16383 bytes, so it is one block (zlib closes a block by itself only when its 16383 symbols are used
          up); a sync or full flush adds an empty stored block at the same position.  The positions are known, the bits are not.

The point rule is restated here in Python (expected_points); tests/test_index_cases_cpu.py checks every case against stdlib zlib.
"""
import collections
import os
import random
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _deflate_synth as DS  # noqa: E402
from _deflate_synth import Stream  # noqa: E402
from flate_amd import synth  # noqa: E402

Case = collections.namedtuple("Case", "name container stream full spacing status block_starts block_pos ranges")
CASES = []
TEXT = bytes(synth.text(7, 1 << 20))
WINDOW = 32768
GZIP_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"
ZLIB_HEADER = b"\x78\x9c"
HEADER_BYTES = {0: 0, 1: len(GZIP_HEADER), 2: len(ZLIB_HEADER)}


def wrap(raw, full, container):
    """a raw deflate stream in its container"""
    if container == 1:
        return GZIP_HEADER + raw + struct.pack("<II", zlib.crc32(full), len(full) & 0xffffffff)
    if container == 2:
        return ZLIB_HEADER + raw + struct.pack(">I", zlib.adler32(full))
    return raw


def point_rule(pos, spacing):
    """indices of the block starts that are points: block 0, and every block whose predecessor holds a grid line"""
    return [k for k in range(len(pos)) if k == 0 or pos[k] // spacing > pos[k - 1] // spacing]


def expected_points(case):
    """[(bit or None, pos)] of the case's points; [] for a stream that fails"""
    if case.status != 0:
        return []
    which = point_rule(case.block_pos, case.spacing)
    return [(case.block_starts[k][0] if case.block_starts else None, case.block_pos[k]) for k in which]


def silent_prefix(k):
    """Blocks of k mod 8 bits in all that produce nothing, as a list of bits: empty fixed blocks (10 bits each) and, for an odd
    k, one empty dynamic block of 95 bits (HCLEN 19; code lengths by the code 18 -> 0, 0 -> 10, 1 -> 11; 256 zeros as two
    repeats, a 1-bit code for symbol 256 alone, one distance code of no bits)."""
    w = DS.BW()
    if k & 1:
        w.bits(0, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(15, 4)
        for sym in DS.CLORD:
            w.bits({18: 1, 0: 2, 1: 2}.get(sym, 0), 3)
        w.code(0, 1); w.bits(127, 7); w.code(0, 1); w.bits(107, 7); w.code(3, 2); w.code(2, 2)
        w.code(0, 1)
    for _ in range(((k - 7) % 8 if k & 1 else k) // 2):
        w.bits(0, 1); w.bits(1, 2); w.code(0, 7)
    n = len(w.b) * 8 + w.n
    assert n % 8 == k
    return np.unpackbits(np.frombuffer(w.done(), np.uint8), bitorder="little")[:n]


def shift_and_reinflate(stream, in_bit, out_pos, full):
    """The property that makes (in_bit, out_pos) a block start of the stream: with the first in_bit bits dropped, what is left
    is a raw stream that inflates to full[out_pos:] against the 32 KiB in front of out_pos.  True when zlib agrees.
    (A stored block further on pads to the ORIGINAL stream's byte grid, so the bits are not simply repacked from in_bit: they
    keep their place in their bytes, behind in_bit mod 8 bits of blocks that produce nothing.  With in_bit on a byte boundary
    that is the plain cut.)"""
    bits = np.unpackbits(np.frombuffer(stream, np.uint8), bitorder="little")[in_bit:]
    data = np.packbits(np.concatenate([silent_prefix(in_bit & 7), bits]), bitorder="little").tobytes()
    zdict = full[max(0, out_pos - WINDOW):out_pos]
    d = zlib.decompressobj(-15, zdict=zdict) if zdict else zlib.decompressobj(-15)
    try:
        got = d.decompress(data)
    except zlib.error:
        return False
    return d.eof and got == full[out_pos:]


def make_ranges(pos_points, size, extra=()):
    """begin at a point, one before, one behind; at 0, size - 1, size and beyond; length 0; across three points; everything"""
    pts = sorted(set(pos_points))
    pick = pts[:5] + pts[-3:] if len(pts) > 8 else pts
    out = []
    for k, p in enumerate(pick):
        out.append((p, 1 + 37 * k))
        if p:
            out.append((p - 1, 3 + k))
        out.append((p + 1, 700 + k))
    out += [(0, 10), (0, 0), (size // 2, 0), (size, 4), (size + 100, 4), (size, 0), (0, size), (0, size + 5), (3, 1 << 63),
            (1 << 63, 1 << 63), ((1 << 64) - 1, (1 << 64) - 1)]
    if size:
        out += [(size - 1, 5), (size - 1, 1), (size // 3, size // 3 + 1)]
    if len(pts) >= 4:
        out.append((pts[1] - 1, pts[3] - pts[1] + 3))  # from in front of point 1 to behind point 3
        out.append((pts[-3] + 1, size))
    out += list(extra)
    return out


def _add(name, container, raw, full, spacing, starts=None, pos=None, status=0, stream=None, extra=()):
    full = bytes(full)
    hb = HEADER_BYTES[container] * 8
    if starts is not None:
        starts = [(b + hb, p) for b, p in starts]
        pos = [p for _, p in starts]
    pts = [pos[k] for k in point_rule(pos, spacing)] if status == 0 else []
    CASES.append(Case(name, container, bytes(stream if stream is not None else wrap(raw, full, container)), full, spacing, status,
                      starts, list(pos), make_ranges(pts, len(full), extra)))


class Rec:
    """a Stream that notes every block start"""

    def __init__(self, seed):
        self.s = Stream(seed)
        self.starts = []

    def _note(self):
        self.starts.append((self.s.bitpos(), len(self.s.hist)))

    def fixed(self, toks, final=0):
        self._note()
        self.s.fixed(toks, final)

    def stored(self, data, final=0):
        self._note()
        self.s.stored(data, final)

    def history(self, n):
        self._note()
        self.s.history(n)

    def random_block(self, ntok, final):
        self._note()
        DS.random_block(self.s, ntok, final)

    def done(self):
        raw, full = self.s.done()
        assert full is not None
        return raw, full


# ---- Family S ------------------------------------------------------------------------------------------------------------
def _tiny_fixed(seed, n_blocks):
    """a few hundred fixed blocks of 0..4 literals (8- and 9-bit codes: the block starts visit every bit residue)"""
    r = Rec(seed)
    rng = random.Random(seed)
    for b in range(n_blocks):
        r.fixed([("L", rng.randrange(256)) for _ in range(rng.choice((0, 1, 1, 2, 3, 4)))], int(b == n_blocks - 1))
    return r


def _family_s():
    # spacing 1: every block behind a block that is not empty is a point; every window is short
    r = _tiny_fixed(11, 300)
    raw, full = r.done()
    for container in (0, 1, 2):
        _add("S_tiny300_c%d" % container, container, raw, full, 1, r.starts)
    _add("S_tiny300_s7", 0, raw, full, 7, r.starts)

    # a point, and right behind it a match of distance exactly 32768: its source is the window's first byte;
    # then a match whose source starts in the window and whose copy runs on into the new bytes
    r = Rec(21)
    r.history(40000)
    r.fixed([("M", 100, 32768), ("L", 65), ("M", 258, 32768)])
    r.history(40000 - 359)
    r.fixed([("M", 200, 7), ("M", 258, 1), ("L", 66)])
    r.history(40000 - 459)
    r.fixed([("L", 1), ("M", 30, 32768)], 1)
    raw, full = r.done()
    assert [p for _, p in r.starts] == [0, 40000, 40359, 80000, 80459, 120000]
    _add("S_dist32768", 0, raw, full, 40000, r.starts)
    _add("S_dist32768_gz", 1, raw, full, 40000, r.starts)

    # ... and with a short window: distance == out_pos, the window's first byte again; and an overlapping copy out of it
    r = Rec(22)
    r.history(1000)
    r.fixed([("M", 50, 1000), ("M", 3, 1050)])
    r.history(947)
    r.fixed([("M", 258, 3), ("M", 258, 2000)], 1)
    raw, full = r.done()
    assert [p for _, p in r.starts] == [0, 1000, 1053, 2000]
    _add("S_dist_eq_pos", 2, raw, full, 1000, r.starts)

    # stored blocks that begin at points; ranges that end inside them
    rng = random.Random(23)
    r = Rec(23)
    r.history(5000)
    r.stored(bytes(rng.randrange(256) for _ in range(3000)))
    r.history(2000)
    r.stored(bytes(rng.randrange(256) for _ in range(65535)))
    r.stored(b"")
    r.stored(bytes(rng.randrange(256) for _ in range(40000)), 1)
    raw, full = r.done()
    _add("S_stored_at_points", 0, raw, full, 5000, r.starts, extra=[(5100, 50), (10001, 70000), (75535, 10), (75536, 40000)])

    # one fixed block of one literal and 1024 matches of length 258: only point 0, a range at its end skips about 260 KiB
    r = Rec(24)
    r.fixed([("L", 90)] + [("M", 258, 1)] * 1024, 1)
    raw, full = r.done()
    assert len(full) == 1 + 1024 * 258
    _add("S_one_long_fixed", 0, raw, full, 4096, r.starts, extra=[(len(full) - 300, 300), (len(full) - 1, 1), (260 * 1024, 1000)])

    # block starts exactly on a grid line, one byte before one and one byte behind one
    r = Rec(25)
    for n in (1000, 999, 1002, 998, 1, 1, 999, 2000, 1):
        r.stored(bytes(rng.randrange(256) for _ in range(n)))
    r.fixed([("L", 7)], 1)
    raw, full = r.done()
    assert [p for _, p in r.starts] == [0, 1000, 1999, 3001, 3999, 4000, 4001, 5000, 7000, 7001]
    _add("S_grid_edges", 0, raw, full, 1000, r.starts)
    assert [p for _, p in expected_points(CASES[-1])] == [0, 1000, 3001, 4000, 5000, 7000]

    # the empty stream and a one-block stream
    r = Rec(26)
    r.stored(b"", 1)
    raw, full = r.done()
    for container in (0, 1, 2):
        _add("S_empty_c%d" % container, container, raw, full, 1, r.starts)
    r = Rec(27)
    r.fixed([("L", c) for c in b"hello"], 1)
    raw, full = r.done()
    _add("S_one_block", 1, raw, full, 1 << 20, r.starts)

    # the streams of _deflate_synth.random_streams, written again with their block starts noted
    seeds = list(range(9000, 9010))
    again = DS.random_streams(seeds[0], len(seeds))
    for seed, (stream, want) in zip(seeds, again):
        r = Rec(seed)
        nb = r.s.rng.randint(1, 6)
        for b in range(nb):
            r.random_block(r.s.rng.choice((0, 1, 50, 3000)), int(b == nb - 1))
        raw, full = r.done()
        assert raw == stream and full == want
        _add("S_random_%d" % seed, seed % 3, raw, full, (64, 1024, 5000)[seed % 3], r.starts)

    # long random streams: dynamic blocks of thousands of tokens, matches of every distance across the points
    for k in range(2):
        r = Rec(9100 + k)
        while len(r.s.hist) < 300000:
            r.random_block(r.s.rng.choice((50, 3000, 20000)), 0)
        r.random_block(100, 1)
        raw, full = r.done()
        _add("S_big_random_%d" % k, (1, 2)[k], raw, full, (32768, 100000)[k], r.starts)


# ---- Family Z ------------------------------------------------------------------------------------------------------------
FLUSHES = (zlib.Z_BLOCK, zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH)
Z_FLUSHES = {}  # name -> sync and full flushes of the stream (each leaves an empty stored block)


def zlib_segments(data, cuts, modes, level, wbits):
    """data compressed with a flush of modes[i] at every cut -> (stream, block positions)"""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits)
    out, pos, at = [], [], 0
    for cut, mode in zip(list(cuts) + [len(data)], list(modes) + [None]):
        assert 0 < cut - at < 16383
        pos.append(at)
        out.append(co.compress(data[at:cut]))
        at = cut
        if mode is None:
            out.append(co.flush())
        else:
            out.append(co.flush(mode))
            if mode != zlib.Z_BLOCK:
                pos.append(at)  # the empty stored block
    return b"".join(out), pos


def _family_z():
    for k, (container, wbits) in enumerate(((0, -15), (1, 31), (2, 15))):
        rng = random.Random(300 + k)
        n_seg = 40
        lens = [rng.choice((1, 200, 3000, 9000, 16000)) for _ in range(n_seg)]
        data = TEXT[1000 * k:1000 * k + sum(lens)]
        cuts = list(np.cumsum(lens))[:-1]
        modes = [FLUSHES[rng.randrange(3)] for _ in cuts]
        for level, spacing in ((6, 20000), (1, 4096)):
            stream, pos = zlib_segments(data, cuts, modes, level, wbits)
            _add("Z_c%d_l%d" % (container, level), container, None, data, spacing, pos=pos, stream=stream)
            Z_FLUSHES[CASES[-1].name] = sum(m != zlib.Z_BLOCK for m in modes)
    # a sync flush's empty stored block that is itself the point
    data = TEXT[:30000]
    stream, pos = zlib_segments(data, [10000, 20000], [zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH], 6, 31)
    assert pos == [0, 10000, 10000, 20000, 20000]
    _add("Z_sync_is_point", 1, None, data, 10000, pos=pos, stream=stream)
    Z_FLUSHES["Z_sync_is_point"] = 2
    # a wrong footer: the stream fails in the build and gets no points
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    good = co.compress(TEXT[:50000]) + co.flush()
    bad = bytearray(good)
    bad[-8] ^= 1
    _add("Z_bad_crc", 1, None, b"", 4096, pos=[0], status=4, stream=bytes(bad))
    co = zlib.compressobj(6, zlib.DEFLATED, 15)
    good = co.compress(TEXT[:50000]) + co.flush()
    bad = bytearray(good)
    bad[-1] ^= 1
    _add("Z_bad_adler", 2, None, b"", 4096, pos=[0], status=6, stream=bytes(bad))


_family_s()
_family_z()
NAMES = [c.name for c in CASES]
assert len(set(NAMES)) == len(NAMES)
BY_NAME = {c.name: c for c in CASES}
