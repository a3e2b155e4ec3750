"""Streams for the scan index (flate_hip_index_scan; test infrastructure): where their flush markers lie, which of the marks
the spacing rule keeps, and which of the kept ones are fresh.

`CASES`: list of Case(name, container, stream, full, spacing, marks, points).  container 0 = raw, 1 = gzip, 2 = zlib; full =
the bytes the stream decodes to; marks = [(in_bit, out_pos)] of every block start that follows an empty stored block without
BFINAL, in stream order, in_bit counted from the stream's first byte with the container's header included; points = the
expected points: block 0 and the fresh kept marks.

The expectation is built without the library.  Marks are known by construction.  The rule is restated here (kept_marks): over
pos[0] = 0 and the marks' positions, entry k >= 1 is kept iff pos[k] // spacing > pos[k - 1] // spacing.  Freshness is decided
by stdlib zlib alone (fresh_by_zlib): the stream cut at the mark's byte, inflated as a raw stream with no dictionary, gives
exactly full[out_pos:] and ends -- or zlib raises (a distance too far back); _index_cases.shift_and_reinflate with an empty
window.

Family P (planted): synthesized streams (_deflate_synth.Stream, _index_cases.Rec) with one match at the edge in question.
Family Z: stdlib zlib streams of 40 text segments with a random Z_SYNC_FLUSH, Z_FULL_FLUSH or Z_BLOCK behind each; a mark's
          in_bit is 8 * len(output so far) once the flush has returned.  The expectation comes from the zlib probe, never from
          the flush mode: most sync-flush marks are not fresh, a few are.
tests/test_index_scan_cases_cpu.py holds every case against stdlib zlib."""
import collections
import os
import random
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _deflate_synth as DS  # noqa: E402
import _index_cases as IC  # noqa: E402

Case = collections.namedtuple("Case", "name container stream full spacing marks points")
CASES = []
OUTCOMES = {}  # edge -> set of (fresh?) seen among the planted cases that test it
TEXT = IC.TEXT
WBITS = {0: -15, 1: 31, 2: 15}


def kept_marks(marks, spacing):
    """indices into marks of the kept ones"""
    pos = [0] + [p for _, p in marks]
    return [k - 1 for k in range(1, len(pos)) if pos[k] // spacing > pos[k - 1] // spacing]


def fresh_by_zlib(stream, in_bit, out_pos, full):
    assert in_bit % 8 == 0
    d = zlib.decompressobj(-15)
    try:
        got = d.decompress(stream[in_bit // 8:])
    except zlib.error:
        return False
    assert d.eof and got == full[out_pos:], "a cut at a mark inflates without a dictionary, to other bytes"
    return True


def expected_points(container, stream, full, spacing, marks):
    pts = [(8 * IC.HEADER_BYTES[container], 0)]
    for k in kept_marks(marks, spacing):
        if fresh_by_zlib(stream, marks[k][0], marks[k][1], full):
            pts.append(marks[k])
    return pts


def add(name, container, stream, full, spacing, marks):
    CASES.append(Case(name, container, bytes(stream), bytes(full), spacing, list(marks),
                      expected_points(container, stream, full, spacing, marks)))
    return CASES[-1]


# ---- Family P --------------------------------------------------------------------------------------------------------------
class Plant(IC.Rec):
    """a Rec that knows its marks"""

    def __init__(self, seed):
        super().__init__(seed)
        self.marks = []

    def marker(self):
        """an empty stored block without BFINAL; the block start behind it is a mark"""
        self.stored(b"")
        self.marks.append((self.s.bitpos(), len(self.s.hist)))

    def dynamic(self, toks, final=0):
        """a dynamic block over a complete code of all 286 + 30 symbols"""
        self._note()
        rng = self.s.rng
        ll = DS.spread(rng, 286, list(range(286)), 15, .5)
        dl = DS.spread(rng, 30, list(range(30)), 15, .5)
        self.s.dynamic(ll, dl, toks, final)

    def silent(self, k):
        """blocks of k mod 8 bits in all that produce nothing (_index_cases.silent_prefix)"""
        for b in IC.silent_prefix(k):
            self.s.w.bits(int(b), 1)


def lits(rng, n):
    return [("L", rng.randrange(256)) for _ in range(n)]


def filler(rng, n, lead=400):
    """tokens of exactly n bytes none of which reaches in front of their own first byte: literals, then matches into them"""
    toks, have = lits(rng, min(lead, n)), min(lead, n)
    while have < n:
        left = n - have
        if left >= 3 and have >= 1:
            ln = min(left, rng.choice((3, 11, 258, 258, 258)))
            if left - ln in (1, 2) and ln > 5:
                ln -= 2
            toks.append(("M", ln, rng.randint(1, min(have, 32768))))
            have += ln
        else:
            toks.append(("L", rng.randrange(256)))
            have += 1
    return toks


def _planted(name, build, spacing=1, edge=None, containers=(0,)):
    """build(Plant) writes the blocks; the stream goes into every container asked for"""
    r = Plant(zlib.crc32(name.encode()))
    build(r)
    raw, full = r.done()
    for container in containers:
        hb = 8 * IC.HEADER_BYTES[container]
        c = add("P_%s_c%d" % (name, container), container, IC.wrap(raw, full, container), full, spacing,
                [(b + hb, p) for b, p in r.marks])
        if edge:
            kept = set(kept_marks(c.marks, spacing))
            for k, which in edge:  # the k-th mark is the one the edge is about
                assert k in kept
                OUTCOMES.setdefault(which, set()).add(c.marks[k] in c.points)
    return CASES[-1]


def _family_p():
    # ---- distance 0 and 1 in front of a mark: a mark at c, k literals, a match of distance k (touches c) / k + 1
    for k in (1, 2, 258):
        for over in (0, 1):
            def build(r, k=k, over=over):
                r.history(600)
                r.marker()
                rng = r.s.rng
                r.fixed(lits(rng, k) + [("M", 7, k + over)] + lits(rng, 20), 1)
            c = _planted("near_k%d_%s" % (k, "in_front" if over else "touches"), build, edge=[(0, "near_k%d" % k)],
                         containers=(0, 1, 2) if k == 2 else (0,))
            assert (c.marks[0] in c.points) == (not over)

    # ---- the 32 KiB edge: a match at c + 32767 with distance 32768 reaches c - 1, at c + 32768 it reaches c
    for path in ("dynamic", "fixed"):
        for at in (32767, 32768):
            def build(r, path=path, at=at):
                rng = r.s.rng
                r.history(40000)
                r.marker()
                toks = filler(rng, at) + [("M", 100, 32768)] + filler(rng, 3000, lead=2000)
                if path == "dynamic":  # thousands of tokens on either side: the match lies in a fast round
                    r.dynamic(toks)
                else:
                    r.fixed(toks)
                r.fixed(lits(rng, 50), 1)
            c = _planted("far_%s_%d" % (path, at), build, edge=[(0, "far_" + path)])
            assert (c.marks[0] in c.points) == (at == 32768)
    # ... and one byte further on in a later block, behind a block that fills the 32 KiB exactly
    def build(r):
        rng = r.s.rng
        r.history(33000)
        r.marker()
        r.dynamic(filler(rng, 32768))
        r.dynamic(filler(rng, 500) + [("M", 3, 32768)] + filler(rng, 500), 1)
    c = _planted("far_next_block", build)
    assert c.marks[0] in c.points

    # ---- two kept marks 100 bytes apart and a later match
    for what, reach in (("between", 50), ("in_front_of_both", -1), ("exactly_second", 100)):
        def build(r, reach=reach):
            rng = r.s.rng
            r.history(1000)
            r.marker()
            r.fixed(lits(rng, 100))
            r.marker()
            r.fixed(lits(rng, 30) + [("M", 9, 130 - reach)] + lits(rng, 5), 1)  # at c1 + 130, to c1 + reach
        c = _planted("two_marks_" + what, build, edge=[(0, "two_first"), (1, "two_second")])
        assert [m in c.points for m in c.marks] == {"between": [True, False], "in_front_of_both": [False, False],
                                                    "exactly_second": [True, True]}[what]

    # ---- marks the rule does not keep: spacing 4096, a mark every 100 bytes, kept at 4100 and 8200
    for what, reach in (("past_unkept_only", 8250), ("past_the_kept_one", 8199), ("exactly_the_kept_one", 8200)):
        def build(r, reach=reach):
            rng = r.s.rng
            for _ in range(84):
                r.fixed(lits(rng, 100))
                r.marker()
            r.fixed(lits(rng, 50) + [("M", 30, 8450 - reach)] + lits(rng, 70), 1)
        c = _planted("unkept_" + what, build, spacing=4096, edge=[(81, "unkept")])
        assert [c.marks[k][1] for k in kept_marks(c.marks, 4096)] == [4100, 8200]
        assert [p for _, p in c.points] == ([0, 4100, 8200] if reach >= 8200 else [0, 4100])

    # ---- shapes of the marker itself
    def build(r):  # two markers in a row at one position: the first block start behind a marker is the mark that is kept
        rng = r.s.rng
        r.history(500)
        r.marker()
        r.marker()
        r.fixed(lits(rng, 40))
        r.marker()
        r.marker()
        r.marker()
        r.fixed(lits(rng, 40), 1)
    c = _planted("two_markers_in_a_row", build, containers=(0, 1))
    assert [p for _, p in c.marks] == [500, 500, 540, 540, 540] and c.points[1:] == [c.marks[0], c.marks[2]]

    for k in range(8):  # the marker's own header begins at every bit residue
        def build(r, k=k):
            rng = r.s.rng
            r.fixed(lits(rng, 300))
            r.silent((k - r.s.bitpos()) % 8)
            assert r.s.bitpos() % 8 == k
            r.marker()
            r.fixed(lits(rng, 10) + [("M", 5, 10)] + lits(rng, 30))
            r.silent((k + 3 - r.s.bitpos()) % 8)
            r.marker()
            r.fixed(lits(rng, 10) + [("M", 5, 11)], 1)
        c = _planted("marker_at_residue_%d" % k, build, containers=(k % 3,))
        assert [m in c.points for m in c.marks] == [True, False]

    def build(r):  # a stored block that is not empty is no marker
        rng = r.s.rng
        r.history(400)
        r.stored(b"x")
        r.fixed(lits(rng, 40))
        r.stored(bytes(rng.randrange(256) for _ in range(300)))
        r.fixed(lits(rng, 40), 1)
    c = _planted("stored_not_empty", build)
    assert c.marks == [] and len(c.points) == 1

    def build(r):  # a final empty stored block: no block start follows it
        r.history(400)
        r.stored(b"", 1)
    c = _planted("final_empty_stored", build, containers=(0, 2))
    assert c.marks == [] and len(c.points) == 1

    for tail in ("fixed", "stored"):  # a mark at out_pos == size
        def build(r, tail=tail):
            r.history(700)
            r.marker()
            if tail == "fixed":
                r.fixed([], 1)
            else:
                r.stored(b"", 1)
        c = _planted("mark_at_size_" + tail, build, containers=(0, 1))
        assert c.points[1:] == [c.marks[0]] and c.marks[0][1] == len(c.full) == 700

    def build(r):  # markers alone: an empty stream with marks at position 0, none kept
        r.marker()
        r.marker()
        r.stored(b"", 1)
    c = _planted("markers_of_an_empty_stream", build, containers=(0, 1, 2))
    assert len(c.marks) == 2 and len(c.points) == 1


# ---- Family Z --------------------------------------------------------------------------------------------------------------
FLUSHES = (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_BLOCK)


def zlib_flushed(data, cuts, modes, level, container):
    """data compressed with a flush of modes[i] at cuts[i] -> (stream, marks): a sync or full flush leaves a mark at 8 * the
    bytes written so far"""
    co = zlib.compressobj(level, zlib.DEFLATED, WBITS[container])
    out, marks, at = bytearray(), [], 0
    for cut, mode in zip(cuts, modes):
        out += co.compress(data[at:cut])
        out += co.flush(mode)
        at = cut
        if mode != zlib.Z_BLOCK:
            assert out[-4:] == b"\x00\x00\xff\xff"
            marks.append((8 * len(out), at))
    out += co.compress(data[at:])
    out += co.flush()
    return bytes(out), marks


def _family_z():
    for container in (0, 1, 2):
        for level in (1, 6):
            rng = random.Random(7000 + 10 * container + level)
            lens = [rng.choice((1, 200, 3000, 9000, 16000)) for _ in range(40)]
            data = TEXT[977 * container:977 * container + sum(lens)]
            cuts, at = [], 0
            for n in lens[:-1]:
                at += n
                cuts.append(at)
            modes = [rng.choice(FLUSHES) for _ in cuts]
            stream, marks = zlib_flushed(data, cuts, modes, level, container)
            for spacing in (1, 4096, 20000):
                add("Z_c%d_l%d_s%d" % (container, level, spacing), container, stream, data, spacing, marks)


# ---- a stream long enough for the size probe's rule to cut it in two ----------------------------------------------------------
def span_case():
    """150000 text bytes as one gzip stream at level 6, a little over 32 KiB compressed: Z_SYNC_FLUSH every 2000 bytes and one
    Z_FULL_FLUSH in each half, spacing 1 -- wherever the cut lands, a mark that is not fresh lies within 32 KiB in front of it"""
    data = TEXT[:150000]
    cuts = list(range(2000, 150000, 2000))
    modes = [zlib.Z_FULL_FLUSH if c in (40000, 110000) else zlib.Z_SYNC_FLUSH for c in cuts]
    stream, marks = zlib_flushed(data, cuts, modes, 6, 1)
    return Case("Z_spans", 1, stream, data, 1, marks, expected_points(1, stream, data, 1, marks))


_family_p()
_family_z()
NAMES = [c.name for c in CASES]
assert len(set(NAMES)) == len(NAMES)
BY_NAME = {c.name: c for c in CASES}
