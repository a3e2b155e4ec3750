"""A DEFLATE stream synthesizer (test infrastructure): raw deflate streams written from a description -- code lengths, header
layout, tokens -- and returned WITH the bytes they must decode to, which the generator computes itself from its own token list.
Dynamic blocks no encoder emits: literal/length codes of exactly 10 / 11 bits and distance codes of 8 / 9 / 10 (the decoders'
table widths), trees 15 deep and runs of 48-bit tokens, one-code and empty distance trees, every header field at its limits, code
length repeats that cross from the literal into the distance lengths (Q6: SURVEY.md 8a a20), thousands of tiny blocks, the longest
header without repeats, and the illegal variants of all of these.

`CASES`: {name: (stream, expected bytes -- or None when the stream is invalid)}.  `INFO[name]`: {"error": the oracle's error name
for an invalid stream (written here next to the case, asserted by tests/test_oracle_inflate_pins.py), "q6": the reference-strict
mode (flags = 1) refuses it, "census": Counter of what the stream holds, "header_bits": of its last dynamic header}.
`random_streams(seed, n)`: n random valid multi-block streams.  Everything is seeded; no stream depends on run order.

    python tests/_deflate_synth.py --seeds 0..400      # the census of CASES and of that sweep
"""
import collections
import random
import sys

from _inflate_edge_cases import BW, DBASE, DEXT, LBASE, LEXT, fixed_lit, fixed_match

CLORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def complete_lengths(rng, n, maxbits, skew):
    """n >= 2 code lengths of a complete prefix code, none above maxbits.  skew 0: random splits (about balanced);
    skew 1: always split the deepest leaf (a comb as deep as maxbits allows)."""
    assert 2 <= n <= 1 << maxbits
    leaves = [1, 1]
    while len(leaves) < n:
        c = [i for i, l in enumerate(leaves) if l < maxbits]
        i = max(c, key=lambda i: leaves[i]) if rng.random() < skew else rng.choice(c)
        l = leaves.pop(i)
        leaves += [l + 1, l + 1]
    rng.shuffle(leaves)
    return leaves


def kraft(lens, maxbits=15):
    """sum of 2^-len in units of 2^-maxbits: == 1 << maxbits for a complete code"""
    return sum(1 << (maxbits - l) for l in lens if l)


def assign(n, groups):
    """a length vector of n symbols from [(code length, symbols)]"""
    lens = [0] * n
    for l, syms in groups:
        for s in syms:
            assert lens[s] == 0
            lens[s] = l
    return lens


def spread(rng, n, syms, maxbits, skew):
    """a random complete code over `syms` in an alphabet of n"""
    return assign(n, zip(complete_lengths(rng, len(syms), maxbits, skew), [[s] for s in syms]))


def canon(lens):
    """canonical codes (RFC 1951 3.2.2): {symbol: (code with its bits REVERSED, ready for an LSB-first writer, length)}"""
    cnt = collections.Counter(l for l in lens if l)
    code, nxt = 0, {}
    for b in range(1, 16):
        code = (code + cnt.get(b - 1, 0)) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            c = nxt[l] & ((1 << l) - 1)  # (an over-subscribed set overflows: its codes are never read)
            nxt[l] += 1
            out[s] = (int(format(c, "0%db" % l)[::-1], 2), l)
    return out


def cl_symbols(rng, seq, hlit, rle, q6):
    """The code-length symbols [(symbol, extra, extra bits)] that write the hlit + hdist lengths `seq`.  rle: with 16 / 17 / 18;
    q6: a run may go on from the literal into the distance lengths (else the two lists are written apart)."""
    if not rle:
        return [(v, 0, 0) for v in seq]
    if not q6:
        return cl_symbols(rng, seq[:hlit], hlit, True, True) + cl_symbols(rng, seq[hlit:], 0, True, True)
    cls, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3 and rng.random() < .9:
            r = min(run, 138)
            if r >= 11 and rng.random() < .2:
                r = rng.randint(3, 10)
            cls.append((18, r - 11, 7) if r >= 11 else (17, r - 3, 3))
            i += r
        elif v and run >= 4 and rng.random() < .8:
            cls.append((v, 0, 0))
            r = min(run - 1, 6)
            cls.append((16, r - 3, 2))
            i += 1 + r
        else:
            cls.append((v, 0, 0))
            i += 1
    return cls


def crosses(cls, hlit):
    """does a repeat go from the literal into the distance lengths (what the reference's inflater refuses: Q6)"""
    pos = 0
    for s, x, _ in cls:
        adv = {16: x + 3, 17: x + 3, 18: x + 11}.get(s, 1)
        if (s == 16 and pos == hlit) or pos < hlit < pos + adv:
            return True
        pos += adv
    return False


def copy_match(hist, length, dist):
    """the byte-by-byte copy of a match, in slices where source and target do not overlap"""
    while length:
        k = min(length, dist)
        start = len(hist) - dist
        hist += hist[start:start + k]
        length -= k


class Stream:
    """One raw deflate stream under construction: blocks are appended, the expansion is kept in `hist`."""

    def __init__(self, seed=0):
        self.rng = random.Random(seed)
        self.w = BW()
        self.hist = bytearray()
        self.valid = True
        self.q6 = False
        self.census = collections.Counter()
        self.header_bits = 0
        self._last48 = False

    def bitpos(self):
        return len(self.w.b) * 8 + self.w.n

    def done(self):
        return self.w.done(), (bytes(self.hist) if self.valid else None)

    # ---- stored and fixed blocks (the writers of _inflate_edge_cases.py)
    def stored(self, data, final=0):
        self.w.bits(final, 1)
        self.w.bits(0, 2)
        if self.w.n:
            self.w.bits(0, 8 - self.w.n)
        for v in (len(data), len(data) ^ 0xffff):
            self.w.bits(v, 16)
        self.w.b += data
        self.hist += data
        self.census["stored_blocks"] += 1
        self._last48 = False

    def fixed(self, toks, final=0):
        self.w.bits(final, 1)
        self.w.bits(1, 2)
        for t in toks:
            if t[0] == "L":
                fixed_lit(self.w, t[1])
                self.hist.append(t[1])
            else:
                assert 1 <= t[2] <= len(self.hist)
                fixed_match(self.w, t[1], t[2])
                copy_match(self.hist, t[1], t[2])
        fixed_lit(self.w, 256)
        self.census["fixed_blocks"] += 1
        self._last48 = False

    def history(self, n):
        """a fixed block that writes exactly n more bytes: random literals, and matches of every distance so far"""
        rng, toks, have, goal = self.rng, [], len(self.hist), len(self.hist) + n
        while have < goal:
            left = goal - have
            if have >= 8 and left >= 3 and rng.random() < .9:
                ln = min(left, rng.choice((3, 17, 130, 258, 258, 258)))
                toks.append(("M", ln, rng.randint(1, min(have, 32768))))
                have += ln
            else:
                toks.append(("L", rng.randrange(256)))
                have += 1
        self.fixed(toks)

    # ---- dynamic blocks
    def header(self, final, ll, dl, rle=False, q6=True, full_hclen=False, skew=.5, hlit=None, hdist=None, hclen=None,
               cls=None, cll=None, fields=None):
        """The header of a dynamic block with the literal/length lengths ll and the distance lengths dl.  Choices an encoder does
        not make: rle / q6 (cl_symbols), HCLEN trimmed or the full 19, HLIT / HDIST above what the lengths need.  The escape
        hatch for illegal headers: cls (the code-length symbols as they are), cll (the 19 lengths of their code), hclen, and
        fields (the raw HLIT / HDIST / HCLEN field values).  Returns the header's length in bits."""
        rng, w = self.rng, self.w
        start = self.bitpos()
        if hlit is None:
            hlit = max(257, max([i for i, l in enumerate(ll) if l] or [0]) + 1)
        if hdist is None:
            hdist = max(1, max([i for i, l in enumerate(dl) if l] or [0]) + 1)
        seq = (list(ll) + [0] * 288)[:hlit] + (list(dl) + [0] * 32)[:hdist]
        if cls is None:
            cls = cl_symbols(rng, seq, hlit, rle, q6)
        if cll is None:
            used = sorted(set(c[0] for c in cls))
            if len(used) < 2:
                used.append((used[0] + 1) % 16)
            cll = spread(rng, 19, used, 7, skew)
        if hclen is None:
            hclen = 19 if full_hclen else max(4, max([i for i in range(19) if cll[CLORD[i]]] or [0]) + 1)
        f = fields or (hlit - 257, hdist - 1, hclen - 4)
        w.bits(final, 1)
        w.bits(2, 2)
        w.bits(f[0], 5)
        w.bits(f[1], 5)
        w.bits(f[2], 4)
        for i in range(hclen):
            w.bits(cll[CLORD[i]], 3)
        cc = canon(cll)
        for s, x, xb in cls:
            w.bits(*cc[s])
            w.bits(x, xb)
        self.q6 = self.q6 or crosses(cls, hlit)
        have = set(c[0] for c in cls)
        for s in (16, 17, 18):
            self.census["hdr_with_%d" % s if s in have else "hdr_without_%d" % s] += 1
        self.census["dynamic_blocks"] += 1
        self.header_bits = self.bitpos() - start
        return self.header_bits

    def tokens(self, ll, dl, toks, eob=True):
        """("L", byte) | ("M", length, distance[, length symbol]) | ("SYM", l/l symbol[, extra, distance symbol, extra]): symbols
        by number, whatever they mean | ("BITS", value, n): n raw bits.  A match further back than what is written, and SYM /
        BITS, make the stream invalid: its expected output is None."""
        w, lc, dc, c = self.w, canon(ll), canon(dl), self.census
        for t in toks:
            if t[0] == "L":
                w.bits(*lc[t[1]])
                self.hist.append(t[1])
                c["ll_bits_%d" % ll[t[1]]] += 1
                self._last48 = False
            elif t[0] == "M":
                ln, dist = t[1], t[2]
                li = t[3] - 257 if len(t) > 3 else (28 if ln == 258 else max(i for i in range(28) if LBASE[i] <= ln))
                di = max(i for i in range(30) if DBASE[i] <= dist)
                assert 0 <= ln - LBASE[li] < 1 << LEXT[li] and dist - DBASE[di] < 1 << DEXT[di]
                w.bits(*lc[257 + li])
                w.bits(ln - LBASE[li], LEXT[li])
                w.bits(*dc[di])
                w.bits(dist - DBASE[di], DEXT[di])
                if dist > len(self.hist) or not self.valid:
                    self.valid = False
                    continue
                bits = ll[257 + li] + LEXT[li] + dl[di] + DEXT[di]
                c["ll_bits_%d" % ll[257 + li]] += 1
                c["d_bits_%d" % dl[di]] += 1
                c["tok_bits_%d" % bits] += 1
                if bits == 48 and self._last48:
                    c["tok48_pairs"] += 1
                self._last48 = bits == 48
                if dist == len(self.hist):
                    c["dist_eq_written"] += 1
                copy_match(self.hist, ln, dist)
            elif t[0] == "SYM":
                self.valid = False
                w.bits(*lc[t[1]])
                if len(t) > 2:
                    w.bits(t[2], LEXT[t[1] - 257] if 257 <= t[1] <= 285 else 0)
                    w.bits(*dc[t[3]])
                    w.bits(t[4], DEXT[t[3]] if t[3] < 30 else 0)
            else:
                self.valid = False
                w.bits(t[1], t[2])
        if eob:
            w.bits(*lc[256])
            c["ll_bits_%d" % ll[256]] += 1

    def dynamic(self, ll, dl, toks, final=0, **hdr):
        self.header(final, ll, dl, **hdr)
        if not toks:
            self.census["blocks_0_tokens"] += 1
        self.tokens(ll, dl, toks)

    # ---- token choice
    def pick(self, ll, dl, n, lbits=None, dbits=None, p_match=.5):
        """n random tokens of the code (ll, dl) that are valid behind what is written so far.  lbits / dbits: the code lengths a
        token's literal/length / distance code may have -- a set, or a list of sets taken in turn (token i: entry i % len)."""
        rng, have, out, memo = self.rng, len(self.hist), [], {}
        turn = lambda sel, i: None if sel is None else (frozenset(sel[i % len(sel)]) if isinstance(sel, list) else frozenset(sel))
        for i in range(n):
            lb, db = turn(lbits, i), turn(dbits, i)
            if (lb, db) not in memo:
                memo[lb, db] = ([s for s in range(256) if ll[s] and (lb is None or ll[s] in lb)],
                                [s for s in range(257, min(286, len(ll))) if ll[s] and (lb is None or ll[s] in lb)],
                                [d for d in range(min(30, len(dl))) if dl[d] and (db is None or dl[d] in db)])
            lits, lens, dsts = memo[lb, db]
            if have < 24577:
                dsts = [d for d in dsts if DBASE[d] <= have]
            if lens and dsts and (not lits or rng.random() < p_match):
                s, d = rng.choice(lens), rng.choice(dsts)
                ln = LBASE[s - 257] + rng.randrange(1 << LEXT[s - 257])  # (symbol 284 with extra 31 is a length of 258 too)
                out.append(("M", ln, min(have, DBASE[d] + rng.randrange(1 << DEXT[d])), s))
                have += ln
            else:
                assert lits, "no token fits: lbits %r dbits %r with %d bytes written" % (lb, db, have)
                out.append(("L", rng.choice(lits)))
                have += 1
        return out

    def fill_to_8(self, ll, toks, lbits=None):
        """toks and literals behind them (of lbits code bits, if given) that bring the stream's output to a multiple of 8 bytes: an
        output slot of that size is exactly full (the engines round slots up to 8)"""
        lits = [s for s in range(256) if ll[s] and (lbits is None or ll[s] in lbits)]
        n = len(self.hist) + sum(1 if t[0] == "L" else t[1] for t in toks)
        return toks + [("L", self.rng.choice(lits)) for _ in range(-n % 8)]

    def random_code(self, maxbits, skew, nl=None, nlen=None, nd=None):
        """a random complete literal/length code and distance code over random subsets of the symbols"""
        rng = self.rng
        nl = rng.randint(2, 256) if nl is None else nl
        nlen = rng.randint(1, 29) if nlen is None else nlen
        nd = rng.randint(2, 30) if nd is None else nd
        ll = spread(rng, 286, rng.sample(range(256), nl) + [256] + rng.sample(range(257, 286), nlen), maxbits, skew)
        return ll, spread(rng, 30, rng.sample(range(30), nd), maxbits, skew)


# ---------------------------------------------------------------------------------------------------------------------------
# the directed families
# ---------------------------------------------------------------------------------------------------------------------------
CASES, INFO = {}, {}
PAD = [("BITS", 0, 24), ("BITS", 0, 24)]  # behind the place an invalid stream fails at: the decoders' look-ahead finds bits there


def _add(name, s, error=None):
    """error: the oracle's name for an invalid stream.  Its verdict is ASSERTED against this (test_oracle_inflate_pins)."""
    assert name not in CASES and (s.valid or error), name
    if error:
        s.valid = False
        s.census["error_" + error] += 1
    stream, want = s.done()
    CASES[name] = (stream, want)
    INFO[name] = {"error": error, "q6": s.q6 and error is None, "census": s.census, "header_bits": s.header_bits}


def _cut(name, base, lo, n, errors):
    """`base` cut behind every byte of [lo, lo + n): errors[k] -- or errors[None] -- is the oracle's name for the cut at lo + k"""
    stream = CASES[base][0]
    assert 0 < lo and lo + n < len(stream)
    for k in range(n):
        err = errors.get(k, errors[None])
        CASES["%s_%03d" % (name, k)] = (stream[:lo + k], None)
        INFO["%s_%03d" % (name, k)] = {"error": err, "q6": False, "census": collections.Counter({"error_" + err: 1}), "header_bits": 0}


def _lut_edge_code():
    """literal/length: 1, 2, 3 bits, then 64 codes of 10 and 128 of 11 bits (the end of block among these); distance: 1..7 bits,
    one code each of 8 and 9 bits, two of 10"""
    l10 = list(range(32, 90)) + [257, 258, 270, 280, 284, 285]
    l11 = list(range(90, 209)) + [256, 259, 260, 265, 269, 273, 277, 281, 283]
    ll = assign(286, [(1, [0]), (2, [255]), (3, [10]), (10, l10), (11, l11)])
    dl = assign(30, [(1, [0]), (2, [3]), (3, [5]), (4, [8]), (5, [11]), (6, [14]), (7, [2]), (8, [17]), (9, [20]), (10, [1, 23])])
    assert kraft(ll) == kraft(dl) == 1 << 15
    return ll, dl


def _family_1_lut_edge():
    ll, dl = _lut_edge_code()
    for k, (lb, db, n) in enumerate([
            ([{10}, {11}], [{8}, {9}, {10}], 500),            # table, walk, table, ... on both codes
            ([{11}], [{10}], 400),                             # every token needs the walk (the end of block has 11 bits too)
            ([{10}], [{8}, {9}], 400),                         # the longest codes the 10-bit and the 9- / 8-bit tables hold
            ([{1, 2, 3}, {11}, {10}, {11}, {11}, {1}], [{9}, {10}, {1, 2, 3}, {8}], 800),
            (None, None, 800)]):
        s = Stream(100 + k)
        s.history(4096)
        s.dynamic(ll, dl, s.pick(ll, dl, n, lb, db), rle=k % 2 == 0, q6=False)
        last = s.fill_to_8(ll, s.pick(ll, dl, n // 3, lb, db), lb[0] if lb else None)
        s.dynamic(ll, dl, last, final=1, rle=True, q6=False, full_hclen=True)
        _add("lut_edge_%d" % k, s)
    # the widest token the tables serve: 10 + 5 bits of length (symbol 284), then 9 + 13 (8 + 13) bits of distance (29 / 28)
    wide = assign(30, [(b, [b]) for b in range(1, 8)] + [(8, [28]), (9, [29]), (10, [0, 27])])
    assert kraft(wide) == 1 << 15
    s = Stream(110)
    s.history(32768)
    toks = [t for t in s.pick(ll, wide, 600, {10}, [{9}, {8}], p_match=1.0) if t[3] == 284][:120]
    assert len(toks) >= 40 and ll[284] + LEXT[27] + wide[29] + DEXT[29] == 37
    s.dynamic(ll, wide, s.fill_to_8(ll, toks, {10}), final=1)
    _add("lut_edge_widest_table_token", s)


def _deep15_code():
    """literal/length: a comb of 1..10 bits and 32 codes of 15 bits, 281..285 and the end of block among them; distance: a comb
    of 1..13 bits, and 28, 29, 0 and 27 with 15 bits"""
    ll = assign(286, [(b, [64 + b]) for b in range(1, 11)] + [(15, list(range(97, 123)) + [256, 281, 282, 283, 284, 285])])
    dl = assign(30, [(b, [b]) for b in range(1, 14)] + [(15, [28, 29, 0, 27])])
    assert kraft(ll) == kraft(dl) == 1 << 15
    return ll, dl


def _family_2_deep15():
    ll, dl = _deep15_code()
    tok48 = lambda s, n: [t for t in s.pick(ll, dl, n, {15}, {15}, p_match=1.0) if t[3] <= 284 and t[2] >= 16385]
    s = Stream(200)  # a run of the longest tokens: 15 + 5 + 15 + 13 bits
    s.history(32768)
    toks = tok48(s, 400)[:150]
    assert len(toks) >= 100
    s.dynamic(ll, dl, s.fill_to_8(ll, toks, {15}), final=1)
    _add("deep15_run48", s)
    s = Stream(201)  # the same in pairs, with literals of 15 bits in between
    s.history(32768)
    toks = []
    for t in tok48(s, 120):
        toks += [t] * 2 + [("L", s.rng.randrange(97, 123)) for _ in range(s.rng.randint(1, 3))]
    s.dynamic(ll, dl, toks, rle=True)
    s.dynamic(ll, dl, s.fill_to_8(ll, s.pick(ll, dl, 200)), final=1, rle=True, q6=False)
    _add("deep15_run48_lit15", s)
    s = Stream(202)  # length 258 as symbol 285 and as symbol 284 with extra 31
    s.history(20000)
    s.dynamic(ll, dl, s.fill_to_8(ll, [("M", 258, 16385 + 7 * i, 285 - i % 2) for i in range(60)], {15}), final=1)
    _add("deep15_len258_both_ways", s)
    for written, err in ((32768, None), (32767, "InvalidMatch")):
        s = Stream(203)
        s.history(written)
        s.dynamic(ll, dl, s.fill_to_8(ll, [("M", 258, 32768, 284), ("L", 97), ("M", 200, 32768)], {15}), final=1)
        _add("deep15_dist32768_written%d" % written, s, err)
    s = Stream(204)  # the smallest stream of the kind, for the truncated family: a header, then a few 48-bit tokens
    s.history(16500)
    s.dynamic(ll, dl, s.fill_to_8(ll, [("M", 131 + i, 16385 + 11 * i, 281) for i in range(12)], {15}), final=1)
    _add("deep15_short", s)


def _family_3_degenerate_trees():
    rng = random.Random(300)
    lits = spread(rng, 286, list(range(65, 76)) + [256, 257, 260, 270, 285], 9, .3)
    one = assign(30, [(1, [4])])  # one distance code of one bit: distances 5 and 6
    s = Stream(301)
    s.history(40)
    s.dynamic(lits, one, s.pick(lits, one, 400), final=1)
    _add("degenerate_trees_one_distance_code", s)
    s = Stream(302)  # the other bit where the distance code stands: no code has it
    s.history(40)
    s.header(1, lits, one)
    s.tokens(lits, one, s.pick(lits, one, 20), eob=False)
    s.w.bits(*canon(lits)[257])
    s.tokens(lits, one, [("BITS", 1, 1)] + PAD)
    _add("degenerate_trees_one_distance_code_other_bit", s, "InvalidCode")
    nolen = spread(rng, 286, list(range(65, 76)) + [256], 9, .3)
    s = Stream(303)  # no distance code at all, literals only
    s.dynamic(nolen, [0], s.pick(nolen, [0], 300), final=1)
    _add("degenerate_trees_no_distance_code_literals_only", s)
    s = Stream(304)  # no distance code, and a length symbol in the data
    s.header(1, lits, [0])
    s.tokens(lits, [0], s.pick(lits, [0], 30), eob=False)
    s.w.bits(*canon(lits)[257])
    s.tokens(lits, [0], PAD)
    _add("degenerate_trees_no_distance_code_then_a_length", s, "InvalidCode")
    only256 = assign(286, [(1, [256])])
    s = Stream(305)  # a literal tree that holds only the end of block, in a one-bit code
    for final in (0, 0, 1):
        s.dynamic(only256, [0], [], final=final)
    _add("degenerate_trees_only_end_of_block", s)
    s = Stream(306)  # ... and the bit it does not have
    s.header(1, only256, [0])
    s.tokens(only256, [0], [("BITS", 1, 1)] + PAD, eob=False)
    _add("degenerate_trees_only_end_of_block_other_bit", s, "InvalidCode")
    s = Stream(307)  # only the end of block, in a two-bit code: a single code of more than one bit is incomplete
    s.dynamic(assign(286, [(2, [256])]), [0], [], final=1)
    _add("degenerate_trees_one_code_of_two_bits", s, "IncompleteHuffmanTree")
    s = Stream(308)  # two-symbol trees on both sides
    s.history(10)
    s.dynamic(assign(286, [(1, [0, 256])]), [0], [("L", 0)] * 50)
    two_l, two_d = assign(286, [(1, [256, 285])]), assign(30, [(1, [0, 29])])
    s.dynamic(two_l, two_d, [("M", 258, 1)] * 130)
    s.dynamic(two_l, two_d, [("M", 258, 24577), ("M", 258, 1), ("M", 258, 32768)], final=1)
    _add("degenerate_trees_two_symbols", s)
    ll8 = [8] * 255 + [0, 8]  # 256 codes of 8 bits
    s = Stream(309)  # a code-length alphabet of ONE code of one bit: fine in the other alphabets, incomplete here
    s.header(1, ll8, [0], cls=[(8, 0, 0)] * 258, cll=assign(19, [(1, [8])]))
    s.tokens(ll8, [0], PAD, eob=False)
    _add("degenerate_trees_code_length_alphabet_of_one", s, "IncompleteHuffmanTree")
    s = Stream(310)  # a code-length alphabet without any code: the first symbol read has none
    s.header(1, ll8, [0], cls=[], cll=[0] * 19)
    s.tokens(ll8, [0], PAD, eob=False)
    _add("degenerate_trees_code_length_alphabet_empty", s, "InvalidCode")


def _family_4_header_fields():
    def lits(s, top=257):
        return spread(s.rng, 288, list(range(48, 58)) + [256] + ([top - 1] if top > 257 else []), 7, .4)

    def dists(s, top):
        return spread(s.rng, 32, sorted(set([0, 1, 2, top - 1])), 5, .4) if top > 1 else assign(32, [(1, [0])])

    good_l, good_d = assign(286, [(3, [97, 98, 99, 100, 256, 257, 258, 259])]), [3] * 8
    # HLIT 257 and 286, HDIST 1 and 30, HCLEN trimmed and 19
    for k, (hlit, hdist, full) in enumerate(((257, 1, False), (286, 30, True), (257, 30, False), (286, 1, True))):
        s = Stream(400 + k)
        s.history(25000)
        ll, dl = lits(s, hlit), dists(s, hdist)
        s.dynamic(ll, dl, s.pick(ll, dl, 60), hlit=hlit, hdist=hdist, full_hclen=full, rle=True, q6=False)
        s.dynamic(ll, dl, s.pick(ll, dl, 60), final=1, hlit=hlit, hdist=hdist, full_hclen=full)
        _add("header_fields_hlit%d_hdist%d_hclen%s" % (hlit, hdist, "19" if full else "trimmed"), s)
    # HCLEN 5, the least a valid block can have (16, 17, 18, 0, 8): 256 codes of 8 bits
    ll8 = [8] * 255 + [0, 8]
    s = Stream(410)
    s.header(1, ll8, [0], cls=[(8, 0, 0)] + [(16, 3, 2)] * 42 + [(8, 0, 0)] * 2 + [(0, 0, 0), (8, 0, 0), (0, 0, 0)],
             cll=assign(19, [(1, [8]), (2, [16]), (3, [0]), (4, [17]), (4, [18])]))
    s.tokens(ll8, [0], [("L", b) for b in range(255)])
    _add("header_fields_hclen5", s)
    # HCLEN 4: codes for 16, 17, 18 and 0 only -- every length is 0, so there is no end of block
    s = Stream(411)
    s.header(1, [0] * 257, [0], cls=[(18, 127, 7), (18, 108, 7), (0, 0, 0)], cll=assign(19, [(1, [18]), (2, [0]), (3, [16, 17])]), hclen=4)
    s.tokens(ll8, [0], PAD, eob=False)
    _add("header_fields_hclen4_no_end_of_block", s, "MissingEndOfBlockCode")
    # HLIT / HDIST field values 30 and 31 (287 / 288 literal/length codes, 31 / 32 distance codes)
    for k, (name, hlit, hdist) in enumerate((("hlit_field30", 287, 4), ("hlit_field31", 288, 4), ("hdist_field30", 270, 31),
                                             ("hdist_field31", 270, 32))):
        s = Stream(420 + k)
        ll, dl = lits(s, hlit), dists(s, hdist)
        s.header(1, ll, dl, hlit=hlit, hdist=hdist)
        s.tokens(ll, dl, [("L", 48)] * 5 + PAD)
        _add("header_fields_" + name, s, "InvalidDynamicBlockHeader")
    # length symbols 286 / 287 and distance symbols 30 / 31 given codes and then used: the header that names them is refused
    for k, (name, sym, isdist) in enumerate((("sym286", 286, 0), ("sym287", 287, 0), ("dist30", 30, 1), ("dist31", 31, 1))):
        s = Stream(430 + k)
        s.history(100)
        ll = lits(s, 258) if isdist else lits(s, sym + 1)
        dl = dists(s, sym + 1) if isdist else dists(s, 3)
        s.header(1, ll, dl)
        s.tokens(ll, dl, [("L", 50), ("SYM", 257, 0, sym, 0) if isdist else ("SYM", sym, 0, 0, 0)] + PAD)
        _add("header_fields_%s_coded_and_used" % name, s, "InvalidDynamicBlockHeader")
    seq = good_l[:260] + good_d  # 268 lengths
    plain = lambda part: [(v, 0, 0) for v in part]
    # 16 as the first code-length symbol
    s = Stream(440)
    s.header(1, good_l, good_d, cls=[(16, 0, 2)] + plain(seq[3:]))
    s.tokens(good_l, good_d, PAD, eob=False)
    _add("header_fields_repeat16_first", s, "InvalidDynamicBlockHeader")
    # 16 / 17 / 18 that overrun HLIT + HDIST by one: the longest repeat where one fewer is left
    for sym, x, xb, n in ((16, 3, 2, 6), (17, 7, 3, 10), (18, 127, 7, 138)):
        s = Stream(441 + sym)
        s.header(1, good_l, good_d, cls=plain(seq[:len(seq) - (n - 1)]) + [(sym, x, xb)])
        s.tokens(good_l, good_d, PAD, eob=False)
        _add("header_fields_repeat%d_overruns_by_one" % sym, s, "InvalidDynamicBlockHeader")
    # Q6 crossings by 16, 17 and 18: valid by the RFC, refused by the reference's inflater (flags = 1)
    for sym in (16, 17, 18):
        s = Stream(460 + sym)
        s.history(300)
        if sym == 16:    # lengths 256..259 and all eight distance lengths are 3: six copies from 257 on
            ll, dl, hlit = good_l, good_d, 260
            cls = plain(seq[:257]) + [(16, 3, 2)] + plain(seq[263:])
        else:            # zeros at the end of the literal/length lengths and at the start of the distance lengths
            ll = spread(s.rng, 286, [97, 98, 99, 100, 256, 257, 258, 259], 6, .3)
            z = 3 if sym == 17 else 10
            dl, hlit = [0] * z + [1, 1], 260 + z
            cls = plain(ll[:260]) + [(17, 2 * z - 3, 3) if sym == 17 else (18, 2 * z - 11, 7)] + plain([1, 1])
        s.header(0, ll, dl, hlit=hlit, cls=cls)
        s.tokens(ll, dl, s.pick(ll, dl, 40))
        s.dynamic(ll, dl, s.pick(ll, dl, 40), final=1, hlit=hlit)
        assert s.q6
        _add("header_fields_q6_crossing_by_%d" % sym, s)
    # a 16 that stands exactly at the first distance length (it copies the last literal/length length)
    s = Stream(480)
    s.history(300)
    dl = [3, 3, 3, 3, 2, 2]
    s.header(0, good_l, dl, cls=plain(good_l[:260]) + [(16, 1, 2), (2, 0, 0), (2, 0, 0)])
    s.tokens(good_l, dl, s.pick(good_l, dl, 40))
    s.dynamic(good_l, dl, s.pick(good_l, dl, 10), final=1)
    assert s.q6
    _add("header_fields_q6_16_at_the_first_distance_length", s)
    # lens[256] == 0; over-subscribed and incomplete sets in each of the three alphabets
    for k, (name, ll, dl, err) in enumerate((
            ("no_end_of_block", assign(286, [(3, [97, 98, 99, 100, 101, 257, 258, 259])]), [1, 1], "MissingEndOfBlockCode"),
            ("literal_oversubscribed", assign(286, [(2, [97, 98, 99, 100, 256])]), [1, 1], "OversubscribedHuffmanTree"),
            ("literal_incomplete", assign(286, [(3, [97, 98, 99, 256, 257, 258, 259])]), [1, 1], "IncompleteHuffmanTree"),
            ("distance_oversubscribed", good_l, [1, 1, 1], "OversubscribedHuffmanTree"),
            ("distance_incomplete", good_l, [2, 2, 2], "IncompleteHuffmanTree"),
            ("distance_one_code_of_two_bits", good_l, [0, 2], "IncompleteHuffmanTree"))):
        s = Stream(490 + k)
        s.header(1, ll, dl)
        s.tokens(good_l, [1, 1], [("L", 97)] * 4 + PAD)
        _add("header_fields_" + name, s, err)
    for err, cll in (("OversubscribedHuffmanTree", assign(19, [(1, [0, 3]), (2, [2])])),
                     ("IncompleteHuffmanTree", assign(19, [(1, [0]), (2, [3])]))):
        s = Stream(498)
        s.header(1, good_l, [1, 1], cll=cll, cls=[(0, 0, 0)] * 262)
        s.tokens(good_l, [1, 1], PAD, eob=False)
        _add("header_fields_code_length_%s" % err[:-11].lower(), s, err)
    # block type 3 behind a block
    s = Stream(499)
    s.dynamic(good_l, [1, 1], [("L", 97)] * 3)
    s.tokens(good_l, [1, 1], [("BITS", 1, 1), ("BITS", 3, 2)] + PAD, eob=False)
    _add("header_fields_block_type_3", s, "InvalidBlockType")


def _tiny_blocks(seed, n_blocks, name):
    """n_blocks dynamic blocks of 0..3 tokens, their headers in full and without repeats, with empty stored blocks and fixed
    blocks in between"""
    s = Stream(seed)
    rng = s.rng
    s.history(600)
    codes = []
    for _ in range(24):
        ll, dl = s.random_code(rng.choice((7, 9, 12, 15)), rng.choice((0, .5, .9)), nl=rng.randint(2, 40), nlen=rng.randint(1, 8),
                               nd=rng.randint(2, 8))
        codes.append((ll, dl, rng.random() < .5))
    for b in range(n_blocks):
        ll, dl, full = codes[rng.randrange(len(codes))]
        s.dynamic(ll, dl, s.pick(ll, dl, rng.choice((0, 0, 1, 2, 3))), hlit=286 if full else None, hdist=30 if full else None,
                  full_hclen=full)
        r = rng.random()
        if r < .15:
            s.stored(b"")
        elif r < .3:
            s.fixed([("L", rng.randrange(256))] * rng.randint(0, 2))
        elif r < .33:
            s.stored(bytes(rng.randrange(256) for _ in range(rng.randint(1, 9))))
    ll, dl, _ = codes[0]
    s.dynamic(ll, dl, s.pick(ll, dl, 3), final=1)
    _add(name, s)


def _family_5_tiny_blocks():
    _tiny_blocks(500, 2200, "tiny_blocks_2200")  # more than 128 KiB: the span path by the library's own rule
    assert len(CASES["tiny_blocks_2200"][0]) > 128 * 1024 and INFO["tiny_blocks_2200"]["census"]["dynamic_blocks"] >= 2000
    _tiny_blocks(501, 60, "tiny_blocks_60")      # (small enough for every split point, and for the truncated family)


def _family_6_long_header():
    """All 19 code-length codes have a code: 1, 2 and 3 bits for 16, 17, 18 (never written), 7 bits for each of the lengths
    0..15; no repeats, HLIT 286, HDIST 30: 17 + 19 * 3 + 316 * 7 = 2286 bits, the most a header without repeats can have."""
    cll = assign(19, [(1, [16]), (2, [17]), (3, [18]), (7, list(range(16)))])
    assert kraft(cll, 7) == 1 << 7
    s = Stream(600)
    s.history(33000)
    ll, dl = complete_lengths(s.rng, 286, 15, .7), complete_lengths(s.rng, 30, 15, .7)
    bits = s.header(0, ll, dl, cll=cll)
    s.tokens(ll, dl, s.pick(ll, dl, 300))
    assert s.header(1, ll, dl, cll=cll) == bits == 17 + 57 + 316 * 7
    s.tokens(ll, dl, [])
    _add("long_header_%d_bits" % bits, s)


def _family_8_big_random():
    for k in range(3):
        s = Stream(800 + k)
        while len(s.w.b) < 150 * 1024:
            random_block(s, s.rng.choice((50, 3000, 20000)), 0)
        random_block(s, 100, 1)
        _add("big_random_%d" % k, s)
        assert len(CASES["big_random_%d" % k][0]) > 128 * 1024


def random_block(s, ntok, final):
    """one block of a random stream: mostly dynamic with a random complete code, the header's choices at random"""
    rng = s.rng
    r = rng.random()
    if r < .08:
        s.stored(bytes(rng.randrange(256) for _ in range(rng.choice((0, 1, 30, 700)))), final)
    elif r < .16:
        have, toks = len(s.hist), []
        for _ in range(min(ntok, 200)):
            if have >= 1 and rng.random() < .5:
                toks.append(("M", rng.randint(3, 258), rng.randint(1, min(have, 32768))))
                have += toks[-1][1]
            else:
                toks.append(("L", rng.randrange(256)))
                have += 1
        s.fixed(toks, final)
    else:
        ll, dl = s.random_code(rng.choice((9, 11, 15, 15)), rng.choice((0, .5, .95)))
        s.dynamic(ll, dl, s.pick(ll, dl, ntok), final=final, rle=rng.random() < .7, q6=rng.random() < .5,
                  full_hclen=rng.random() < .2, skew=rng.choice((0, .5, .95)),
                  hlit=286 if rng.random() < .15 else None, hdist=30 if rng.random() < .15 else None)


def random_stream(seed):
    """-> (stream, expected bytes, whether the reference-strict mode refuses it (Q6), census)"""
    s = Stream(seed)
    nb = s.rng.randint(1, 6)
    for b in range(nb):
        random_block(s, s.rng.choice((0, 1, 50, 3000)), int(b == nb - 1))
    stream, want = s.done()
    return stream, want, s.q6, s.census


def random_streams(seed, n, info=None):
    """the random valid multi-block streams of the seeds seed .. seed + n - 1: [(stream, expected bytes)]; `info`, a list, gets
    (q6, census) of each"""
    out = []
    for k in range(n):
        stream, want, q6, census = random_stream(seed + k)
        out.append((stream, want))
        if info is not None:
            info.append((q6, census))
    return out


_family_1_lut_edge()
_family_2_deep15()
_family_3_degenerate_trees()
_family_4_header_fields()
_family_5_tiny_blocks()
_family_6_long_header()
_family_8_big_random()
# 7: cut at every byte of a 64-byte stretch that spans a block header and a few 48-bit tokens / a few tiny blocks
_cut("truncated_deep15", "deep15_short", len(CASES["deep15_short"][0]) - 110, 64, {None: "EndOfStream"})
_cut("truncated_tiny_blocks", "tiny_blocks_60", len(CASES["tiny_blocks_60"][0]) // 2, 64, {None: "EndOfStream"})

VALID = sorted(n for n in CASES if CASES[n][1] is not None)
INVALID = sorted(n for n in CASES if CASES[n][1] is None)
SMALL = sorted(n for n in CASES if len(CASES[n][0]) <= 12000)      # every split point of these is tried (test_gpu_inflater)
LARGE = sorted(n for n in CASES if len(CASES[n][0]) > 128 * 1024)  # the span path by the library's own rule


def census(names=None, seeds=()):
    """what the directed cases (all, or `names`) and the random streams of `seeds` hold, counted from the generator's records"""
    total = collections.Counter()
    for n in CASES if names is None else names:
        total.update(INFO[n]["census"])
    for k in seeds:
        total.update(random_stream(k)[3])
    return total


# the classes the tests rely on (test_oracle_inflate_pins: test_synth_census): none may be empty
CENSUS_CLASSES = (["ll_bits_10", "ll_bits_11", "ll_bits_15", "d_bits_8", "d_bits_9", "d_bits_10", "d_bits_15", "tok_bits_48",
                   "tok48_pairs", "dist_eq_written", "blocks_0_tokens", "stored_blocks", "fixed_blocks"]
                  + ["hdr_%s_%d" % (w, s) for w in ("with", "without") for s in (16, 17, 18)]
                  + ["error_" + e for e in ("EndOfStream", "InvalidCode", "OversubscribedHuffmanTree", "IncompleteHuffmanTree",
                                            "MissingEndOfBlockCode", "InvalidMatch", "InvalidBlockType", "InvalidDynamicBlockHeader")])


if __name__ == "__main__":
    lo, hi = 0, 0
    if "--seeds" in sys.argv:
        lo, hi = (int(x) for x in sys.argv[sys.argv.index("--seeds") + 1].split(".."))
    c = census(seeds=range(lo, hi))
    print("%d directed cases (%d valid, %d invalid), %d compressed bytes; random seeds %d..%d"
          % (len(CASES), len(VALID), len(INVALID), sum(len(v[0]) for v in CASES.values()), lo, hi))
    for k in sorted(c):
        print("%-28s %d" % (k, c[k]))
    for k in CENSUS_CLASSES:
        assert c[k] > 0, k
