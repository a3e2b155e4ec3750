"""Token blocks no tokenizer emits, for the block bit packers (k_plan, k_offsets, k_encode<true>, k_encode_wave,
k_encode<false>): every case drives one branch of the packers to its limit and asserts ON THE CPU, from the oracle's
Huffman codes and the length / distance tables, that it still does -- a case that stops exercising its edge fails in
the CPU tier instead of passing silently.  CPU only, deterministic (no random numbers: orders come from strides).

A case is (name, tokens, input, eof, dyn) and `want`, what tests/test_block_synth_cpu.py must find in it.  Tokens are in
the oracle's encoding (O.tok_lit / O.tok_match).  `input`, when not None, is the byte expansion of the tokens: a stored
block is meaningful and the block inflates to it.  eof / dyn are the variant a case is named for; the tests run every
case with both values of each.

The expected bytes always come from the oracle at test time; nothing here is a fixture.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

import _oracle as O

MAX_TOKENS = 32768


class Case(NamedTuple):
    name: str
    tokens: np.ndarray
    input: Optional[bytes]
    eof: int
    dyn: int
    want: dict


# ---------------------------------------------------------------- tables (from the oracle, not from the code under test)
@functools.lru_cache(None)
def tabs():
    L = O.lib()
    lcode = np.array([L.fo_length_code(v) for v in range(256)], np.int64)      # by length - 3
    lextra = np.array([L.fo_length_extra_bits(c) if c >= 257 else 0 for c in range(286)], np.int64)
    dcode = np.array([L.fo_distance_code(d) for d in range(32768)], np.int64)  # by distance - 1
    dextra = np.array([L.fo_distance_extra_bits(c) for c in range(30)], np.int64)
    lbase = {c: int(np.nonzero(lcode == c)[0][0]) + 3 for c in range(257, 286)}
    dbase = {c: int(np.nonzero(dcode == c)[0][0]) + 1 for c in range(30)}
    return lcode, lextra, dcode, dextra, lbase, dbase


def histogram(tokens):
    """(lit/len frequencies with the end-of-block count, distance frequencies) as BlockWriter.indexTokens builds them."""
    lcode, _, dcode, _, _, _ = tabs()
    t = np.asarray(tokens, np.uint32).astype(np.int64)
    m = ((t >> 23) & 1) == 1
    lit = np.bincount((t[~m] >> 15) & 0xFF, minlength=286)
    lit += np.bincount(lcode[(t[m] >> 15) & 0xFF], minlength=286)
    lit[256] += 1
    dist = np.bincount(dcode[t[m] & 0x7FFF], minlength=30)
    return lit, dist


def dynamic_code_lengths(tokens):
    lit, dist = histogram(tokens)
    if not dist.any():
        dist[0] = 1  # block_writer.zig:476-481
    return O.huffman_generate(lit, 15)[1].astype(np.int64), O.huffman_generate(dist, 15)[1].astype(np.int64)


def item_widths(tokens):
    """Bits of every token's item in a DYNAMIC block: code + extra bits (+ distance code + extra bits)."""
    lcode, lextra, dcode, dextra, _, _ = tabs()
    ll, dl = dynamic_code_lengths(tokens)
    t = np.asarray(tokens, np.uint32).astype(np.int64)
    m = ((t >> 23) & 1) == 1
    w = ll[(t >> 15) & 0xFF]
    lc = lcode[(t[m] >> 15) & 0xFF]
    dc = dcode[t[m] & 0x7FFF]
    w[m] = ll[lc] + lextra[lc] + dl[dc] + dextra[dc]
    return w


def group_bits(widths, phase=0):
    """Bit totals of the aligned groups of 64 items, the first group holding 64 - phase of them."""
    w = np.concatenate([np.zeros(phase, np.int64), np.asarray(widths, np.int64)])
    w = np.concatenate([w, np.zeros(-w.size % 64, np.int64)])
    return w.reshape(-1, 64).sum(1)


def expand(tokens):
    """The bytes the tokens stand for, or None when a distance reaches in front of the block."""
    out = bytearray()
    for t in np.asarray(tokens, np.uint32).tolist():
        if (t >> 23) & 1:
            d, n = (t & 0x7FFF) + 1, ((t >> 15) & 0xFF) + 3
            if d > len(out):
                return None
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                pat = bytes(out[-d:])
                out += (pat * (n // d + 1))[:n]
        else:
            out.append((t >> 15) & 0xFF)
    return bytes(out)


def _arr(tokens):
    return np.array(tokens, dtype=np.uint32)


def _history():
    """33025 bytes (a literal, then 128 x (length 258, distance 1)): every distance is valid behind them."""
    return [O.tok_lit(0x41)] + [O.tok_match(1, 258)] * 128


def _stride_order(n, stride):
    """A fixed permutation of range(n): i -> i * stride mod n, the stride moved on until it shares no divisor with n."""
    while np.gcd(stride, n) != 1:
        stride += 2
    return (np.arange(n, dtype=np.int64) * stride) % n


def _case(name, tokens, with_input=True, eof=0, dyn=0, **want):
    tokens = _arr(tokens)
    assert tokens.size <= MAX_TOKENS, name
    inp = expand(tokens) if with_input else None
    assert not with_input or inp is not None, name
    return Case(name, tokens, inp, eof, dyn, want)


# ---------------------------------------------------------------- wide-tokens
WIDE_RUN = 128         # consecutive match tokens of length codes 281..284 and distance codes 28 / 29
WIDE_RUN_AT = 256      # token index of the run in `wide-tokens`; `wide-tokens@k` has it at 256 + k
WIDE_SLACK = 66        # what the literals in front (at most 64) and the end-of-block count add to the rare tail


def wide_head(budget=MAX_TOKENS - 64 - 1):
    """Counts of the dominant symbols.  The rare tail (the run's codes, the literal, end-of-block) weighs at most
    U0 = WIDE_RUN + WIDE_SLACK.  Every dominant count is one more than the heaviest the subtree below the PREVIOUS dominant
    symbol can be, so Huffman's two lightest nodes are always "everything rarer" and the next dominant symbol: a chain
    (Fibonacci growth: the slowest that still chains), one bit deeper per dominant symbol, whatever 0..64 literals add."""
    u0 = WIDE_RUN + WIDE_SLACK
    head, below, acc = [u0], u0, 2 * u0  # `below`: bound of the subtree under the last symbol's sibling
    while True:
        c = below + 1
        if acc + c - WIDE_SLACK > budget:
            return head
        head.append(c)
        below, acc = acc, acc + c


def wide_tokens(k=0):
    """k literals, the history (129 tokens), dominant matches up to token 256 + k, the run, the remaining dominant
    matches.  Lengths and distances are paired by position only: both alphabets see the same dominant counts."""
    _, lextra, _, dextra, lbase, dbase = tabs()
    head = wide_head()
    # dominant length codes: the lightest is 285 (it holds the history's 128), then 257, 258, ...; distances: the
    # heaviest is code 0 (the history's), then codes 1, 2, ...
    lsyms = [285] + list(range(257, 257 + len(head) - 1))
    lens_pool = [c for c, n in zip(lsyms, head) for _ in range(n)][128:]
    dsyms = list(range(len(head)))
    dist_pool = [c for c, n in zip(dsyms, sorted(head, reverse=True)) for _ in range(n)][128:]
    n = len(lens_pool)
    assert len(dist_pool) == n
    toks = [O.tok_lit(0x41)] * k + _history()
    li, di = _stride_order(n, 7919), _stride_order(n, 104729)  # two fixed shuffles: lengths and distances pair up by chance
    fill = []
    for i in range(n):
        lc, dc = lens_pool[li[i]], dist_pool[di[i]]
        ln = lbase[lc] + (i % (1 << lextra[lc]) if lc != 285 else 0)
        ds = dbase[dc] + (i * 5) % (1 << dextra[dc])
        fill.append(O.tok_match(ds, ln))
    runt = []
    for i in range(WIDE_RUN):
        lc, dc = 281 + i % 4, 28 + (i // 4) % 2
        le = (31, 0, 21, 10, 16, 1)[i % 6]          # all ones, none, alternating bits: a dropped spill shows
        de = (8191, 0, 0x1555, 0x0AAA, 4096, 1)[(i // 2) % 6]
        runt.append(O.tok_match(dbase[dc] + de, lbase[lc] + le))
    cut = WIDE_RUN_AT - 129
    return toks + fill[:cut] + runt + fill[cut:]


WIDE_REACHED = {"item_bits": 42, "group_bits": 2640, "group_bits_any_phase": 2672}


@functools.lru_cache(None)
def _wide_base():
    toks = _arr(wide_tokens(0))
    return toks, expand(toks)


def _wide_case(k):
    """`wide-tokens` (k None) and `wide-tokens@k`.  What the shape reaches, from the oracle's codes
    (test_block_synth_cpu.py asserts these numbers, WIDE_REACHED):
      widest item      42 bits  (structural bound 48 = 15 + 5 + 15 + 13): 11..12-bit length codes, 12-bit distance codes
      widest group   2640 bits  in `wide-tokens` (structural bound 64 x 48 = 3072), up to 2672 among `wide-tokens@k`
    A Huffman-optimal code over at most 32768 tokens cannot give 64 consecutive tokens 15-bit length AND distance codes: a
    symbol used 32 times among 32768 gets about 10 bits from a geometric head (counts x2: 2256 bits a group), up to 14
    at the end of a Fibonacci chain.  A chain without the slack reached 2768 bits for k = 0 and fell to 2480 with 64
    literals in front (the literal's count re-balances the tail); a run of 192 or 256 tokens reaches less (2352, 2272)."""
    name = "wide-tokens" if k is None else "wide-tokens@%d" % k
    base, base_input = _wide_base()
    k = k or 0
    toks = np.concatenate([np.full(k, O.tok_lit(0x41), np.uint32), base])
    w = item_widths(toks)
    at = WIDE_RUN_AT + k
    best = int(group_bits(w).max())
    assert best > 2048 and int(w.max()) >= 34, (name, best, int(w.max()))
    assert (w[at:at + WIDE_RUN] >= 34).all(), name
    return Case(name, toks, b"A" * k + base_input, k & 1, 1,
                {"min_group_bits": 2049, "min_item_bits": 34, "run": (at, WIDE_RUN)})


# ---------------------------------------------------------------- every-code
def every_code_tokens():
    _, _, _, dextra, _, dbase = tabs()
    dists = []
    for c in range(30):
        dists += [dbase[c], dbase[c] + (1 << dextra[c]) - 1]
    dists += [1, 2, 4, 5, 32768]
    dists = list(dict.fromkeys(dists))
    toks = _history()
    for i, ln in enumerate(range(3, 259)):
        toks.append(O.tok_match(dists[i % len(dists)], ln))
        if i % 9 == 0:
            toks.append(O.tok_lit(i & 0xFF))
    toks += [O.tok_match(32768, 3), O.tok_match(1, 258), O.tok_match(32768, 258), O.tok_match(1, 3)]
    return toks


def _every_code_case():
    lcode, _, dcode, _, _, _ = tabs()
    toks = _arr(every_code_tokens())
    m = ((toks >> 23) & 1) == 1
    assert set(((toks[m] >> 15) & 0xFF).tolist()) == set(range(256))
    assert set(dcode[toks[m] & 0x7FFF].tolist()) == set(range(30))
    assert set(lcode[(toks[m] >> 15) & 0xFF].tolist()) == set(range(257, 286))
    return _case("every-code", toks, eof=1, dyn=0)


# ---------------------------------------------------------------- count-N
COUNTS = (0, 1, 62, 63, 64, 65, 127, 128, 129, 4096, 32767, 32768)


def _skewed_literal(i):
    """A byte whose value thins out geometrically: a text-like Huffman tree without a random number."""
    x = (i * 2654435761) & 0xFFFFFFFF
    z = 0
    while x & 1 and z < 40:
        x >>= 1
        z += 1
    return 0x61 + z * 3 + ((x >> 1) & 1)


def count_tokens(n, mixed):
    toks = []
    for i in range(n):
        if mixed and i >= 4 and i % 3 == 0:
            back = len(toks)  # (a lower bound of the bytes so far)
            toks.append(O.tok_match(1 + (i * 37) % min(back, 32768), 3 + (i * 11) % 256))
        else:
            toks.append(O.tok_lit(_skewed_literal(i)))
    return toks


def _count_cases():
    out = []
    for n in COUNTS:
        for mixed in (False, True):
            if mixed and n < 62:
                continue  # (the same tokens as the literal case)
            name = "count-%d%s" % (n, "-mixed" if mixed else "")
            c = _case(name, count_tokens(n, mixed), eof=n & 1, dyn=0, n_tokens=n)
            assert c.tokens.size == n
            out.append(c)
    # the Zig null: a full block whose bytes a window slide took away
    out.append(_case("count-32768-null", count_tokens(32768, True), with_input=False, eof=1, dyn=0, n_tokens=32768))
    return out


# ---------------------------------------------------------------- header-edges
# Blocks whose dynamic header has a given size.  kind "lin": the first n literals with counts 1 + (i * a) % m; kind
# "pow": all 256 literals, the 29 length codes and 30 distance codes with counts 2 ** ((i * a) % m) -- many code
# lengths in no order, the longest headers.  (kind, n, a, m) were found by `python tests/_block_synth.py` (the search at
# the bottom, against the CPU planner); test_block_synth_cpu.py asserts the header's bit count again.
HEADER_RECIPES = {
    # name: (kind, n, a, m, header bits)
    "63-bytes": ("lin", 242, 1, 2, 497),
    "64-bytes": ("lin", 244, 1, 2, 505),
    "65-bytes": ("lin", 250, 1, 2, 515),
    "128-bytes": ("pow", 256, 1, 6, 1022),
    "bits-0": ("lin", 28, 2, 2, 120),
    "bits-1": ("lin", 31, 2, 2, 113),
    "bits-2": ("lin", 24, 1, 2, 138),
    "bits-3": ("lin", 20, 2, 2, 115),
    "bits-4": ("lin", 22, 2, 2, 116),
    "bits-5": ("lin", 20, 1, 2, 125),
    "bits-6": ("lin", 25, 2, 2, 118),
    "bits-7": ("lin", 27, 2, 2, 119),
}


def _shuffled(toks):
    return [toks[i] for i in _stride_order(len(toks), 7919)]


def header_tokens(kind, n, a, m):
    _, _, _, _, lbase, dbase = tabs()
    toks = []
    if kind == "lin":
        for i in range(n):
            toks += [O.tok_lit(i)] * (1 + (i * a) % m)
        return _shuffled(toks)
    for i in range(n):
        toks += [O.tok_lit(i)] * (1 << ((i * a) % m))
    for j in range(29):
        toks += [O.tok_match(dbase[j], lbase[257 + j])] * (1 << (((256 + j) * a) % m))
    toks.append(O.tok_match(dbase[29], 3))
    return _history() + _shuffled(toks)


def _header_cases():
    return [_case("header-edges-" + name, header_tokens(kind, n, a, m), eof=i & 1, dyn=1, hdr_nbits=bits)
            for i, (name, (kind, n, a, m, bits)) in enumerate(HEADER_RECIPES.items())]


# ---------------------------------------------------------------- empty alphabets
def _alphabet_cases():
    one = [O.tok_lit(0x61)] * 100
    nodist = [O.tok_lit(_skewed_literal(i)) for i in range(500)]
    onedist = []
    for i in range(300):
        onedist.append(O.tok_lit(_skewed_literal(i)))
        if i > 40 and i % 2:
            onedist.append(O.tok_match(33 + i % 16, 3 + i % 60))  # distances 33..48: code 10 alone
    _, _, dcode, _, _, _ = tabs()
    t = _arr(onedist)
    m = ((t >> 23) & 1) == 1
    assert len(set(dcode[t[m] & 0x7FFF].tolist())) == 1
    assert not histogram(_arr(nodist))[1].any() and np.count_nonzero(histogram(_arr(one))[0]) == 2
    return [_case("one-symbol", one, eof=1, dyn=1), _case("no-distance", nodist, eof=0, dyn=1),
            _case("one-distance", onedist, eof=1, dyn=0)]


# ---------------------------------------------------------------- type-ties
# Blocks whose candidate sizes (BlockWriter.write's estimates: stored, fixed, dynamic) differ by -1, 0, +1 bits.
# kind "lit": the bytes first .. first + n_sym - 1 with counts f(i) = 1 + (i * a) % m; kind "run": the same and then `r`
# matches (length 3 + j % 5, distance 1).  Found by the search at the bottom; want = (pairing, difference), checked
# against the CPU planner's choice by test_block_synth_cpu.py.
TIE_RECIPES = {
    # name: (kind, first, n_sym, a, m, r, stored bits, fixed bits, dynamic bits)
    "dynamic=fixed": ("lit", 144, 4, 3, 8, 0, 152, 141, 141),
    "dynamic=fixed+1": ("lit", 144, 4, 4, 7, 0, 152, 141, 142),
    "dynamic=fixed+1-run": ("run", 144, 3, 3, 7, 2, 192, 142, 143),
    "dynamic=fixed-1": ("lit", 97, 3, 4, 9, 0, 160, 135, 134),
    "stored=dynamic": ("lit", 144, 33, 0, 1, 0, 304, 312, 304),
    "stored=dynamic+1": ("lit", 144, 18, 1, 2, 0, 256, 258, 255),
    "stored=dynamic-1": ("lit", 144, 32, 0, 1, 0, 296, 303, 297),
    "stored=fixed": ("lit", 144, 17, 1, 2, 0, 240, 240, 244),
    "stored=fixed+1": ("lit", 144, 16, 1, 2, 0, 232, 231, 238),
    "stored=fixed-1": ("lit", 144, 26, 0, 1, 0, 248, 249, 257),
}


def tie_tokens(kind, first, n_sym, a, m, r):
    toks = []
    for i in range(n_sym):
        toks += [O.tok_lit(first + i)] * (1 + (i * a) % m)
    if kind == "run":
        toks += [O.tok_match(1, 3 + j % 5) for j in range(r)]
    return toks


def _tie_cases():
    out = []
    for i, (name, (kind, first, n_sym, a, m, r, sb, fb, db)) in enumerate(TIE_RECIPES.items()):
        toks = tie_tokens(kind, first, n_sym, a, m, r)
        out.append(_case("type-ties-" + name, toks, eof=i & 1, dyn=0, sizes=(sb, fb, db)))
        out.append(_case("type-ties-" + name + "-null", toks, with_input=False, eof=~i & 1, dyn=0, sizes=(None, fb, db)))
    return out


def fixed_and_stored_bits(tokens, in_len):
    """Two of BlockWriter.write's three candidate sizes (block_writer.zig:206-229, 307-334) for a block that can be
    stored: (stored, fixed) in bits.  The third, dynamic, needs the header: the tests take it from the CPU planner."""
    _, lextra, _, dextra, _, _ = tabs()
    lit, dist = histogram(tokens)
    extra = int((lit * lextra).sum() + (dist * dextra).sum())
    flen = np.array([8] * 144 + [9] * 112 + [7] * 24 + [8] * 6)
    fixed = 3 + extra + int((lit * flen).sum()) + 5 * max(int(dist.sum()), 1)  # (a block without matches: one phantom distance)
    return (in_len + 5) * 8, fixed


# ---------------------------------------------------------------- peak-bytes (huffman-only inputs, plain bytes)
PEAK_LEN = 65535
PEAK_LEVELS = 7        # dominant bytes with counts 32768, 16384, ... 512; the other 249 byte values share 511
PEAK_RUN_STARTS = (0, 1, 2, 3, 4093, 16646, 33291, 49936, 65535 - 511)


def peak_bytes(run_start):
    """65535 bytes whose 511 rare ones are contiguous at run_start.  Returns (bytes, (start, length) of the longest
    stretch of 15-bit codes)."""
    counts = [32768 >> i for i in range(PEAK_LEVELS)]
    rest = PEAK_LEN - sum(counts)
    nr = 256 - PEAK_LEVELS
    rare = [rest // nr + (1 if i < rest % nr else 0) for i in range(nr)]
    freq = np.zeros(286, np.int64)
    freq[:PEAK_LEVELS] = counts
    freq[PEAK_LEVELS:256] = rare
    freq[256] = 1
    ln = O.huffman_generate(freq, 15)[1].astype(np.int64)
    rare_bytes = [PEAK_LEVELS + i for i in range(nr) for _ in range(rare[i])]
    # the 15-bit ones first, in a fixed shuffle; the few shorter ones behind them
    wide = [b for b in rare_bytes if ln[b] == 15]
    short = [b for b in rare_bytes if ln[b] != 15]
    k = len(wide)
    wide = [wide[(i * 211) % k] for i in range(k)] if np.gcd(211, k) == 1 else wide
    dom = np.concatenate([np.full(c, i, np.uint8) for i, c in enumerate(counts)])
    n = dom.size
    stride = 104729
    while np.gcd(stride, n) != 1:
        stride += 2
    dom = dom[(np.arange(n, dtype=np.int64) * stride) % n]
    data = np.concatenate([dom[:run_start], np.array(wide + short, np.uint8), dom[run_start:]])
    assert data.size == PEAK_LEN
    assert (np.bincount(data, minlength=256) == freq[:256]).all()
    assert k >= 256 and (ln[data[run_start:run_start + k]] == 15).all(), (k, np.bincount(ln[:256]))
    return data.tobytes(), (run_start, k)


@functools.lru_cache(None)
def peak_cases():
    """[(name, bytes, (start, length) of the run of 15-bit bytes)]"""
    return [("peak-bytes@%d" % s,) + peak_bytes(s) for s in PEAK_RUN_STARTS]


# ---------------------------------------------------------------- the lists
@functools.lru_cache(None)
def token_cases():
    """Every named case but the 64 lane phases of wide-tokens."""
    return ([_wide_case(None), _every_code_case()] + _count_cases() + _header_cases() + _alphabet_cases() + _tie_cases())


@functools.lru_cache(None)
def wide_phase_cases():
    return [_wide_case(k) for k in range(64)]


# ---------------------------------------------------------------- the searches behind HEADER_RECIPES and TIE_RECIPES
def _search():
    """Prints recipes: the smallest block of each family that has the wanted header size / size difference, judged by
    the CPU build of the planner (about a minute)."""
    from _planner_shim import dynamic_estimate_bits, load_shim, plan_histogram
    shim = load_shim()

    found = {}

    def keep(key, size, recipe):
        if key not in found or found[key][0] > size:
            found[key] = (size, recipe)

    for kind, ns, ms in (("lin", range(20, 257), range(2, 40)), ("pow", (256,), range(4, 12))):
        for n in ns:
            for a in range(1, 40 if kind == "pow" else 24):
                for m in ms:
                    lit, dist = histogram(_arr(header_tokens(kind, n, a, m))) if kind == "pow" else (np.zeros(286, np.int64), np.zeros(30, np.int64))
                    if kind == "lin":
                        lit[:n] = 1 + (np.arange(n) * a) % m
                    else:
                        lit[256] -= 1
                    if lit.sum() >= MAX_TOKENS:
                        continue
                    bits = plan_histogram(shim, 2, lit, dist).hdr_nbits
                    nbytes = (bits + 7) // 8
                    keep("%d-bytes" % nbytes if nbytes in (63, 64, 65, 128) else "bits-%d" % (bits & 7), int(lit.sum()),
                         (kind, n, a, m, bits))
    for first in (0x61, 0x90):
        for n_sym in range(1, 40):
            for a in range(5):
                for m in range(1, 10) if a else (1,):
                    for kind, r in [("lit", 0)] + [("run", r) for r in range(1, 30)]:
                        toks = _arr(tie_tokens(kind, first, n_sym, a, m, r))
                        if toks.size > 400:
                            continue
                        sb, fb = fixed_and_stored_bits(toks, len(expand(toks)))
                        lit, dist = histogram(toks)
                        lit[256] -= 1
                        db = dynamic_estimate_bits(shim, lit, dist)
                        if abs(db - fb) <= 1:
                            keep("dynamic=fixed%+d" % (db - fb), toks.size, (kind, first, n_sym, a, m, r, sb, fb, db))
                        if fb <= db and abs(sb - fb) <= 1:
                            keep("stored=fixed%+d" % (sb - fb), toks.size, (kind, first, n_sym, a, m, r, sb, fb, db))
                        if db < fb and abs(sb - db) <= 1:
                            keep("stored=dynamic%+d" % (sb - db), toks.size, (kind, first, n_sym, a, m, r, sb, fb, db))
    for key in sorted(found):
        print('    "%s": %r,' % (key, found[key][1]))


if __name__ == "__main__":
    _search()
