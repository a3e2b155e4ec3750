"""k_lz_emit and k_encode_wave at the edges of their rounds and groups, byte for byte against the oracle (raw container).

The chunk path (levels 4, 6, 9; level 9 reaches both kernels through k_lz_walk): inputs that end on and around a wave's
span (512 positions) and a part (8192), chunks of more than 32768 tokens -- token 32768 falls inside a part and inside
a round, both histograms are used, the block is cut -- a chunk of one repeated byte, anchors that carry many literals
beside anchors that carry one, and a skipped first chunk.

The wave packer through flate_hip_debug_write_blocks (encoder 1, plain and paired): token counts around its groups of
128 tokens (two a lane) with the end-of-block code riding in the last group or in a group of its own, the widest items
two to a lane and groups of more than 4096 bits.  A block behind a neighbour at every bit offset of their shared dword
cannot be made through that seam (its slots start on bytes and share no dword): it is made through the chunk path, where
a chunk's second block starts where its first one ends, in a batch of 4096 chunks, which is what it takes for the chunk
path to run the wave packer.
"""
import functools

import numpy as np
import pytest

import _block_synth as S
import _oracle as O
from gpu_util import engine

pytestmark = pytest.mark.gpu

LEVELS = (4, 6, 9)
TEXT_SIZES = (1, 3, 4, 511, 512, 513, 8191, 8192, 8193, 16385, 65535)


# ---------------------------------------------------------------- inputs
@functools.lru_cache(None)
def de_bruijn16():
    """The 65536 letters of a de Bruijn sequence B(16, 4) (Fredricksen-Kessler-Maiorana: the Lyndon words whose length
    divides 4, in order), as the bytes 'a'..'p': read cyclically every 4-gram occurs once, so a stretch of it holds no
    match of the minimum length 4 and every token is a literal."""
    k, n = 16, 4
    a = [0] * (n + 1)
    seq = []
    i = 1
    while True:  # (iterative FKM: the next necklace prefix, kept when its period divides n)
        if n % i == 0:
            seq.extend(a[1:i + 1])
        for j in range(1, n - i + 1):
            a[i + j] = a[j]
        i = n
        while i > 0 and a[i] == k - 1:
            i -= 1
        if i == 0:
            break
        a[i] += 1
    out = np.array(seq, np.uint8) + ord("a")
    assert out.size == k ** n
    return out


def _ladder():
    """Matches that grow by one byte at each of 100 consecutive positions: behind a dictionary of the stretches
    B[k .. 2k + 4) of 256 distinct bytes B, the copy of B finds a match of 4 + k bytes at its position k, each longer than
    the one pending, so a lazy matcher turns one literal after the other before the match goes out -- an anchor with as
    many literals as the level's `lazy` allows (level 9: about a hundred, fewer than the 128 a descriptor can count)."""
    B = bytes((i * 37 + 11) & 0xFF for i in range(256))
    assert len(set(B)) == 256
    parts = []
    for k in range(100):
        seg = B[k:2 * k + 4]
        sep = bytes([B[2 * k + 4] ^ 0x80])  # (ends the stretch: not the byte B goes on with)
        parts.append(seg + sep)
    return b"".join(parts) + B


@functools.lru_cache(None)
def chunk_inputs():
    from flate_amd import synth
    rng = np.random.default_rng(1951)
    text = synth.text(synth.SEED_TEXT, 65535).tobytes()
    inputs = {"empty-first": b""}  # (the batch's first chunk is marked `skip`)
    for n in TEXT_SIZES:
        inputs["text-%d" % n] = text[:n]
    inputs["random-65535"] = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
    inputs["de-bruijn-65535"] = de_bruijn16()[:65535].tobytes()
    inputs["one-byte-65535"] = b"\xa5" * 65535  # (about 254 anchors, each a match of 258)
    inputs["run-then-text"] = b"a" * 300 + text[:65235]
    inputs["ladder-then-text"] = _ladder() + text[:20000]
    return inputs


_ref = {}


def ref(name, data, level, repair=False):
    """The oracle's stream, computed once and shared by the tests."""
    key = (name, level, repair)
    if key not in _ref:
        _ref[key] = O.compress(data, O.RAW, level, repair_q1=repair)
    return _ref[key]


# ---------------------------------------------------------------- the chunk path
@pytest.mark.parametrize("level", LEVELS)
def test_chunk_edges_match_the_oracle(level):
    eng = engine()
    inputs = chunk_inputs()
    names, datas = list(inputs), list(inputs.values())
    assert len(datas) <= 36
    # more than 32768 tokens: the chunk's second histogram and plan slot are used
    for nm in ("random-65535", "de-bruijn-65535"):
        assert O.tokenize(inputs[nm], level).size > S.MAX_TOKENS, nm
    outs, st = eng.compress_many(datas, O.RAW, level)
    for nm, d, got, s in zip(names, datas, outs, st):
        # 102: the reference's own stream does not inflate to the input (its quirk at a full token block); the bytes are
        # the reference's all the same
        assert s in ((0, 102) if O.tokenize(d, level).size >= S.MAX_TOKENS else (0,)), (nm, level, s)
        assert got == ref(nm, d, level), (nm, level)


@pytest.mark.parametrize("level", LEVELS)
def test_full_token_blocks_with_the_q1_repair(level):
    """FLATE_HIP_DEFLATE_REPAIR_Q1: the cut block is handed the bytes its tokens cover (e1, not v1, of k_lz_emit)."""
    from flate_amd import _capi
    eng = engine()
    inputs = chunk_inputs()
    names = ["random-65535", "de-bruijn-65535", "text-65535", "run-then-text"]
    datas = [inputs[n] for n in names]
    eng.set_flags(_capi.DEFLATE_REPAIR_Q1)
    try:
        outs, st = eng.compress_many(datas, O.RAW, level)
    finally:
        eng.set_flags(0)
    assert st == [0] * len(datas)
    for nm, d, got in zip(names, datas, outs):
        assert got == ref(nm, d, level, repair=True), (nm, level)


# ---------------------------------------------------------------- a second block at every bit offset behind the first
def _second_block_bit(data, level):
    """The bit of the stream at which the chunk's second block starts, from the oracle alone: the one offset at which
    the oracle's two blocks, written one by one from the oracle's tokens, overlay to the oracle's stream.  None when the
    stream is not those two blocks (a stored block, the reference's quirk at the seam)."""
    toks = O.tokenize(data, level)
    if toks.size <= S.MAX_TOKENS or toks.size > 2 * S.MAX_TOKENS:
        return None
    stream = int.from_bytes(O.compress(data, O.RAW, level), "little")
    b1 = O.block_write("wb", toks[:S.MAX_TOKENS], 0, None)
    b2 = int.from_bytes(O.block_write("wb", toks[S.MAX_TOKENS:], 1, None), "little")
    v1 = int.from_bytes(b1, "little")
    found = [bit for bit in range(8 * len(b1) - 7, 8 * len(b1) + 1) if v1 | (b2 << bit) == stream and v1 >> bit == 0]
    return found[0] if len(found) == 1 else None


@functools.lru_cache(None)
def _seam_inputs():
    """Chunks of literals only, a few dozen, whose second blocks start at all 32 bit offsets of a dword: rotations of
    the de Bruijn sequence behind r distinct rare bytes, which move the first block's end about."""
    seq = de_bruijn16()
    picked = {}
    for r in range(200):
        if len(picked) == 32:
            break
        rare = bytes(128 + (i * 5 + r) % 128 for i in range(r % 23))
        data = rare + np.roll(seq, -997 * r)[:65535 - len(rare)].tobytes()
        bit = _second_block_bit(data, 6)
        if bit is not None and bit % 32 not in picked:
            picked[bit % 32] = data
    return picked


WAVE_PACKER_MIN_CHUNKS = 4096  # (enqueue_back_end: k_encode_wave from 8192 plan slots up, two slots a chunk; k_encode<true> below)


@pytest.mark.parametrize("packer", ["k_encode", "k_encode_wave"])
def test_second_block_starts_at_every_bit_offset(packer):
    """The chunk's slots are dword-aligned, so the offset of the second block's first bit in the stream is its offset in
    the dword it shares with the first block's last bits: both blocks OR into that dword (a plain store of either
    loses the other's bits).  The 32 chunks alone are a batch of 64 plan slots, which the workgroup packer writes;
    among one-byte chunks that fill the batch up to 4096 chunks they are written by the wave packer."""
    eng = engine()
    picked = _seam_inputs()
    assert sorted(picked) == list(range(32)), sorted(picked)
    datas = [picked[b] for b in range(32)]
    want = [O.compress(d, O.RAW, 6) for d in datas]
    if packer == "k_encode":
        batch, at = datas, list(range(32))
    else:
        n = WAVE_PACKER_MIN_CHUNKS
        batch = [b"x"] * n
        at = [(i * n) // 32 + i % 3 for i in range(32)]  # (spread over the batch, in first and second halves of the slot order)
        for i, d in zip(at, datas):
            batch[i] = d
        assert len(batch) == n and 2 * n >= 8192
    outs, st = eng.compress_many(batch, O.RAW, 6)
    for b, i in enumerate(at):
        assert st[i] in (0, 102), (b, st[i])
        assert outs[i] == want[b], b
    if packer == "k_encode_wave":
        filler = O.compress(b"x", O.RAW, 6)
        assert all(o == filler for i, o in enumerate(outs) if i not in set(at))


# ---------------------------------------------------------------- the wave packer's groups
GROUP_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 32768)


def _widest_tokens(k):
    """k literals, then 256 matches of length 258 at distance 32768 in a block whose other tokens are eight kinds of match
    in counts that grow like Fibonacci numbers (the slowest growth at which Huffman's tree is still a chain, as
    _block_synth.wide_head): length code 285 and distance code 29 sit at the chain's end, 13 extra bits behind them."""
    _, _, _, _, lbase, dbase = S.tabs()
    u0 = 256 + 2
    head, below, acc = [], u0, 2 * u0
    while acc + below + 1 <= S.MAX_TOKENS - 256 - 64:
        c = below + 1
        head.append(c)
        below, acc = acc, acc + c
    dom = [O.tok_match(dbase[i], lbase[257 + i]) for i, c in enumerate(head) for _ in range(c)]
    dom = [dom[i] for i in S._stride_order(len(dom), 7919)]
    run = [O.tok_match(32768, 258)] * 256
    return np.array([O.tok_lit(0x41)] * k + dom[:100] + run + dom[100:], np.uint32)


def _write(eng, blocks, paired, fn):
    at, starts = 0, []
    for i, (tok, inp, _) in enumerate(blocks):
        at = (at + 3) // 4 * 4 + (i * 7 + 1) % 4
        starts.append(at)
        at += eng.debug_block_bound(len(tok), 0 if inp is None else len(inp))
    return eng.debug_write_blocks(blocks, encoder=1, paired=paired, dynamic_only=fn == "dyn", slot_starts=starts)


@pytest.mark.parametrize("paired", [False, True], ids=["plain", "paired"])
def test_token_counts_around_the_groups(paired):
    """The end-of-block code rides in the last group (a slot is free) or goes in a group of its own (counts that are a
    multiple of 128, and no token at all)."""
    eng = engine()
    blocks, names = [], []
    for n in GROUP_COUNTS:
        for mixed in (False, True):
            if mixed and n < 63:
                continue
            toks = np.array(S.count_tokens(n, mixed), np.uint32)
            for eof in (0, 1):
                blocks.append((toks, None, eof))
                names.append((n, mixed, eof))
    if not paired and len(blocks) % 2 == 0:
        blocks.append(blocks[0])  # (an odd count: the other index order of the kernel's callers)
        names.append(names[0])
    assert len(blocks) < 64
    for fn in ("wb", "dyn"):
        got = _write(eng, blocks, paired, fn)
        for nm, (toks, inp, eof), g in zip(names, blocks, got):
            assert g == O.block_write(fn, toks, eof, inp), (nm, fn)


@pytest.mark.parametrize("paired", [False, True], ids=["plain", "paired"])
def test_widest_items_two_to_a_lane(paired):
    """256 items of code 285 / code 29 with the longest codes a block of 32768 tokens gives 256 of a kind, two to a lane,
    starting at an even and at an odd slot, in and across groups."""
    eng = engine()
    cases = [_widest_tokens(k) for k in (0, 1, 27)]
    # ... and _block_synth's run of 128 items of 34 bits and more, as one whole group (it starts at token 256) and across
    # two: more than 4096 bits a group, the third round of the write-out and of the clearing
    wide = [next(c for c in S.token_cases() if c.name == "wide-tokens").tokens, S.wide_phase_cases()[1].tokens]
    for toks in wide:
        w = S.item_widths(toks)
        g = np.concatenate([w, np.zeros(-w.size % 128, np.int64)]).reshape(-1, 128).sum(1)
        assert int(g.max()) > 4096, int(g.max())
    for k, toks in zip((0, 1, 27), cases):
        w = S.item_widths(toks)
        at = k + 100
        # the chain of eight dominant symbols puts distance code 29 at depth 8 and length code 285, which shares the
        # chain's end with the end-of-block code, at depth 9: 9 + 8 + 13 extra bits
        assert (w[at:at + 256] >= 30).all(), (k, int(w[at:at + 256].min()))
        g = np.concatenate([w, np.zeros(-w.size % 128, np.int64)]).reshape(-1, 128).sum(1)
        assert int(g.max()) > 2048, (k, int(g.max()))  # (more than 64 dwords a group: the write-out's second round)
    blocks = [(t, None, eof) for t in cases + wide for eof in (0, 1)]
    if not paired:
        blocks.append(blocks[0])
    for fn in ("wb", "dyn"):
        got = _write(eng, blocks, paired, fn)
        for i, ((toks, inp, eof), g) in enumerate(zip(blocks, got)):
            assert g == O.block_write(fn, toks, eof, inp), (i, fn)
