"""The synthesized token blocks of _block_synth.py on the CPU: the shared planner (flate_amd/csrc/flate_common.h) plus
the Python model of the bit packers must write the oracle's bytes for every case, the blocks must inflate to their
input, and every case must still exercise the edge it is named for -- measured from the model's item widths and
printed (run with -s to see what was reached).  No GPU."""
import zlib

import numpy as np
import pytest

import _block_synth as S
import _oracle as O
from _planner_shim import dynamic_estimate_bits, encode_block, load_shim


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def _variants(c, full):
    """(fn, input, eof): the whole cross product, or the variant the case is named for with and without its input."""
    fns = ("wb", "dyn") if full else (("dyn",) if c.dyn else ("wb",))
    eofs = (0, 1) if full else (c.eof,)
    inputs = (c.input, None) if c.input is not None else (None,)
    return [(fn, inp, eof) for fn in fns for inp in inputs for eof in eofs]


def _inflates_to(block, plan, eof, want):
    """The block (padded to a byte) as a raw deflate stream: a block that is not final gets an empty fixed final block
    behind its last BIT -- an inflater does not skip the padding."""
    if not eof:
        if plan.type == 0:
            block = block + b"\x03\x00"
        else:
            v = int.from_bytes(block, "little") | (3 << plan.size_bits)
            block = v.to_bytes((plan.size_bits + 10 + 7) // 8, "little")
    return zlib.decompress(block, -15) == want


@pytest.mark.parametrize("which", ["cases", "phases"])
def test_cpu_model_writes_the_oracles_bytes_and_they_inflate(shim, which):
    cases = S.token_cases() if which == "cases" else S.wide_phase_cases()
    n = 0
    for c in cases:
        for fn, inp, eof in _variants(c, which == "cases"):
            want = O.block_write(fn, c.tokens, eof, inp)
            got, plan = encode_block(shim, 0, c.tokens, inp, eof, fn == "dyn")
            assert got == want, (c.name, fn, inp is not None, eof)
            if inp is not None:
                assert _inflates_to(got, plan, eof, inp), (c.name, fn, eof)
            n += 1
    assert n >= len(cases) * 2


def _widths(shim, c):
    w = {}
    _, plan = encode_block(shim, 0, c.tokens, None, c.eof, True, widths=w)
    assert plan.type == 2
    items = np.concatenate([w["hdr"], w["sym"], [w["eob"]]])
    return w, items, plan


def test_wide_cases_reach_two_store_rounds_and_the_third_dword(shim):
    """More than 2048 bits in an aligned group of 64 (the second round of dword stores and of the window's clear) and
    items of 34 bits or more (a third dword at some shift), in both packers' groupings: k_encode_wave groups the tokens
    alone, k_encode the header's bytes, the tokens and the end-of-block code together."""
    reached, spills = [], [0] * 4
    for c in [S.token_cases()[0]] + S.wide_phase_cases():
        w, items, plan = _widths(shim, c)
        assert (w["sym"] == S.item_widths(c.tokens)).all()  # the generator's own widths (oracle codes) are the model's
        tok_groups, item_groups = S.group_bits(w["sym"]), S.group_bits(items)
        at, run = c.want["run"]
        assert int(w["sym"][at:at + run].min()) >= c.want["min_item_bits"], c.name
        assert int(tok_groups.max()) >= c.want["min_group_bits"], c.name
        assert int(item_groups.max()) >= c.want["min_group_bits"], c.name
        # two wide groups one behind the other: what a window that was not cleared spoils
        wide = np.nonzero(tok_groups > 2048)[0]
        assert wide.size >= 2 or c.name != "wide-tokens", c.name
        # the third dword itself: a block starts on a byte of its slot, the slot at any residue mod 4 -- an item of n bits
        # at bit offset o needs it when (o & 31) + n > 64, and a forced-zero `hi` shows when the bits up there are not 0
        off = plan.hdr_nbits + np.cumsum(w["sym"]) - w["sym"]
        for residue in range(4):
            sh = (8 * residue + off[at:at + run]) & 31
            n, v = w["sym"][at:at + run], w["symv"][at:at + run]
            spill = (sh + n > 64) & ((v >> np.maximum(64 - sh, 1).astype(np.uint64)) != 0)
            assert spill.any(), (c.name, residue)
            spills[residue] += int(spill.sum())
        reached.append((c.name, int(w["sym"].max()), int(tok_groups.max()), int(item_groups.max()), plan.hdr_nbits))
    for r in reached:
        print("%-16s widest item %d bits, widest token group %d bits, widest item group %d bits, header %d bits" % r)
    print("run items with set bits in a third dword, by slot residue mod 4:", spills)
    assert reached[0][1] == S.WIDE_REACHED["item_bits"] and reached[0][2] == S.WIDE_REACHED["group_bits"]
    assert max(r[2] for r in reached) == S.WIDE_REACHED["group_bits_any_phase"]
    # the run meets every lane phase, and starts at several bit offsets inside a dword
    assert {c.want["run"][0] % 64 for c in S.wide_phase_cases()} == set(range(64))
    starts = set()
    for c in S.wide_phase_cases():
        w, items, plan = _widths(shim, c)
        starts.add((plan.hdr_nbits + int(w["sym"][:c.want["run"][0]].sum())) & 31)
    print("bit offsets (mod 32) at which the run starts:", sorted(starts))
    assert len(starts) >= 8


def test_count_and_alphabet_cases_are_what_they_are_named(shim):
    by_name = {c.name: c for c in S.token_cases()}
    for n in S.COUNTS:
        assert by_name["count-%d" % n].tokens.size == n
        if n >= 62:
            t = by_name["count-%d-mixed" % n].tokens
            assert t.size == n and ((t >> 23) & 1).any() and not ((t >> 23) & 1).all()
    assert by_name["count-32768-null"].input is None and by_name["count-32768-null"].tokens.size == 32768
    assert by_name["count-0"].input == b""
    # the literal-only counts are stored-capable: the planner has all three block types to choose from
    assert len(by_name["count-32768"].input) == 32768


def test_header_edges_have_the_header_sizes_they_are_named_for(shim):
    seen_bytes, seen_bits = set(), set()
    for c in S.token_cases():
        if not c.name.startswith("header-edges-"):
            continue
        _, _, plan = _widths(shim, c)
        print("%-26s header %4d bits = %3d bytes, %d in the last" % (c.name, plan.hdr_nbits, (plan.hdr_nbits + 7) // 8, plan.hdr_nbits & 7))
        assert plan.hdr_nbits == c.want["hdr_nbits"], c.name
        seen_bytes.add((plan.hdr_nbits + 7) // 8)
        seen_bits.add(plan.hdr_nbits & 7)
    assert {63, 64, 65, 128} <= seen_bytes and seen_bits == set(range(8))


def test_type_ties_differ_by_what_they_are_named_for(shim):
    """The three candidate sizes of BlockWriter.write, and the planner's choice among them: ties go to fixed over
    dynamic and to Huffman over stored (block_writer.zig:362, 369)."""
    diffs = set()
    for c in S.token_cases():
        if not c.name.startswith("type-ties-") or c.input is None:
            continue
        sb, fb, db = c.want["sizes"]
        stored, fixed = S.fixed_and_stored_bits(c.tokens, len(c.input))
        lit, dist = S.histogram(c.tokens)
        lit[256] -= 1
        dynamic = dynamic_estimate_bits(shim, lit, dist)
        assert (stored, fixed, dynamic) == (sb, fb, db), c.name
        want_type = 1 if fixed <= dynamic else 2
        if stored < min(fixed, dynamic):
            want_type = 0
        _, plan = encode_block(shim, 0, c.tokens, c.input, 0)
        assert plan.type == want_type, c.name
        print("%-30s stored %d fixed %d dynamic %d -> type %d" % (c.name, sb, fb, db, plan.type))
        diffs.add(("fd", db - fb))
        if fb <= db:
            diffs.add(("sf", sb - fb))
        else:
            diffs.add(("sd", sb - db))
    assert diffs >= {(p, d) for p in ("fd", "sf", "sd") for d in (-1, 0, 1)}


def test_peak_bytes_hold_64_items_of_60_bits(shim):
    """huffman-only: 256 consecutive bytes with 15-bit codes, and -- k_encode<false> packs four bytes an item, the items
    counted from the header's first byte -- an aligned group of 64 items with 64 x 60 = 3840 bits, the size FL_STG_DW is
    made for."""
    best = 0
    for name, data, (start, length) in S.peak_cases():
        w = {}
        got, plan = encode_block(shim, 1, None, data, 1, widths=w)
        want = O.block_write("huff", np.zeros(0, np.uint32), 1, data)
        assert got == want and plan.type == 2, name
        assert zlib.decompress(got, -15) == data
        sym = w["sym"]
        assert length >= 256 and (sym[start:start + length] == 15).all(), name
        four = np.concatenate([sym, np.zeros(-sym.size % 4, np.int64)]).reshape(-1, 4).sum(1)
        items = np.concatenate([w["hdr"], four, [w["eob"]]])
        g = S.group_bits(items)
        # the group of a workgroup's wave: ranges of ceil(n / 4) items rounded up to 64, so aligned from item 0
        print("%-18s header %d bytes, widest group of 64 items %d bits (group %d of %d)" %
              (name, w["hdr"].size, int(g.max()), int(g.argmax()), g.size))
        assert int(four.max()) == 60
        best = max(best, int(g.max()))
    assert best == 3840
