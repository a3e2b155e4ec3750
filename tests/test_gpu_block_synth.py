"""The block bit packers on the synthesized token blocks of _block_synth.py (token blocks no tokenizer emits: groups of
more than 2048 bits, items that spill into a third dword, every count around a group boundary, header sizes, empty
alphabets, block-type ties), byte for byte against the oracle's block writer -- through flate_hip_debug_write_blocks,
which runs k_plan, k_offsets and either token encoder on many blocks at once -- and the huffman-only packer at its
widest group through the production path."""
import zlib

import pytest

import _block_synth as S
import _oracle as O
from gpu_util import engine

pytestmark = pytest.mark.gpu

ENCODERS = {"k_encode": 0, "k_encode_wave": 1}
_want = {}


def want(c, fn, inp, eof):
    """The oracle's block, computed once per variant and shared by the tests."""
    key = (c.name, fn, inp is not None, eof)
    if key not in _want:
        _want[key] = O.block_write(fn, c.tokens, eof, inp)
    return _want[key]


def _starts(eng, blocks, salt):
    """Slot starts at every residue mod 4, a block's bound (which holds 8 spare bytes) apart."""
    at, starts = 0, []
    for i, (tok, inp, _) in enumerate(blocks):
        at = (at + 3) // 4 * 4 + (i * 7 + salt) % 4
        starts.append(at)
        at += eng.debug_block_bound(len(tok), 0 if inp is None else len(inp))
    assert {s % 4 for s in starts} == {0, 1, 2, 3} or len(starts) < 4
    return starts


def _check(eng, cases, variants, encoder):
    """Every (case, input, eof) of `variants` as one launch per block-writer function and slot layout."""
    for fn in ("wb", "dyn"):
        for paired in (True, False):
            todo = [(c, inp, eof) for c in cases for inp, eof in variants(c)]
            if not paired and len(todo) % 2 == 0:
                todo.append(todo[0])  # one slot a chunk and an ODD count: the other index order of k_encode_wave's callers
            assert len(todo) < 200
            blocks = [(c.tokens, inp, eof) for c, inp, eof in todo]
            got = eng.debug_write_blocks(blocks, encoder=encoder, paired=paired, dynamic_only=fn == "dyn",
                                         slot_starts=_starts(eng, blocks, int(paired)))
            for (c, inp, eof), g in zip(todo, got):
                assert g == want(c, fn, inp, eof), (c.name, fn, "paired" if paired else "single", inp is not None, eof)


@pytest.mark.parametrize("encoder", list(ENCODERS), ids=list(ENCODERS))
@pytest.mark.parametrize("with_input", [True, False], ids=["input", "null"])
def test_every_case_through_both_token_encoders(encoder, with_input):
    eng = engine()
    if with_input:
        cases = [c for c in S.token_cases() if c.input is not None]
        _check(eng, cases, lambda c: [(c.input, 0), (c.input, 1)], ENCODERS[encoder])
    else:
        _check(eng, S.token_cases(), lambda c: [(None, 0), (None, 1)], ENCODERS[encoder])


@pytest.mark.parametrize("encoder", list(ENCODERS), ids=list(ENCODERS))
def test_wide_groups_at_every_lane_phase(encoder):
    """The run of 42-bit tokens behind 0..63 literals: the groups of more than 2048 bits start at every lane, and the
    headers differ, so at several bit offsets."""
    eng = engine()
    _check(eng, S.wide_phase_cases(), lambda c: [(c.input if c.eof else None, c.eof)], ENCODERS[encoder])


def test_single_block_seam_agrees():
    """flate_hip_debug_write_block (one block, bit offset 0, k_encode<true>) and the batch seam on the same cases."""
    eng = engine()
    cases = S.token_cases()
    todo = [(c, inp) for c in cases for inp in ((c.input, None) if c.input is not None else (None,))]
    for dyn in (0, 1):
        batch = eng.debug_write_blocks([(c.tokens, inp, c.eof) for c, inp in todo], encoder=0, paired=False,
                                       dynamic_only=bool(dyn))
        for (c, inp), b in zip(todo, batch):
            one = eng.debug_write_block(c.tokens, inp, c.eof, bool(dyn))
            assert one == b == want(c, "dyn" if dyn else "wb", inp, c.eof), (c.name, dyn, inp is not None)


@pytest.mark.parametrize("container", [O.RAW, O.GZIP, O.ZLIB], ids=["raw", "gzip", "zlib"])
def test_peak_bytes_through_huffman_only_compress(container):
    """k_encode<false> at the staging window's design point -- 64 items of four 15-bit bytes -- as single blocks and as
    the middle block of a stream, where it starts at a bit offset behind another Huffman block."""
    from flate_amd import synth
    eng = engine()
    peaks = [data for _, data, _ in S.peak_cases()]
    head = synth.text(synth.SEED_TEXT, 65535).tobytes()
    tail = synth.text(synth.SEED_TEXT + 2, 200000 - 2 * 65535).tobytes()
    inputs = peaks + [head + p + tail for p in peaks[:4] + peaks[-1:]]
    outs, st = eng.compress_many(inputs, container, O.HUFFMAN)
    assert st == [0] * len(inputs)
    for i, (data, got) in enumerate(zip(inputs, outs)):
        assert got == O.compress(data, container, O.HUFFMAN), i
    back, st, _ = eng.decompress_many(outs, container, caps=[len(d) + 1 for d in inputs])
    assert st == [0] * len(inputs) and back == inputs


@pytest.mark.parametrize("level", [4, 6, 9])
def test_wide_blocks_through_level_compress(level):
    """The bytes that `wide-tokens` and `every-code` stand for through the production path: the tokenizer chooses its
    own tokens (the expansion of mostly matches has little variety); far, long matches with rare codes flow through
    k_plan and the encoder a batch of this size takes, as chunks and as whole streams behind 70000 other bytes."""
    from flate_amd import synth
    eng = engine()
    by_name = {c.name: c for c in S.token_cases()}
    junk = synth.text(synth.SEED_TEXT + 3, 70000).tobytes()
    inputs = []
    for name in ("wide-tokens", "every-code"):
        data = by_name[name].input
        inputs += [data[-65535:], data[:65535], junk + data]
    outs, st = eng.compress_many(inputs, O.RAW, level)
    for i, (data, got) in enumerate(zip(inputs, outs)):
        ref = O.compress(data, O.RAW, level)
        assert got == ref, (level, i)
        # status 102 exactly where the reference's own stream does not inflate to the input (its quirk at a full token
        # block, flate_hip.h FLATE_HIP_ST_REFERENCE_Q1_STREAM), 0 everywhere else
        try:
            valid = zlib.decompress(ref, -15) == data
        except zlib.error:
            valid = False
        assert st[i] == (0 if valid else 102), (level, i, st[i], valid)
