"""The host-memory ways through flate_hip_decompress_batch that no other test takes at a small size: pinned buffers in
sub-batches (every input copy on the input stream before any output copy on the output stream, then per sub-batch the
kernels and an output copy), the single staged copy beside it, and what comes home from a pageable call dense and packed.
FLATE_HIP_HOST_PASS_CHUNKS=2 brings the sub-batches down to 20 streams; which way a call goes and how it is cut is asked
of the CPU build of the rule (tests/_inflate_plan.py, flate_amd/csrc/inflate_plan.h), never of the device.  The reference
is stdlib zlib."""
import zlib

import numpy as np
import pytest

import _inflate_plan as P
import _oracle as O

pytestmark = pytest.mark.gpu

KNOB = 2
EMPTY, CORRUPT = 5, 11
SIZES = [300, 70000, 1234, 65535, 65536, 0, 4097, 33000, 517, 20000, 69999, 45000, 800, 32768, 9001, 61000, 2500, 12345, 50001, 700]


def gzip(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


@pytest.fixture(scope="module")
def batch():
    """(streams, what each inflates to): 20 gzip streams of a few hundred to 70000 bytes of text, one of them empty and one
    with a damaged CRC-32 in its footer"""
    from flate_amd import synth
    text = synth.text(synth.SEED_TEXT + 31, sum(SIZES)).tobytes()
    plain, at = [], 0
    for n in SIZES:
        plain.append(text[at:at + n])
        at += n
    assert plain[EMPTY] == b"" and len(plain) == 20
    streams = [gzip(p) for p in plain]
    bad = bytearray(streams[CORRUPT])
    bad[-8] ^= 0xff
    streams[CORRUPT] = bytes(bad)
    for i, s in enumerate(streams):
        if i != CORRUPT:
            assert zlib.decompress(s, 31) == plain[i]
    with pytest.raises(zlib.error):
        zlib.decompress(streams[CORRUPT], 31)
    return streams, plain


@pytest.fixture
def engine(monkeypatch):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from flate_amd import Engine
    monkeypatch.setenv("FLATE_HIP_HOST_PASS_CHUNKS", str(KNOB))
    eng = Engine(0)
    eng._sync_env()
    yield eng
    eng.close()


def offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(sizes, dtype=np.uint64), out=off[1:])
    return off


def inflate(eng, streams, slots, pinned, with_consumed=True, fill=0):
    """one flate_hip_decompress_batch call on host memory -> (out buffer, out_off, out_len, status, consumed or None)"""
    import torch
    from flate_amd import _capi
    n = len(streams)
    in_off, out_off = offsets([len(s) for s in streams]), offsets(slots)
    blob = np.frombuffer(b"".join(streams), dtype=np.uint8).copy()
    out = np.full(int(out_off[-1]) + 8, fill, dtype=np.uint8)
    keep = [blob, out]
    if pinned:
        keep = [torch.from_numpy(blob).pin_memory(), torch.from_numpy(out).pin_memory()]
        src, dst = keep[0].data_ptr(), keep[1].data_ptr()
    else:
        src, dst = blob.ctypes.data, out.ctypes.data
    out_len, status = np.zeros(n, dtype=np.uint64), np.full(n, -77, dtype=np.int32)
    consumed = np.zeros(n, dtype=np.uint64) if with_consumed else None
    rc = eng._L.flate_hip_decompress_batch(eng._h, src, in_off.ctypes.data, n, O.GZIP, 0, dst, out_off.ctypes.data, out_len.ctypes.data,
                                           status.ctypes.data, consumed.ctypes.data if with_consumed else None, _capi.MEM_HOST)
    eng._check(rc, "flate_hip_decompress_batch")
    got = keep[1].numpy().copy() if pinned else out
    return got, out_off, out_len, status, consumed


def check(result, streams, plain, corrupt=None, want_corrupt=None, beyond=0):
    """every stream's bytes, out_len and status against zlib; the bytes of a slot beyond out_len are `beyond`"""
    out, out_off, out_len, status, consumed = result
    for i, p in enumerate(plain):
        a, b = int(out_off[i]), int(out_off[i + 1])
        if i == corrupt:
            assert (int(status[i]), int(out_len[i])) == want_corrupt
        else:
            assert int(status[i]) == 0 and int(out_len[i]) == len(p), i
            assert out[a:a + len(p)].tobytes() == p, i
            if consumed is not None:
                assert int(consumed[i]) == len(streams[i]), i
        assert not (out[a + int(out_len[i]):b] != beyond).any(), i


def round8(sizes):
    return [(n + 7) & ~7 for n in sizes]


def test_pinned_sub_batches_and_the_single_staged_copy(engine, batch):
    streams, plain = batch
    slots = round8(SIZES)
    in_bytes, out_bytes = sum(len(s) for s in streams), sum(slots)
    # the rule (CPU): 20 streams are above 4 * 2 and go in three sub-batches of 7, 7 and 6
    assert P.pin_io(True, True, in_bytes, out_bytes, 20, KNOB) and not P.pin_io(False, True, in_bytes, out_bytes, 20, KNOB)
    assert P.sub_batches(20, KNOB) == [7, 7, 6]
    # the damaged stream: what a pageable call (one staged copy, copy_out_host) says about it
    pageable = inflate(engine, streams, slots, pinned=False)
    want = (int(pageable[3][CORRUPT]), int(pageable[2][CORRUPT]))
    assert O.STATUS[want[0]] == "WrongGzipChecksum"
    check(pageable, streams, plain, CORRUPT, want)
    for with_consumed in (True, False):
        pinned = inflate(engine, streams, slots, pinned=True, with_consumed=with_consumed, fill=0xAA)
        check(pinned, streams, plain, CORRUPT, want)     # (zeros beyond out_len, not the caller's 0xAA -- with slots this tight the
        # single staged copy would do the same; that the sub-batches ran is shown by the test below, with wider slots)
        assert np.array_equal(pinned[2], pageable[2]) and np.array_equal(pinned[3], pageable[3])
        if with_consumed:
            assert np.array_equal(pinned[4], pageable[4])
    # 8 streams are not above 4 * 2: pinned buffers, and still the single staged copy -- identical results
    first = [i for i in range(20) if i not in (EMPTY, CORRUPT)][:6] + [EMPTY, CORRUPT]
    s8, p8, slots8 = [streams[i] for i in first], [plain[i] for i in first], [slots[i] for i in first]
    assert not P.pin_io(True, True, sum(map(len, s8)), sum(slots8), 8, KNOB)
    for with_consumed in (True, False):
        one = inflate(engine, s8, slots8, pinned=True, with_consumed=with_consumed)
        check(one, s8, p8, 7, want)
        assert [int(x) for x in one[2]] == [int(pageable[2][i]) for i in first]
        assert [int(x) for x in one[3]] == [int(pageable[3][i]) for i in first]


def test_pinned_twice_on_one_handle_the_second_batch_smaller(engine, batch):
    """the second call finds the handle's staging buffers full of the first call's output and its output stream behind the
    first call's copies: nothing of that may show, the bytes of a slot beyond out_len are zeros"""
    streams, plain = batch
    good = [i for i in range(20) if i != CORRUPT]
    slots = round8(SIZES)
    check(inflate(engine, [streams[i] for i in good] + [streams[0]], [slots[i] for i in good] + [slots[0]], pinned=True, fill=0x55),
          [streams[i] for i in good] + [streams[0]], [plain[i] for i in good] + [plain[0]])
    # 12 streams, the short ones first, every slot three times its stream and 24 bytes
    order = sorted(good, key=lambda i: SIZES[i])[:12]
    s2, p2 = [streams[i] for i in order], [plain[i] for i in order]
    slots2 = [3 * ((len(p) + 7) & ~7) + 24 for p in p2]
    assert P.pin_io(True, True, sum(map(len, s2)), sum(slots2), 12, KNOB) and P.sub_batches(12, KNOB) == [6, 6]
    # This is what shows that the library found the buffers pinned and took the sub-batches, which bring whole slots home:
    # the single staged copy would bring these slots home packed and leave the caller's 0x55 beyond every out_len.
    assert P.copy_out(list(offsets(slots2)), [len(p) for p in p2])[0] == P.PACKED
    check(inflate(engine, s2, slots2, pinned=True, fill=0x55), s2, p2)
    # ... as it does for the same buffers when they are pageable
    check(inflate(engine, s2, slots2, pinned=False, fill=0x55), s2, p2, beyond=0x55)


@pytest.mark.parametrize("factor, kind", [(1, P.DENSE), (16, P.PACKED)])
def test_pageable_copy_out_dense_and_packed(engine, batch, factor, kind):
    """slots exactly the streams' sizes: the range comes home as it is; slots of 16 times that: only the produced bytes,
    packed -- either way the caller's buffer beyond each out_len stays the zeros it held"""
    streams, plain = batch
    pick = [1, 2, 6, 8, 12, 17]
    s6, p6 = [streams[i] for i in pick], [plain[i] for i in pick]
    slots = [factor * len(p) for p in p6]
    assert P.copy_out(list(offsets(slots)), [len(p) for p in p6])[0] == kind
    result = inflate(engine, s6, slots, pinned=False)
    check(result, s6, p6)
    assert not result[0][int(result[1][-1]):].any()
