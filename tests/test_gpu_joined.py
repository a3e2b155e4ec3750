"""GPU tests of joined compress: flate_hip_compress_joined on device and on host memory, byte for byte against
tests/_joined_cases.py (whose expectations tests/test_joined_cases_cpu.py holds against stdlib zlib): every level, container
and piece size, single pieces against flate_hip_compress_batch, pieces over several passes, tight and fenced slots, the
bound, Q1 pieces, a round trip of 8 MiB, the errors of the call, joined= of the Python mirror and tools/gzip.py --joined."""
import io
import os
import subprocess
import sys
import zlib as pyzlib

import numpy as np
import pytest

import _joined_cases as jc
import _oracle as O
from conftest import ROOT
from gpu_util import engine

pytestmark = pytest.mark.gpu

FILL = 0xA5
WBITS = {O.RAW: -15, O.GZIP: 31, O.ZLIB: 15}


def offsets(lens, base=0):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off + base


def run_device(eng, streams, piece, container, mode, caps, out_base=0):
    """flate_hip_compress_joined on device memory, slot i of caps[i] bytes, the first one out_base bytes into the buffer.
    Returns (outs, statuses, whole buffer)."""
    import torch

    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()

    n = len(streams)
    t_in = dev(np.frombuffer(b"".join(streams) + b"\0", np.uint8))
    off = offsets(caps, out_base)
    t_inoff, t_outoff = dev(offsets([len(s) for s in streams])), dev(off)
    t_out = torch.full((int(off[-1]) + 64,), FILL, dtype=torch.uint8, device="cuda")
    t_len = torch.zeros(n, dtype=torch.int64, device="cuda")
    t_st = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.compress_joined_device(t_in.data_ptr(), t_inoff.data_ptr(), n, piece, container, mode, t_out.data_ptr(), t_outoff.data_ptr(),
                               t_len.data_ptr(), t_st.data_ptr())
    torch.cuda.synchronize()
    out, ln, st = t_out.cpu().numpy(), t_len.cpu().numpy(), t_st.cpu().numpy()
    outs = [out[int(off[i]): int(off[i]) + int(ln[i])].tobytes() for i in range(n)]
    return outs, [int(s) for s in st], out


def bounds(eng, streams, piece, container, mode):
    return [(eng.joined_bound(len(s), piece, container, mode) + 7) & ~7 for s in streams]


def check(names, outs, st, want, status=0):
    for name, o, s, w in zip(names, outs, st, want):
        assert s == status, (name, s)
        assert len(o) == len(w), (name, len(o), len(w))
        assert o == w, name


# ---------------------------------------------------------------- parity with the oracle

@pytest.mark.parametrize("piece", jc.PIECES)
@pytest.mark.parametrize("container", jc.CONTAINERS)
@pytest.mark.parametrize("level", jc.LEVELS)
def test_parity_with_the_oracle(level, container, piece):
    """one call over text, noise (stored ends: the five-byte marker) and the 64-symbol bytes (two-block pieces) of every
    length around the piece size"""
    eng = engine()
    names, streams = zip(*jc.batch(piece))
    want = [jc.expected(s, piece, container, level) for s in streams]
    outs, st, _ = run_device(eng, streams, piece, container, level, bounds(eng, streams, piece, container, level))
    check(names, outs, st, want)


@pytest.mark.parametrize("container", jc.CONTAINERS)
def test_host_and_device_memory_give_the_same_bytes(container):
    eng = engine()
    for piece in (7, 4096):
        names, streams = zip(*jc.batch(piece))
        want = [jc.expected(s, piece, container, 6) for s in streams]
        houts, hst = eng.compress_joined(streams, container, 6, piece=piece)
        check(names, houts, hst, want)
        douts, dst, _ = run_device(eng, streams, piece, container, 6, bounds(eng, streams, piece, container, 6))
        assert douts == houts and dst == hst


@pytest.mark.parametrize("container", jc.CONTAINERS)
@pytest.mark.parametrize("level", jc.LEVELS)
def test_a_single_piece_is_the_batch_streams(level, container):
    """P == 1: byte for byte flate_hip_compress_batch with the same container"""
    eng = engine()
    streams = [s for piece in jc.PIECES for _, s in jc.batch(piece) if len(s) <= 4096]
    streams.append(jc.content("text", 65535, 999))
    plain, pst = eng.compress_many(streams, container, level)
    for piece in (4096, 65535, 0):
        if piece == 4096:
            sub = [s for s in streams if len(s) <= 4096]
            outs, st, _ = run_device(eng, sub, piece, container, level, bounds(eng, sub, piece, container, level))
            assert outs == [p for p, s in zip(plain, streams) if len(s) <= 4096] and st == [0] * len(sub)
        else:  # (0 means 65535)
            outs, st, _ = run_device(eng, streams, piece, container, level, bounds(eng, streams, 65535, container, level))
            assert outs == plain and st == pst == [0] * len(streams), piece


# ---------------------------------------------------------------- more pieces than a pass holds

def test_pieces_over_several_passes(monkeypatch):
    """passes of seven pieces: a stream of 20 pieces of 4096 bytes (it straddles the ends of passes 0 and 1), one of four
    pieces (pass 2's end) and one of five (pass 3's end)"""
    eng = engine()
    streams = [jc.content("text", 20 * 4096), jc.content("noise", 3 * 4096 + 100, 50), jc.content("sym64", 5 * 4096, 70)]
    names = ["a", "b", "c"]
    for container in (O.GZIP, O.ZLIB):
        want = [jc.expected(s, 4096, container, 6) for s in streams]
        caps = bounds(eng, streams, 4096, container, 6)
        outs, st, _ = run_device(eng, streams, 4096, container, 6, caps)
        check(names, outs, st, want)
        monkeypatch.setenv("FLATE_HIP_MAX_PASS_CHUNKS", "7")
        outs7, st7, _ = run_device(eng, streams, 4096, container, 6, caps)
        houts7, hst7 = eng.compress_joined(streams, container, 6, piece=4096)
        monkeypatch.delenv("FLATE_HIP_MAX_PASS_CHUNKS")
        check(names, outs7, st7, want)
        check(names, houts7, hst7, want)
    eng.compress_many([b"x"], 0, 6)  # (the handle reads the knob again: the default for whoever comes next)


# ---------------------------------------------------------------- slots

@pytest.mark.parametrize("container", jc.CONTAINERS)
def test_tight_unaligned_fenced_slots(container):
    """every stream in a slot of exactly its length, at unaligned starts, with one-byte slots of empty streams between
    them as guards (an empty stream needs two bytes at least: status 100, the byte stays) -- then one slot a byte short:
    100 for that stream alone, nothing written into its slot, neighbours and guards as they were"""
    eng = engine()
    real = [jc.content("text", 3 * 4096 + 5), jc.content("noise", 2 * 4096), jc.content("sym64", 4096 + 1, 9), jc.content("text", 777, 3)]
    want = [jc.expected(s, 4096, container, 6) for s in real]
    streams = [b""]
    for s in real:
        streams += [s, b""]
    for short in (None, 0, 1, 3):
        caps = [1]
        for i, w in enumerate(want):
            caps += [len(w) - (1 if short == i else 0), 1]
        outs, st, buf = run_device(eng, streams, 4096, container, 6, caps, out_base=3)
        off = offsets(caps, 3)
        assert (buf[:3] == FILL).all() and (buf[int(off[-1]):] == FILL).all()
        for k in range(len(streams)):
            slot = buf[int(off[k]): int(off[k + 1])]
            if k % 2 == 0:
                assert st[k] == 100 and outs[k] == b"" and (slot == FILL).all(), (short, k)
            elif short == k // 2:
                assert st[k] == 100 and outs[k] == b"" and (slot == FILL).all(), (short, k)
            else:
                assert st[k] == 0 and outs[k] == want[k // 2] and slot.tobytes() == want[k // 2], (short, k)


def test_bound_holds_every_length_seen():
    eng = engine()
    for level in jc.LEVELS:
        for piece in jc.PIECES:
            for name, s in jc.batch(piece):
                for container in jc.CONTAINERS:
                    b = eng.joined_bound(len(s), piece, container, level)
                    assert len(jc.expected(s, piece, container, level)) <= b, (name, piece, container)
                    ps = jc.pieces_of(s, piece)
                    assert b == {0: 0, 1: 18, 2: 6}[container] + sum(eng.compress_bound(len(p), O.RAW, level) + 5 for p in ps)
    noise = jc.content("noise", 5 * 65535)  # five pieces that go out stored: the worst there is
    for piece in (65535, 0):
        outs, st, _ = run_device(eng, [noise], piece, O.GZIP, 6, [eng.joined_bound(len(noise), piece, O.GZIP, 6)])
        assert st == [0] and outs[0] == jc.expected(noise, 65535, O.GZIP, 6)
        assert len(outs[0]) > 18 + len(noise) + 5 * 5 + 4 * 5  # (a stored block or two a piece, four long markers)


# ---------------------------------------------------------------- Q1

@pytest.mark.parametrize("level", jc.LEVELS)
def test_q1_pieces_are_reported_and_repairable(level):
    from flate_amd import _capi
    eng = engine()
    n102 = 0
    for name, data, piece in jc.q1_streams(level):
        broken = any(O.decompress(jc.finished(p, level), O.RAW, 0, cap=len(p) + 600)[1] != p for p in jc.pieces_of(data, piece))
        outs, st = eng.compress_joined([data], O.GZIP, level, piece=piece)
        assert st == [102 if broken else 0] and outs[0] == jc.expected(data, piece, O.GZIP, level), name
        n102 += broken
        eng.set_flags(_capi.DEFLATE_REPAIR_Q1)
        try:
            outs, st = eng.compress_joined([data], O.GZIP, level, piece=piece)
        finally:
            eng.set_flags(0)
        assert st == [0] and pyzlib.decompress(outs[0], 31) == data, name
    assert n102 >= 4


# ---------------------------------------------------------------- a round trip at size

def test_round_trip_of_8_mib():
    from flate_amd import synth
    eng = engine()
    text = synth.text(synth.SEED_TEXT + 5, 8 << 20).tobytes()
    outs, st = eng.compress_joined([text], O.GZIP, 6)
    assert st == [0] and pyzlib.decompress(outs[0], 31) == text
    back, bst, used = eng.decompress_many(outs, O.GZIP, caps=[len(text) + 8])
    assert bst == [0] and back[0] == text and used == [len(outs[0])]
    assert len(outs[0]) < len(text) // 2


# ---------------------------------------------------------------- errors, the Python mirror, the tool

def test_argument_errors_and_the_empty_call():
    eng = engine()
    L, h = eng._L, eng._h
    data = np.frombuffer(jc.TEXT[:5000], np.uint8)
    in_off = np.array([0, 5000], np.uint64)
    out_off = np.array([0, 8192], np.uint64)

    def call(piece, container, mode, n=1):
        out = np.full(8192, FILL, np.uint8)
        ln, st = np.full(1, 77, np.uint64), np.full(1, -77, np.int32)
        rc = L.flate_hip_compress_joined(h, data.ctypes.data, in_off.ctypes.data, n, piece, container, mode, out.ctypes.data,
                                         out_off.ctypes.data, ln.ctypes.data, st.ctypes.data, 0)
        return rc, out, int(ln[0]), int(st[0])

    for piece, container, mode in ((4096, 0, 0), (4096, 1, 1), (4096, 3, 6), (4096, -1, 6), (65536, 1, 6), (4096, 1, 3), (4096, 1, 10)):
        rc, out, ln, st = call(piece, container, mode)
        assert rc == -2 and (out == FILL).all() and ln == 77 and st == -77, (piece, container, mode)
    rc, out, ln, st = call(4096, 1, 6, n=0)
    assert rc == 0 and (out == FILL).all() and ln == 77 and st == -77
    rc, out, ln, st = call(4096, 1, 6)
    assert rc == 0 and st == 0 and out[:ln].tobytes() == jc.expected(jc.TEXT[:5000], 4096, O.GZIP, 6)
    assert eng.compress_joined([], O.GZIP, 6) == ([], [])
    with pytest.raises(ValueError):
        eng.compress_joined([b"abc"], O.GZIP, 6, piece=65536)


def test_joined_keyword_of_compress():
    from flate_amd import api, flate, gzip, zlib
    engine()
    data = jc.content("text", 3 * 65535 + 17, 1234)
    for mod, container in ((flate, O.RAW), (gzip, O.GZIP), (zlib, O.ZLIB)):
        w = io.BytesIO()
        mod.compress(io.BytesIO(data), w, joined=True)
        assert w.getvalue() == jc.expected(data, 65535, container, 6)
        w = io.BytesIO()
        mod.compress(data, w, api.Options(api.Level.best), joined=4096)
        assert w.getvalue() == jc.expected(data, 4096, container, 9)
        assert pyzlib.decompressobj(WBITS[container]).decompress(w.getvalue()) == data
    for bad in (0, 65536, -1):
        with pytest.raises(ValueError):
            gzip.compress(data, io.BytesIO(), joined=bad)
    with pytest.raises(ValueError):
        zlib.compress(b"abc", io.BytesIO(), joined=True, zdict=b"abcdef")
    with pytest.raises(ValueError):
        gzip.compress(b"abc", io.BytesIO(), joined=True, piece=4096)
    for simple in (gzip.huffman, gzip.store):
        with pytest.raises(ValueError):
            simple.compress(b"abc", io.BytesIO(), joined=True)
    w = io.BytesIO()
    gzip.compress(b"abc", w)  # (without joined= nothing has changed)
    assert w.getvalue() == O.compress(b"abc", O.GZIP, 6)


def test_gzip_tool_joined(tmp_path):
    engine()
    data = jc.content("text", 2 * 65535 + 100, 4321)
    path = tmp_path / "input.txt"
    path.write_bytes(data)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gzip.py"), str(path), "--joined"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "input.txt.gz").read_bytes() == jc.expected(data, 65535, O.GZIP, 6)
