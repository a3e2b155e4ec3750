"""GPU tests of seekable compress: flate_hip_compress_joined_indexed (the bytes of flate_hip_compress_joined, and a fresh
seek index whose points are piece starts) and flate_hip_decompress_ranges on such an index (k_inflate_part on both LDS
rings, direct and scratch parts, k_range_settle), export / import of the version-2 blob, the Python mirror and the tools,
through ctypes on device and on host memory.  The inputs and what they compress to are tests/_joined_cases.py."""
import ctypes as C
import io
import os
import struct
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

HOST, DEVICE = 0, 1
E_INVALID_ARG = -2
FILL = 0xA5
HDR = {O.RAW: 0, O.GZIP: 10, O.ZLIB: 2}
WBITS = {O.RAW: -15, O.GZIP: 31, O.ZLIB: 15}


class Mem:
    """arrays where memkind says: numpy arrays, or torch tensors on the device"""

    def __init__(self, kind):
        self.kind = kind

    def put(self, a):
        a = np.ascontiguousarray(a)
        if self.kind == HOST:
            a = a.copy()
            return a, a.ctypes.data
        import torch
        signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
        t = torch.from_numpy(a.view(signed).copy() if signed else a.copy()).cuda()
        return t, t.data_ptr()

    def get(self, holder, dtype):
        if self.kind == HOST:
            return holder
        return holder.cpu().numpy().view(dtype)

    def sync(self):
        if self.kind == DEVICE:
            import torch
            torch.cuda.synchronize()


def offsets(lens, base=0):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.array(lens, np.uint64))
    return off + np.uint64(base)


def rule_pieces(n, piece, spacing):
    """piece 0; piece k >= 1 iff a grid line lies in ((k - 1) * piece, k * piece]; spacing 0 is 1 MiB"""
    s = spacing or (1 << 20)
    return [k for k in range(max(1, -(-n // piece))) if k == 0 or (k * piece) // s > ((k - 1) * piece) // s]


def expected_points(data, piece, container, level, spacing):
    """[(in_bit, out_pos)] of the fresh index: the pieces the rule selects, each where the flushed pieces in front of it end"""
    ps = jc.pieces_of(data, piece)
    place, at = [], HDR[container]
    for p in ps:
        place.append(at)
        at += len(jc.flushed(p, level))
    return [(8 * place[k], k * piece) for k in rule_pieces(len(data), piece, spacing)]


def count_parts(pos, size, begin, length):
    """(direct, scratch) parts of the range [begin, begin + length) of a stream of `size` bytes with points at `pos`"""
    end = min(begin + length, size)
    direct = scratch = 0
    for k, p in enumerate(pos):
        nxt = pos[k + 1] if k + 1 < len(pos) else size
        a, b = max(begin, p), min(end, nxt)
        if a < b:
            if a == p and b == nxt:
                direct += 1
            else:
                scratch += 1
    return direct, scratch


def bounds(eng, streams, piece, container, level):
    return [(eng.joined_bound(len(s), piece, container, level) + 7) & ~7 for s in streams]


def compress_indexed(eng, streams, piece, container, level, spacing, kind, caps=None, out_base=0):
    """flate_hip_compress_joined_indexed in memory of one kind -> (rc, index handle or None, outs, statuses, whole buffer)"""
    m, n = Mem(kind), len(streams)
    caps = bounds(eng, streams, piece, container, level) if caps is None else caps
    off = offsets(caps, out_base)
    t_in = m.put(np.frombuffer(b"".join(streams) + b"\0", np.uint8))
    t_inoff, t_outoff = m.put(offsets([len(s) for s in streams])), m.put(off)
    t_out = m.put(np.full(int(off[-1]) + 64, FILL, np.uint8))
    t_len, t_st = m.put(np.zeros(n + 1, np.uint64)), m.put(np.full(n + 1, -77, np.int32))
    ix = C.c_void_p(0xdead)
    m.sync()
    eng._sync_env()
    rc = eng._L.flate_hip_compress_joined_indexed(eng._h, t_in[1], t_inoff[1], n, piece, container, level, t_out[1], t_outoff[1],
                                                  t_len[1], t_st[1], kind, spacing, C.byref(ix))
    m.sync()
    out, ln, st = m.get(t_out[0], np.uint8), m.get(t_len[0], np.uint64), m.get(t_st[0], np.int32)
    assert int(st[n]) == -77
    outs = [out[int(off[i]): int(off[i]) + int(ln[i])].tobytes() for i in range(n)]
    return rc, (ix if ix.value else None), outs, [int(s) for s in st[:n]], out


def run_ranges(eng, ix, comp, kind, ranges, caps, out_base=0):
    """flate_hip_decompress_ranges on the compressed streams `comp`, back to back in memory of one kind; ranges: [(stream,
    begin, len)], caps: the slots' sizes -> (rc, out, out_len, status, slot starts)"""
    m, n = Mem(kind), len(ranges)
    starts = offsets(caps, out_base)
    t_in = m.put(np.frombuffer(b"".join(comp) + b"\0", np.uint8))
    t_inoff = m.put(offsets([len(s) for s in comp]))
    rs = m.put(np.array([r[0] for r in ranges] + [0], np.uint32))
    rb = m.put(np.array([r[1] for r in ranges] + [0], np.uint64))
    rl = m.put(np.array([r[2] for r in ranges] + [0], np.uint64))
    so = m.put(starts)
    out = m.put(np.full(int(starts[-1]) + 64, FILL, np.uint8))
    ln, st = m.put(np.full(n + 1, 12345, np.uint64)), m.put(np.full(n + 1, -77, np.int32))
    m.sync()
    rc = eng.decompress_ranges_device(ix, t_in[1], t_inoff[1], len(comp), n, rs[1], rb[1], rl[1], out[1], so[1], ln[1], st[1], kind)
    m.sync()
    got_ln, got_st = m.get(ln[0], np.uint64), m.get(st[0], np.int32)
    assert int(got_ln[n]) == 12345 and int(got_st[n]) == -77
    return rc, m.get(out[0], np.uint8), got_ln, got_st, starts


def check_ranges(eng, ix, comp, datas, kind, ranges, tight=(), unspecified=None, status_of=None):
    """Every range delivers exactly data[b : b + L'] into a slot whose start takes every residue mod 16, fenced by the fill;
    the slots of `tight` are one byte too small: 100, nothing written.  status_of(j): the expected non-zero status of a
    range that fails (out_len 0; its first L' bytes are unspecified when it is in `unspecified`)."""
    caps, want = [], []
    for j, (i, b, n) in enumerate(ranges):
        data = datas[i]
        w = data[b:b + n] if b < len(data) else b""
        cap = len(w) + (j * 7) % 18
        if j in tight and w:
            cap = len(w) - 1
            want.append((100, b""))
        elif status_of is not None and status_of(j):
            want.append((status_of(j), b""))
        else:
            want.append((0, w))
        caps.append(cap)
    rc, out, ln, st, starts = run_ranges(eng, ix, comp, kind, ranges, caps, out_base=3)
    assert rc == 0
    clean = np.full(out.size, FILL, np.uint8)
    for j, (r, (status, data)) in enumerate(zip(ranges, want)):
        assert int(st[j]) == status and int(ln[j]) == len(data), (r, int(st[j]), int(ln[j]), status, len(data))
        a = int(starts[j])
        assert out[a:a + len(data)].tobytes() == data, r
        clean[a:a + len(data)] = out[a:a + len(data)]
        if unspecified and j in unspecified:  # the clipped length of a range with a failed part
            lp = max(0, min(r[2], len(datas[r[0]]) - r[1]))
            clean[a:a + lp] = out[a:a + lp]
    assert np.array_equal(out, clean), "a byte outside the first L' bytes of a slot was written"
    return starts


def ranges_around_points(si, size, piece, pos):
    """the ranges of one stream: the whole of it, begins and ends on every point and one byte either side of it, zero
    length, begins at and beyond the size"""
    out = [(si, 0, size), (si, 0, size + 100), (si, 0, 0), (si, size, 5), (si, size + 7, 5), (si, max(size - 1, 0), 5), (si, 1, 0)]
    for p in pos + [size]:
        for b in (p - 1, p, p + 1):
            if 0 <= b < size:
                out += [(si, b, 1), (si, b, piece), (si, b, 2 * piece + 1), (si, b, size)]
        for e in (p - 1, p, p + 1):
            for b in (0, 1, pos[len(pos) // 2], pos[len(pos) // 2] + 1):
                if b < e <= size:
                    out.append((si, b, e - b))
    return out


# ---------------------------------------------------------------- 1. the compress output and the points

@pytest.mark.parametrize("piece", jc.PIECES)
@pytest.mark.parametrize("container", jc.CONTAINERS)
@pytest.mark.parametrize("level", jc.LEVELS)
def test_output_is_compress_joined_and_points_are_piece_starts(level, container, piece):
    """one call over text, noise (stored blocks) and the 64-symbol bytes of every length around the piece size, an empty and
    a one-byte stream among them: the bytes, out_len and status of flate_hip_compress_joined, and the points the rule
    selects among the piece starts"""
    eng = engine()
    names, streams = zip(*jc.batch(piece))
    spacing = (1, piece, 2 * piece + 1, 0)[(level + container + piece) % 4]
    rc, ix, outs, st, _ = compress_indexed(eng, streams, piece, container, level, spacing, DEVICE)
    assert rc == 0 and ix is not None
    try:
        for i, (name, s) in enumerate(zip(names, streams)):
            want = jc.expected(s, piece, container, level)
            assert st[i] == 0 and outs[i] == want, name
            assert eng.index_info(ix, i) == (len(s), 0, len(rule_pieces(len(s), piece, spacing))), name
            assert eng.index_points(ix, i) == expected_points(s, piece, container, level, spacing), name
    finally:
        eng.index_destroy(ix)


@pytest.mark.parametrize("container", jc.CONTAINERS)
def test_host_and_device_memory_give_the_same_output_and_points(container):
    eng = engine()
    for piece, spacing in ((7, 15), (4096, 1)):
        names, streams = zip(*jc.batch(piece))
        got = []
        for kind in (HOST, DEVICE):
            rc, ix, outs, st, _ = compress_indexed(eng, streams, piece, container, 6, spacing, kind)
            assert rc == 0
            got.append((outs, st, [eng.index_points(ix, i) for i in range(len(streams))], eng.index_export(ix)))
            eng.index_destroy(ix)
        assert got[0] == got[1]
        assert got[0][0] == [jc.expected(s, piece, container, 6) for s in streams]
        assert got[0][2] == [expected_points(s, piece, container, 6, spacing) for s in streams]
        # the plain call, untouched
        plain, pst = eng.compress_joined(streams, container, 6, piece=piece)
        assert plain == got[0][0] and pst == got[0][1]


def test_a_stream_that_does_not_fit_has_no_points():
    eng = engine()
    streams = [jc.content("text", 3 * 4096 + 5), jc.content("noise", 2 * 4096), jc.content("text", 100, 7)]
    want = [jc.expected(s, 4096, O.GZIP, 6) for s in streams]
    caps = [len(want[0]), len(want[1]) - 1, len(want[2])]
    rc, ix, outs, st, buf = compress_indexed(eng, streams, 4096, O.GZIP, 6, 1, DEVICE, caps=caps, out_base=3)
    assert rc == 0 and st == [0, 100, 0] and outs == [want[0], b"", want[2]]
    try:
        assert eng.index_info(ix, 1) == (0, 100, 0) and eng.index_points(ix, 1) == []
        assert eng.index_info(ix, 0) == (len(streams[0]), 0, 4) and eng.index_info(ix, 2) == (100, 0, 1)
        assert (buf[3 + caps[0]: 3 + caps[0] + caps[1]] == FILL).all()
        rc, out, ln, rst, _ = run_ranges(eng, ix, outs, DEVICE, [(1, 0, 10), (0, 4090, 10), (2, 0, 100)], [10, 10, 100])
        assert rc == 0 and [int(x) for x in rst[:3]] == [100, 0, 0] and [int(x) for x in ln[:3]] == [0, 10, 100]
        assert out[10:20].tobytes() == streams[0][4090:4100] and out[20:120].tobytes() == streams[2] and (out[:10] == FILL).all()
    finally:
        eng.index_destroy(ix)


# ---------------------------------------------------------------- 2. every fresh point is a block start

def test_fresh_points_are_block_starts_of_the_stream():
    """flate_hip_index_build of the same streams at spacing 1 makes a point of the first block start at every output
    position: the fresh points are among them -- except that in front of piece k >= 1 lies the sync-flush marker, an
    empty stored block at the same output position, which is the build's point there; then the fresh point is the block
    start right behind that marker (three header bits, padding to the byte, 00 00 ff ff).  And stdlib zlib, started at a
    fresh point with no history, inflates the rest of the stream's output."""
    eng = engine()
    for container in jc.CONTAINERS:
        streams = [jc.content("text", 3 * 4096 + 5), jc.content("noise", 2 * 4096 + 1, 9), jc.content("sym64", 5 * 4096, 3), b"", b"x"]
        rc, ix, outs, st, _ = compress_indexed(eng, streams, 4096, container, 6, 1, DEVICE)
        assert rc == 0 and st == [0] * len(streams)
        built, back, bst, _ = eng.build_index(outs, container, 0, spacing=1)
        try:
            assert bst == [0] * len(streams) and back == list(streams)
            for i, s in enumerate(streams):
                fresh, every = eng.index_points(ix, i), built.points(i)
                assert len(fresh) == max(1, -(-len(s) // 4096)) and fresh[0] == every[0], i
                assert [p for _, p in fresh] == [k * 4096 for k in range(len(fresh))]
                at = dict((pos, bit) for bit, pos in every)
                for bit, pos in fresh[1:]:
                    body = (at[pos] + 3 + 7) // 8  # the marker's LEN / NLEN
                    assert outs[i][body:body + 4] == b"\x00\x00\xff\xff" and bit == 8 * (body + 4), (i, pos)
                    two = int.from_bytes(outs[i][at[pos] // 8: at[pos] // 8 + 2], "little")
                    assert (two >> (at[pos] % 8)) & 7 == 0  # BFINAL 0, BTYPE 00
                for bit, pos in fresh:
                    assert bit % 8 == 0 and pyzlib.decompressobj(-15).decompress(outs[i][bit // 8:]) == s[pos:], (i, pos)
        finally:
            built.close()
            eng.index_destroy(ix)


# ---------------------------------------------------------------- 3. ranges against the input bytes

@pytest.mark.parametrize("ring", [2048, 32768])
@pytest.mark.parametrize("kind", [DEVICE, HOST])
@pytest.mark.parametrize("piece", [7, 1001, 65535])
def test_ranges_deliver_the_input_bytes(monkeypatch, piece, kind, ring):
    """Pieces of 1001 bytes put part boundaries on every residue mod 8 of the slot address.  Every spacing; ranges around
    every point; slots at odd offsets, fenced; a slot one byte too small; both instances of k_inflate_part
    (FLATE_HIP_INFLATE_RING); direct parts and scratch parts both run."""
    monkeypatch.setenv("FLATE_HIP_INFLATE_RING", str(ring))
    eng = engine()
    n0 = {7: 5 * 7 + 3, 1001: 6 * 1001 + 5, 65535: 3 * 65535 + 5}[piece]
    datas = [jc.content("text", n0), jc.content("noise", 2 * piece + 1, 11), b"", b"q", jc.content("sym64", 3 * piece, 5)]
    for k, spacing in enumerate((1, piece, 2 * piece + 1, 0)):
        container = (O.RAW, O.GZIP, O.ZLIB, O.GZIP)[k]
        rc, ix, comp, st, _ = compress_indexed(eng, datas, piece, container, 6, spacing, kind)
        assert rc == 0 and st == [0] * len(datas)
        try:
            ranges = []
            for i, d in enumerate(datas):
                pos = [p for _, p in eng.index_points(ix, i)]
                assert pos == [q * piece for q in rule_pieces(len(d), piece, spacing)]
                ranges += ranges_around_points(i, len(d), piece, pos)
            tight = set(range(0, len(ranges), 5))
            check_ranges(eng, ix, comp, datas, kind, ranges, tight=tight)
            direct, scratch = eng.index_parts()
            assert direct > 0 and scratch > 0, (spacing, direct, scratch)
            # the whole streams alone: direct parts only
            whole = [(i, 0, len(d)) for i, d in enumerate(datas)]
            check_ranges(eng, ix, comp, datas, kind, whole)
            assert eng.index_parts() == (sum(len(rule_pieces(len(d), piece, spacing)) for d in datas if d), 0)
        finally:
            eng.index_destroy(ix)


# ---------------------------------------------------------------- 4. byte exactness at the seams of the parts

@pytest.mark.parametrize("ring", [2048, 32768])
@pytest.mark.parametrize("kind", [DEVICE, HOST])
def test_no_wave_writes_outside_its_part(monkeypatch, kind, ring):
    """One whole-stream range over streams of many pieces of 1001 bytes -- Huffman blocks, stored blocks, two-block pieces --
    in a slot at every alignment 0..7: adjacent direct parts are written by different waves at the same time, and every
    byte is the input's"""
    monkeypatch.setenv("FLATE_HIP_INFLATE_RING", str(ring))
    eng = engine()
    datas = [jc.content("text", 60 * 1001 + 13), jc.content("noise", 60 * 1001 + 500, 3), jc.content("sym64", 59 * 1001 + 1000, 1)]
    rc, ix, comp, st, _ = compress_indexed(eng, datas, 1001, O.RAW, 6, 1, kind)
    assert rc == 0 and st == [0, 0, 0]
    try:
        ranges, caps = [], []
        for a in range(8):
            for i, d in enumerate(datas):
                ranges.append((i, 0, len(d)))
                caps.append(len(d) + (1 - len(d)) % 8 + (8 if i == 2 else 0))  # (three slots on: the next residue)
        rc, out, ln, rst, starts = run_ranges(eng, ix, comp, kind, ranges, caps, out_base=5)
        assert rc == 0 and eng.index_parts() == (8 * (61 + 61 + 60), 0)
        assert {int(s) % 8 for s in starts[:-1:3]} == set(range(8))
        clean = np.full(out.size, FILL, np.uint8)
        for j, (i, _, n) in enumerate(ranges):
            a = int(starts[j])
            assert int(rst[j]) == 0 and int(ln[j]) == n
            got = out[a:a + n]
            if got.tobytes() != datas[i]:
                bad = np.flatnonzero(got != np.frombuffer(datas[i], np.uint8))
                raise AssertionError("range %d: %d bytes differ, the first at %d (part %d, byte %d of it)" %
                                     (j, bad.size, bad[0], bad[0] // 1001, bad[0] % 1001))
            clean[a:a + n] = got
        assert np.array_equal(out, clean)
    finally:
        eng.index_destroy(ix)


# ---------------------------------------------------------------- 5. passes

def test_many_ranges_in_passes_under_a_small_budget(monkeypatch):
    eng = engine()
    data = jc.content("text", 6 * 65535)
    rc, ix, comp, st, _ = compress_indexed(eng, [data], 4096, O.ZLIB, 6, 1, DEVICE)
    assert rc == 0 and st == [0]
    try:
        rng = np.random.default_rng(5)
        ranges = [(0, int(b), 9000) for b in rng.integers(0, len(data) - 9000, 200)]
        one = run_ranges(eng, ix, comp, DEVICE, ranges, [9000] * len(ranges))
        assert one[0] == 0 and eng.index_passes() == 1
        parts = eng.index_parts()
        pos = [4096 * k for k in range(96)]
        each = [count_parts(pos, len(data), b, n) for _, b, n in ranges]
        assert parts == (sum(d for d, _ in each), sum(s for _, s in each))
        assert parts[0] >= 200 and parts[1] >= 380  # (9000 bytes hold a whole piece of 4096, and begin and end inside others)
        monkeypatch.setenv("FLATE_HIP_INDEX_PASS_BYTES", str(64 * 1024))
        many = run_ranges(eng, ix, comp, DEVICE, ranges, [9000] * len(ranges))
        assert many[0] == 0 and eng.index_passes() > 1 and eng.index_parts() == parts
        for j, (_, b, n) in enumerate(ranges):
            assert int(many[3][j]) == 0 and int(many[2][j]) == n
            assert many[1][9000 * j:9000 * j + n].tobytes() == data[b:b + n]
        assert np.array_equal(one[1], many[1]) and np.array_equal(one[2], many[2]) and np.array_equal(one[3], many[3])
        # a budget below one scratch part: every scratch part is a pass of its own
        monkeypatch.setenv("FLATE_HIP_INDEX_PASS_BYTES", "100")
        few = run_ranges(eng, ix, comp, DEVICE, ranges[:10], [9000] * 10)
        assert few[0] == 0 and eng.index_passes() == eng.index_parts()[1] == sum(s for _, s in each[:10]) >= 18
        assert np.array_equal(few[1][:90000], one[1][:90000])
    finally:
        monkeypatch.delenv("FLATE_HIP_INDEX_PASS_BYTES", raising=False)
        eng.index_destroy(ix)
        eng.compress_many([b"x"], 0, 6)  # (the handle reads the knob again: the default for whoever comes next)


# ---------------------------------------------------------------- 6. a failing part stays local

@pytest.mark.parametrize("kind", [DEVICE, HOST])
def test_a_failing_part_fails_its_ranges_only(kind):
    """The compressed bytes of piece 5 zeroed: a stored header with LEN = NLEN = 0 is WrongStoredBlockNlen.  Ranges that touch
    the piece report it with out_len 0, the others deliver the input; nothing outside any slot's first L' bytes changes."""
    eng = engine()
    piece, bad = 1001, 5
    data = jc.content("text", 10 * piece + 77)
    rc, ix, comp, st, _ = compress_indexed(eng, [data], piece, O.RAW, 6, 1, kind)
    assert rc == 0 and st == [0]
    try:
        pts = eng.index_points(ix, 0)
        lo, hi = pts[bad][0] // 8, pts[bad + 1][0] // 8
        broken = comp[0][:lo] + bytes(hi - lo) + comp[0][hi:]
        ranges = [(0, 0, len(data)), (0, 0, bad * piece), (0, 0, bad * piece + 1), (0, (bad + 1) * piece, 3000), (0, (bad + 1) * piece - 1, 3000),
                  (0, bad * piece + 500, 1), (0, bad * piece, piece), (0, 3, 2 * piece), (0, 4 * piece + 1, 3 * piece), (0, 7 * piece, 5000),
                  (0, bad * piece - 1, 1), (0, (bad + 1) * piece, 1)]
        touches = {j for j, (_, b, n) in enumerate(ranges) if b < (bad + 1) * piece and min(b + n, len(data)) > bad * piece}
        assert len(touches) == 6
        check_ranges(eng, ix, [broken], [data], kind, ranges, unspecified=touches, status_of=lambda j: 13 if j in touches else 0)
        check_ranges(eng, ix, comp, [data], kind, ranges)  # (and the index is as good as before on the bytes it was made for)
    finally:
        eng.index_destroy(ix)


# ---------------------------------------------------------------- 7. streams that failed in the compress

def test_q1_streams_have_no_points_unless_repaired():
    from flate_amd import _capi
    eng = engine()
    n102 = 0
    plain = jc.content("text", 5000, 77)
    for name, data, piece in jc.q1_streams(6):
        is_q1 = any(O.decompress(jc.finished(p, 6), O.RAW, 0, cap=len(p) + 600)[1] != p for p in jc.pieces_of(data, piece))
        rc, ix, comp, st, _ = compress_indexed(eng, [data, plain], piece, O.GZIP, 6, 1, DEVICE)
        assert rc == 0 and st == [102 if is_q1 else 0, 0] and comp[0] == jc.expected(data, piece, O.GZIP, 6), name
        try:
            if is_q1:
                n102 += 1
                assert eng.index_info(ix, 0) == (0, 102, 0) and eng.index_points(ix, 0) == [], name
                rc, out, ln, rst, _ = run_ranges(eng, ix, comp, DEVICE, [(0, 0, 100), (1, 10, 100), (0, piece, 1)], [100, 100, 1])
                assert rc == 0 and [int(x) for x in rst[:3]] == [102, 0, 102] and [int(x) for x in ln[:3]] == [0, 100, 0]
                assert (out[:100] == FILL).all() and out[100:200].tobytes() == plain[10:110] and out[200] == FILL
            else:
                check_ranges(eng, ix, comp, [data, plain], DEVICE, [(0, 0, len(data)), (1, 0, 5000)])
        finally:
            eng.index_destroy(ix)
        eng.set_flags(_capi.DEFLATE_REPAIR_Q1)
        try:
            rc, ix, comp, st, _ = compress_indexed(eng, [data, plain], piece, O.GZIP, 6, 1, DEVICE)
        finally:
            eng.set_flags(0)
        assert rc == 0 and st == [0, 0] and pyzlib.decompress(comp[0], 31) == data, name
        try:
            assert eng.index_info(ix, 0) == (len(data), 0, 2) and [p for _, p in eng.index_points(ix, 0)] == [0, piece]
            check_ranges(eng, ix, comp, [data, plain], DEVICE, [(0, 0, len(data)), (0, piece - 1, 2), (0, piece, 3000), (1, 1, 4000)])
        finally:
            eng.index_destroy(ix)
    assert n102 >= 2


# ---------------------------------------------------------------- 8. export, import, ranges again

def test_export_import_on_a_fresh_handle():
    from flate_amd import Engine
    from flate_amd._capi import FlateHipError
    eng = engine()
    datas = [jc.content("text", 6 * 1001 + 5), b"", jc.content("noise", 3000, 1), jc.content("sym64", 2 * 1001, 2)]
    rc, ix, comp, st, _ = compress_indexed(eng, datas, 1001, O.GZIP, 6, 2003, DEVICE, caps=[8000, 1, 8000, 8000])
    assert rc == 0 and st == [0, 100, 0, 0]
    info = [eng.index_info(ix, i) for i in range(4)]
    pts = [eng.index_points(ix, i) for i in range(4)]
    blob = eng.index_export(ix)
    eng.index_destroy(ix)
    assert [len(p) for p in pts] == [3, 0, 1, 1] and info[1] == (0, 100, 0)
    assert [[q for _, q in p] for p in pts] == [[0, 3003, 5005], [], [0], [0]]
    assert len(blob) == 48 + 32 * 4 + 24 * 5
    magic, version, container, ns, spacing, npts, win_bytes, total = struct.unpack_from("<IIIIQQQQ", blob)
    assert (magic, version, container, ns, spacing, npts, win_bytes, total) == (0x58444946, 2, 1, 4, 2003, 5, 0, len(blob))
    assert all(struct.unpack_from("<II", blob, 48 + 32 * 4 + 24 * k + 16) == (0, 0) for k in range(5))
    ranges = [r for i, d in enumerate(datas) for r in ranges_around_points(i, len(d), 1001, [p for _, p in pts[i]] or [0])]
    failed = {j for j, r in enumerate(ranges) if r[0] == 1}
    other = Engine(0)
    try:
        ix2 = other.index_import(blob)
        assert [other.index_info(ix2, i) for i in range(4)] == info and [other.index_points(ix2, i) for i in range(4)] == pts
        assert other.index_export(ix2) == blob
        for kind in (DEVICE, HOST):  # (host memory on the fresh handle: only what the parts can consume is staged)
            check_ranges(other, ix2, comp, datas, kind, ranges, status_of=lambda j: 100 if j in failed else 0)
            assert min(other.index_parts()) > 0
        other.index_destroy(ix2)
        point_at = 48 + 32 * 4
        for bad in (blob[:-1], blob[:47], blob[:100], b"", blob + b"\0",
                    blob[:4] + struct.pack("<I", 1) + blob[8:],                                  # the other version
                    blob[:4] + struct.pack("<I", 3) + blob[8:],
                    blob[:32] + struct.pack("<Q", 1) + blob[40:],                                # win_bytes
                    blob[:point_at + 24 + 16] + struct.pack("<I", 1001) + blob[point_at + 24 + 20:]):  # a window length
            with pytest.raises(FlateHipError, match="-2"):
                other.index_import(bad)
        # a version-1 blob still imports and reads as before
        built, back, bst, _ = eng.build_index([comp[0]], O.GZIP, 0, spacing=1001)
        v1 = built.to_bytes()
        built.close()
        assert bst == [0] and struct.unpack_from("<II", v1) == (0x58444946, 1) and struct.unpack_from("<Q", v1, 32)[0] > 0
        old = other.index_from_bytes(v1, [comp[0]])
        outs, rst = old.read_ranges([(0, 1000, 3000), (0, 0, len(datas[0]))])
        assert rst == [0, 0] and outs == [datas[0][1000:4000], datas[0]] and old.to_bytes() == v1
        assert other.index_parts() == (0, 0)
        old.close()
    finally:
        other.close()


# ---------------------------------------------------------------- 9. the device flow as a caller writes it

def test_compress_gather_then_ranges_on_the_packed_streams():
    """compress into slots with slack -> flate_hip_gather_streams -> ranges: the index's in_len is the stream's out_len, so
    the streams must lie back to back"""
    import torch
    eng = engine()
    m = Mem(DEVICE)
    datas = [jc.content("text", 9 * 4096 + 100), jc.content("sym64", 3 * 4096, 4), jc.content("noise", 4096 + 9, 6)]
    n = len(datas)
    caps = bounds(eng, datas, 4096, O.ZLIB, 6)
    t_in = m.put(np.frombuffer(b"".join(datas), np.uint8))
    t_inoff, t_outoff = m.put(offsets([len(d) for d in datas])), m.put(offsets(caps))
    t_out = m.put(np.full(sum(caps) + 64, FILL, np.uint8))
    t_len, t_st = m.put(np.zeros(n, np.uint64)), m.put(np.full(n, -77, np.int32))
    torch.cuda.synchronize()
    ix = eng.compress_joined_indexed_device(t_in[1], t_inoff[1], n, 4096, O.ZLIB, 6, t_out[1], t_outoff[1], t_len[1], t_st[1], spacing=8192)
    try:
        t_dst, t_dstoff = m.put(np.full(sum(caps) + 64, FILL, np.uint8)), m.put(np.zeros(n + 1, np.uint64))
        eng.gather_streams_device(t_out[1], t_outoff[1], t_len[1], n, t_dst[1], t_dstoff[1])
        torch.cuda.synchronize()
        lens = m.get(t_len[0], np.uint64)
        assert [int(x) for x in m.get(t_st[0], np.int32)] == [0] * n
        assert [int(x) for x in m.get(t_dstoff[0], np.uint64)] == [int(x) for x in offsets([int(v) for v in lens])]
        assert [eng.index_info(ix, i)[0] for i in range(n)] == [len(d) for d in datas]
        ranges = [(0, 5000, 20000), (1, 0, 3 * 4096), (2, 4000, 200), (0, 8192, 8192), (0, 8191, 2)]
        caps_r = [r[2] for r in ranges]
        rs = m.put(np.array([r[0] for r in ranges], np.uint32))
        rb, rl = m.put(np.array([r[1] for r in ranges], np.uint64)), m.put(np.array([r[2] for r in ranges], np.uint64))
        so, out = m.put(offsets(caps_r)), m.put(np.full(sum(caps_r) + 64, FILL, np.uint8))
        ln, st = m.put(np.zeros(len(ranges), np.uint64)), m.put(np.full(len(ranges), -77, np.int32))
        torch.cuda.synchronize()
        assert eng.decompress_ranges_device(ix, t_dst[1], t_dstoff[1], n, len(ranges), rs[1], rb[1], rl[1], out[1], so[1], ln[1], st[1]) == 0
        # on the slots with slack the lengths are not the index's: refused
        assert eng.decompress_ranges_device(ix, t_out[1], t_outoff[1], n, len(ranges), rs[1], rb[1], rl[1], out[1], so[1], ln[1],
                                            st[1]) == E_INVALID_ARG
        torch.cuda.synchronize()
        got, at = m.get(out[0], np.uint8), 0
        assert [int(x) for x in m.get(st[0], np.int32)] == [0] * len(ranges)
        assert [int(x) for x in m.get(ln[0], np.uint64)] == [len(datas[i][b:b + k]) for i, b, k in ranges]
        for (i, b, k) in ranges:
            want = datas[i][b:b + k]  # (clipped to the stream's size)
            assert got[at:at + len(want)].tobytes() == want and (got[at + len(want):at + k] == FILL).all(), (i, b, k)
            at += k
        pos = [[0, 8192, 16384, 24576, 32768], [0, 8192], [0]]
        assert [[q for _, q in eng.index_points(ix, i)] for i in range(n)] == pos
        each = [count_parts(pos[i], len(datas[i]), b, k) for i, b, k in ranges]
        assert each == [(2, 2), (2, 0), (0, 1), (1, 0), (0, 2)] and eng.index_parts() == (5, 5)
    finally:
        eng.index_destroy(ix)


# ---------------------------------------------------------------- 10. errors

def test_argument_errors_and_the_empty_call():
    eng = engine()
    L, h = eng._L, eng._h
    data = np.frombuffer(jc.TEXT[:5000], np.uint8)
    in_off = np.array([0, 5000], np.uint64)
    out_off = np.array([0, 8192], np.uint64)

    def call(piece, container, mode, n=1, with_idx=True, spacing=1):
        out = np.full(8192, FILL, np.uint8)
        ln, st = np.full(1, 77, np.uint64), np.full(1, -77, np.int32)
        ix = C.c_void_p(0xdead)
        rc = L.flate_hip_compress_joined_indexed(h, data.ctypes.data, in_off.ctypes.data, n, piece, container, mode, out.ctypes.data,
                                                 out_off.ctypes.data, ln.ctypes.data, st.ctypes.data, 0, spacing,
                                                 C.byref(ix) if with_idx else None)
        return rc, out, int(ln[0]), int(st[0]), ix

    for piece, container, mode in ((4096, 0, 0), (4096, 1, 1), (4096, 3, 6), (4096, -1, 6), (65536, 1, 6), (4096, 1, 3), (4096, 1, 10)):
        rc, out, ln, st, ix = call(piece, container, mode)
        assert rc == E_INVALID_ARG and (out == FILL).all() and ln == 77 and st == -77 and ix.value is None, (piece, container, mode)
    rc, out, ln, st, ix = call(4096, 1, 6, with_idx=False)
    assert rc == E_INVALID_ARG and (out == FILL).all() and ln == 77 and st == -77
    ln1 = np.zeros(1, np.uint64)
    ix = C.c_void_p(0xdead)
    rc = L.flate_hip_compress_joined_indexed(h, data.ctypes.data, None, 1, 4096, 1, 6, None, out_off.ctypes.data, ln1.ctypes.data, None, 0, 1,
                                             C.byref(ix))
    assert rc == E_INVALID_ARG and ix.value is None
    # no streams: an empty index
    rc, out, ln, st, ix = call(4096, 1, 6, n=0)
    assert rc == 0 and (out == FILL).all() and ln == 77 and st == -77 and ix.value
    assert len(eng.index_export(ix)) == 48 and struct.unpack_from("<II", eng.index_export(ix)) == (0x58444946, 2)
    assert eng.decompress_ranges_device(ix, None, in_off.ctypes.data, 0, 0, None, None, None, None, None, None, None, HOST) == 0
    eng.index_destroy(ix)
    # ... and the call itself
    rc, out, ln, st, ix = call(4096, 1, 6, spacing=0)
    assert rc == 0 and st == 0 and out[:ln].tobytes() == jc.expected(jc.TEXT[:5000], 4096, O.GZIP, 6)
    assert eng.index_points(ix, 0) == expected_points(jc.TEXT[:5000], 4096, O.GZIP, 6, 0) and len(eng.index_points(ix, 0)) == 1
    eng.index_destroy(ix)
    res = eng.compress_joined([], O.GZIP, 6, index_spacing=1)
    assert res[:2] == ([], []) and len(eng.index_export(res[2])) == 48
    eng.index_destroy(res[2])
    assert eng.compress_joined([], O.GZIP, 6) == ([], [])


# ---------------------------------------------------------------- 11. the Python mirror and the tools

def test_index_keyword_of_compress():
    from flate_amd import api, flate, gzip, zlib
    engine()
    data = jc.content("text", 5 * 65535 + 17, 1234)
    for mod, container in ((flate, O.RAW), (gzip, O.GZIP), (zlib, O.ZLIB)):
        w = io.BytesIO()
        blob = mod.compress(io.BytesIO(data), w, joined=4096, index=True)
        assert w.getvalue() == jc.expected(data, 4096, container, 6)
        assert isinstance(blob, bytes) and struct.unpack_from("<II", blob) == (0x58444946, 2)
        assert struct.unpack_from("<Q", blob, 16)[0] == 1 << 20 and len(blob) == 48 + 32 + 24 * 1
        ix = mod.index_from_bytes(blob, w.getvalue())
        assert ix.size == len(data) and ix.read_at(300000, 5000) == data[300000:305000]
        ix.close()
        w = io.BytesIO()
        blob = mod.compress(data, w, api.Options(api.Level.best), joined=4096, index=10000)
        assert w.getvalue() == jc.expected(data, 4096, container, 9) and struct.unpack_from("<Q", blob, 16)[0] == 10000
        ix = mod.index_from_bytes(blob, w.getvalue())
        pts = ix.points()
        assert [p for _, p in pts] == [4096 * k for k in rule_pieces(len(data), 4096, 10000)] and pts == expected_points(data, 4096, container, 9, 10000)
        for a, b in ((0, 10), (4096, 8192), (123457, 300001), (len(data) - 5, len(data) + 100), (len(data), len(data) + 1)):
            assert ix.read_at(a, b - a) == data[a:b]
        assert ix.read_ranges([(5, 5), (200000, 70000)]) == [data[5:10], data[200000:270000]]
        assert ix.to_bytes() == blob
        ix.close()
        # without index= the call returns what it returned: nothing
        assert mod.compress(data[:100], io.BytesIO(), joined=True) is None
    with pytest.raises(ValueError):
        gzip.compress(data, io.BytesIO(), index=True)
    with pytest.raises(ValueError):
        gzip.compress(data, io.BytesIO(), joined=True, index=-5)


def test_gzip_tool_writes_an_index_gunzip_reads(tmp_path):
    engine()
    data = jc.content("text", 3 * 65535 + 100, 4321)
    path, idx = tmp_path / "input.txt", tmp_path / "input.idx"
    path.write_bytes(data)
    tools = os.path.join(ROOT, "tools")
    r = subprocess.run([sys.executable, os.path.join(tools, "gzip.py"), str(path), "--joined", "4096", "--index", str(idx), "--spacing", "65536"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    gz = (tmp_path / "input.txt.gz").read_bytes()
    assert gz == jc.expected(data, 4096, O.GZIP, 6) and pyzlib.decompress(gz, 31) == data
    blob = idx.read_bytes()
    assert struct.unpack_from("<IIIIQ", blob) == (0x58444946, 2, 1, 1, 65536) and len(blob) == 48 + 32 + 24 * 4
    r = subprocess.run([sys.executable, os.path.join(tools, "gunzip.py"), "--index", str(idx), "--range", "150000:1234",
                        str(tmp_path / "input.txt.gz")], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == data[150000:151234]
