"""Every place where the library computes a CRC-32 or an Adler-32, against Python's zlib on the plain bytes (never the oracle,
never the library itself), over tests/_checksum_cases.py: contents (all 0xFF -- Adler-32's worst case --, zeros, random, a single
odd byte at either end or in the middle) x lengths at the arithmetic limits of the code, at every alignment 0..15 of the plain
bytes in the memory a kernel reads (compress) or writes and sums (inflate).

Compress side (C1..C5): the assertion is on the footer bytes cut from the output (CRC-32 and ISIZE little-endian; Adler-32
big-endian).  Inflate side (D1..D5): streams of stored blocks written here, header and footer from zlib; the right footer must
give Ok and the bytes, one flipped footer bit the Wrong... status -- and for the workgroup-per-stream kernel and the span path,
which hand a stream whose footer they cannot confirm on to k_inflate, a case only counts when Engine.inflate_paths() says that
the path under test finished it (no stream handed on), so a wrong checksum there cannot hide behind a second decode.

The cases whose names contain "4gib" or "1gib" move gigabytes: `-k "not 4gib and not 1gib"` leaves them out."""
import json
import os
import subprocess
import sys
import zlib as pyzlib

import numpy as np
import pytest

import _big_member as B
import _checksum_cases as K
from conftest import ROOT
from gpu_util import engine

pytestmark = pytest.mark.gpu

GZIP, ZLIB = 1, 2
STORE, HUFFMAN = 0, 1
KNOBS = ("FLATE_HIP_INFLATE_PAR", "FLATE_HIP_INFLATE_SPANS", "FLATE_HIP_INFLATE_RING", "FLATE_HIP_SPAN_TWO_RUNS")
# the knobs of tests/test_gpu_inflate_synth.py's PATHS; here the span path is switched off where another path is meant (left
# on, it takes every long stream of a small batch first)
PATHS = {
    "D1-k_inflate-ring2048": {"FLATE_HIP_INFLATE_PAR": "0", "FLATE_HIP_INFLATE_SPANS": "0", "FLATE_HIP_INFLATE_RING": "2048"},
    "D1-k_inflate-ring32768": {"FLATE_HIP_INFLATE_PAR": "0", "FLATE_HIP_INFLATE_SPANS": "0", "FLATE_HIP_INFLATE_RING": "32768"},
    "D2-k_inflate_par": {"FLATE_HIP_INFLATE_PAR": "1", "FLATE_HIP_INFLATE_SPANS": "0"},
    "D3-spans-symbols": {"FLATE_HIP_INFLATE_PAR": "0", "FLATE_HIP_INFLATE_SPANS": "1"},
    "D3-spans-two-runs": {"FLATE_HIP_INFLATE_PAR": "0", "FLATE_HIP_INFLATE_SPANS": "1", "FLATE_HIP_SPAN_TWO_RUNS": "1"},
}
WRONG = {GZIP: 4, ZLIB: 6}  # WrongGzipChecksum, WrongZlibChecksum
BIG = 4097 * K.BLOCK + 1
MID = 65 * K.BLOCK + 1  # the lengths up to here go through everything; the ones above through what is cheap at any size


def choose(monkeypatch, path):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS.get(path, {}).items():
        monkeypatch.setenv(k, v)


def cut_footer(container, out):
    return out[len(out) - K.FOOTER_BYTES[container]:]


def padded_batch(datas, offset):
    """[pad, data, pad, data, ...]: every data chunk starts `offset` bytes past a multiple of 16 in the batch's input.
    Engine.compress_many joins the chunks back to back and the library stages that blob at the start of a device allocation (256-byte
    aligned), so this is the alignment of the address the checksum kernel reads.  Returns (chunks, index of every data chunk)."""
    chunks, idx, pos = [], [], 0
    for d in datas:
        pad = (offset - pos) % 16
        chunks.append(b"\xa5" * pad)
        pos += pad
        assert pos % 16 == offset
        idx.append(len(chunks))
        chunks.append(d)
        pos += len(d)
    return chunks, idx


def check_footers(eng, datas, names, container, mode, offset=None):
    if offset is None:
        chunks, idx = list(datas), list(range(len(datas)))
    else:
        chunks, idx = padded_batch(datas, offset)
    outs, st = eng.compress_many(chunks, container, mode)
    bad = []
    for name, d, i in zip(names, datas, idx):
        assert st[i] in (0, 102), (name, st[i])  # (102: the reference's own Q1 stream -- its footer is the input's all the same)
        if cut_footer(container, outs[i]) != K.footer(container, d):
            bad.append((name, offset, cut_footer(container, outs[i]).hex(), K.footer(container, d).hex()))
    assert not bad, (container, mode, len(bad), bad[:6])


# ------------------------------------------------------------------ C1: flate_hip_checksum
@pytest.mark.parametrize("content", K.CONTENTS)
def test_c1_engine_checksum_over_the_case_list(content):
    """Engine.checksum (k_checksum per 65535-byte unit + k_fold_checksum) == zlib, every length of the list, both containers.
    (The buffer is staged at the start of a device allocation: offset 0 only.  The other alignments of k_checksum: C2 and C3.)"""
    eng = engine()
    for n in K.LENGTHS:
        data = K.make(content, n)
        for container in (GZIP, ZLIB):
            got, want = eng.checksum(data, container), K.reference(container, data)
            assert got == want, (content, n, container, hex(got), hex(want))
        assert eng.checksum_combine(GZIP, K.crc32(data[:n // 3]), K.crc32(data[n // 3:]), n - n // 3) == K.crc32(data)


def test_c1_checksum_of_the_longest_buffer_4gib():
    """0xfffffff0 bytes of 0xFF, the longest buffer flate_hip_checksum takes (65537 units and 0xfff0 bytes); one byte more is
    refused"""
    eng = engine()
    n = 0xFFFFFFF0
    data = np.full(n + 1, 0xFF, dtype=np.uint8)
    crc, adler = 0, 1
    for k in range(0, n, 1 << 28):
        piece = data[k:min(k + (1 << 28), n)]
        crc, adler = pyzlib.crc32(piece, crc), pyzlib.adler32(piece, adler)
    v = np.zeros(1, dtype=np.uint32)
    for container, want in ((GZIP, crc), (ZLIB, adler)):
        assert eng._L.flate_hip_checksum(eng._h, data.ctypes.data, n, container, v.ctypes.data) == 0
        assert int(v[0]) == want, (container, hex(int(v[0])), hex(want))
        assert eng._L.flate_hip_checksum(eng._h, data.ctypes.data, n + 1, container, v.ctypes.data) != 0


# ------------------------------------------------------------------ C2: the chunk path, one part per chunk
@pytest.mark.parametrize("container", [GZIP, ZLIB])
@pytest.mark.parametrize("level", [4, 9])
def test_c2_chunk_path_footers(level, container):
    """chunks of at most 65535 bytes at levels 4 and 9: every content x every length of the list up to 65535, at every
    alignment 0..15 of the chunk in the batch's input (padded_batch)"""
    eng = engine()
    cs = K.cases(hi=K.BLOCK)
    assert len(cs) == 17 * len(K.CONTENTS)
    datas, names = [K.make(c, n) for _, c, n in cs], [name for name, _, _ in cs]
    for offset in K.OFFSETS:
        check_footers(eng, datas, names, container, level, offset)


# ------------------------------------------------------------------ C3: streams of many blocks
@pytest.mark.parametrize("container", [GZIP, ZLIB])
@pytest.mark.parametrize("mode", [STORE, HUFFMAN])
def test_c3_simple_streams_every_length_and_alignment(mode, container):
    """one store-only / huffman-only stream per content x length up to 65 x 65535 + 1, at every alignment 0..15 of the stream in
    the batch's input: k_checksum per block, the finish kernel's fold with one wave (the batch has fewer than 32 blocks a chunk)"""
    eng = engine()
    cs = K.cases(hi=MID)
    for content in K.CONTENTS:
        sel = [(name, n) for name, c, n in cs if c == content]
        datas, names = [K.make(content, n) for _, n in sel], [name for name, _ in sel]
        for offset in K.OFFSETS:
            check_footers(eng, datas, names, container, mode, offset)


@pytest.mark.parametrize("container", [GZIP, ZLIB])
@pytest.mark.parametrize("mode", [STORE, HUFFMAN])
def test_c3_simple_streams_above_the_middle_lengths(mode, container):
    """1024 x 5552 and 4097 x 65535 + 1 bytes (-1, +0, +1), a stream a call: at least 87 blocks, so the finish kernel folds with
    its sixteen waves"""
    eng = engine()
    for n in K.lengths(lo=MID + 1):
        for content in ("ff", "random", "ff_zero_mid") if n < BIG - 1 else ("ff", "random"):
            check_footers(eng, [K.make(content, n)], ["%s-%d" % (content, n)], container, mode)


@pytest.mark.parametrize("container", [GZIP, ZLIB])
def test_c3_block_counts_around_the_fold(container):
    """block counts 1, 63, 64, 65 and 64 W - 1, 64 W, 64 W + 1 for the W = 16 waves the finish kernel runs with on a stream of
    32 blocks or more; each count with a last block of one byte less than full and with an EMPTY last block (a stream of n
    bytes has n / 65535 + 1 blocks); alone in its call (W = 16 from 32 blocks on) and beside 7 one-byte chunks (W = 1: fewer
    than 32 blocks a chunk)"""
    eng = engine()
    for nb in (1, 63, 64, 65, 64 * 16 - 1, 64 * 16, 64 * 16 + 1):
        for n in (nb * K.BLOCK - 1, (nb - 1) * K.BLOCK):
            for content in ("ff", "random"):
                d = K.make(content, n)
                name = "%s-%d blocks-%d" % (content, nb, n)
                for mode in (STORE, HUFFMAN):
                    check_footers(eng, [d], [name], container, mode)
                    if nb <= 65:
                        check_footers(eng, [b"x"] * 7 + [d], ["x"] * 7 + [name], container, mode)


@pytest.mark.parametrize("container", [GZIP, ZLIB])
def test_c3_level6_whole_streams(container):
    """level 6, one stream each: the lengths above 65535 up to 65 x 65535 (whole-stream passes; their checksum is the same
    per-block parts and the same fold)"""
    eng = engine()
    cs = [c for c in K.cases(lo=K.BLOCK + 1, hi=65 * K.BLOCK)]
    assert len(cs) == 10 * len(K.CONTENTS)
    check_footers(eng, [K.make(c, n) for _, c, n in cs], [name for name, _, _ in cs], container, 6)


# ------------------------------------------------------------------ C4: footers of streams written flush by flush
PIECES = (1, 65520, 65521, 65535, 65536)


@pytest.mark.parametrize("container", [GZIP, ZLIB])
@pytest.mark.parametrize("mode", [STORE, HUFFMAN, 6])
def test_c4_python_compressor_flush_by_flush(mode, container):
    """all-0xFF data in pieces of 1, 65520, 65521, 65535, 65536 bytes, three rounds, a flush after each: Engine.checksum per piece,
    flate_hip_checksum_combine between them"""
    import io
    from flate_amd import api
    eng = engine()
    w = io.BytesIO()
    c = api._Compressor(container, mode, w, eng)
    total = 0
    for n in PIECES * 3:
        c.write(b"\xff" * n)
        c.flush()
        total += n
    c.finish()
    assert cut_footer(container, w.getvalue()) == K.footer(container, b"\xff" * total)


def test_c4_cpp_compressor_flush_by_flush():
    """the same through flate_amd/host/flate.hpp's CompressorImpl (tests/host_cpp/test_checksum_flush.cpp, built as
    tests/test_host_cpp.py builds its program)"""
    engine()
    from flate_amd import _capi
    src = os.path.join(ROOT, "tests", "host_cpp", "test_checksum_flush.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_checksum_flush")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, src, "-L" + os.path.dirname(_capi.LIB_PATH), "-lflate_hip",
                    "-Wl,-rpath," + os.path.dirname(_capi.LIB_PATH)], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "checksum flush ok" in r.stdout, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(("gzip ", "zlib "))]
    assert len(lines) == 8
    for name, total, foot in lines:
        assert bytes.fromhex(foot) == K.footer(GZIP if name == "gzip" else ZLIB, b"\xff" * int(total)), (name, total, foot)


# ------------------------------------------------------------------ C5: the resumable deflater
def deflater_footer(eng, container, mode, pieces, op):
    """feed the pieces (each FLUSH or MORE, the last FINISH); returns the last bytes of the stream"""
    from flate_amd._capi import FEED_FINISH, ST_NEED_OUTPUT
    d = eng.deflater(1, container, mode)
    tail = b""
    try:
        for k, p in enumerate(pieces):
            last = k == len(pieces) - 1
            outs, st, cons = d.feed([p], op=FEED_FINISH if last else op)
            assert cons[0] == len(p)
            tail = (tail + outs[0])[-16:]
            while st[0] == ST_NEED_OUTPUT:
                outs, st, _ = d.feed([b""], op=0)
                tail = (tail + outs[0])[-16:]
            assert st[0] in (0, 104), st
        assert st[0] == 0
    finally:
        d.close()
    return tail


@pytest.mark.parametrize("container", [GZIP, ZLIB])
@pytest.mark.parametrize("mode", [STORE, HUFFMAN])
def test_c5_deflater_pieces(mode, container):
    """the piece sizes of C4, all 0xFF and random, as FLUSH feeds and as MORE feeds: the running checksum of the deflater"""
    from flate_amd._capi import FEED_FLUSH, FEED_MORE
    eng = engine()
    for content in ("ff", "random"):
        pieces = [K.make(content, n, seed=k) for k, n in enumerate(PIECES * 3)] + [b""]
        for op in (FEED_FLUSH, FEED_MORE):
            got = deflater_footer(eng, container, mode, pieces, op)
            assert cut_footer(container, got) == K.footer(container, b"".join(pieces)), (content, op)


@pytest.mark.parametrize("container", [GZIP, ZLIB])
def test_c5_deflater_stream_past_4gib(container):
    """all 0xFF, 17 feeds of 256 MiB (huffman-only: a bit a byte comes back): the 64-bit total and the running checksum past 2^32
    bytes; the footer's reference is zlib run piece by piece"""
    eng = engine()
    piece = b"\xff" * (256 << 20)
    crc, adler = 0, 1
    for _ in range(17):
        crc, adler = pyzlib.crc32(piece, crc), pyzlib.adler32(piece, adler)
    total = 17 * len(piece)
    want = (crc.to_bytes(4, "little") + (total & 0xFFFFFFFF).to_bytes(4, "little")) if container == GZIP else adler.to_bytes(4, "big")
    got = deflater_footer(eng, container, HUFFMAN, [piece] * 17 + [b""], 0)
    assert cut_footer(container, got) == want


# ------------------------------------------------------------------ D1, D2, D3: one-shot inflate
def inflate_cases(eng, container, items, slot_offset):
    """items: (name, stream, plain).  One flate_hip_decompress_batch call on host buffers with an out_off array of its own
    (Engine.decompress_many rounds every slot to 8 bytes; the library takes any slot start).  The library stages the slots at
    out_off[i] - out_off[0] from the start of a device allocation (256-byte aligned), so the first slot of a call is always at
    offset 0: it is `slot_offset` bytes longer than a multiple of 16, every slot behind it a multiple of 16, and so every slot
    behind the first starts `slot_offset` bytes past a multiple of 16 in the memory the kernels write and sum -- asserted on the
    out_off array that is passed.  Returns the outputs and the statuses."""
    from flate_amd._capi import MEM_HOST
    eng._sync_env()
    n = len(items)
    caps = [((len(p) + 15) & ~15) + 16 for _, _, p in items]
    caps[0] += slot_offset
    lens = np.array([len(s) for _, s, _ in items], dtype=np.uint64)
    in_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=in_off[1:])
    out_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.array(caps, dtype=np.uint64), out=out_off[1:])
    for k in range(1, n):
        assert (int(out_off[k]) - int(out_off[0])) % 16 == slot_offset
    blob = np.frombuffer(b"".join(s for _, s, _ in items), dtype=np.uint8)
    out = np.zeros(int(out_off[-1]) + 64, dtype=np.uint8)
    out_len, status, consumed = np.zeros(n, dtype=np.uint64), np.full(n, -99, dtype=np.int32), np.zeros(n, dtype=np.uint64)
    rc = eng._L.flate_hip_decompress_batch(eng._h, blob.ctypes.data, in_off.ctypes.data, n, container, 0, out.ctypes.data,
                                           out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data, consumed.ctypes.data,
                                           MEM_HOST)
    eng._check(rc, "flate_hip_decompress_batch")
    outs = [out[int(out_off[i]): int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
    st = [int(v) for v in status]
    for (name, s, _), u, v in zip(items, consumed, st):
        assert v != 0 or int(u) == len(s), name
    return outs, st


def batches(items, n_max=24, byte_max=48 << 20):
    """at most 24 streams a call: the span path takes at most 32 long streams"""
    out, cur, size = [], [], 0
    for it in items:
        if cur and (len(cur) >= n_max or size + len(it[2]) > byte_max):
            out.append(cur)
            cur, size = [], 0
        cur.append(it)
        size += len(it[2])
    if cur:
        out.append(cur)
    return out


def inflate_case_list(container):
    """The case list of a path: everything up to 1024 x 5552 + 1 bytes, and 4097 x 65535 + 1 bytes (+-1).  At that last size
    (268 MB a stream, one wave in D1) all 0xFF and random go through both containers, the other four contents through gzip only,
    for time: CRC-32 is where a lane's share is moved by x^(8 x the bytes behind it) -- what `one_first` isolates for lane 0 --,
    and Adler-32's term for the bytes behind a share is linear in the content, which 0xFF (its largest sums) and random cover."""
    return K.cases(hi=K.FP_THREADS * 5552 + 1) + K.cases(lo=BIG - 1, contents=K.CONTENTS if container == GZIP else ("ff", "random"))


@pytest.mark.parametrize("container", [GZIP, ZLIB])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_d123_stored_streams_right_and_wrong_footer(path, container, monkeypatch):
    """Every case as a stream of stored blocks (1:1, any content), through one path at a time: the right footer gives Ok and the
    bytes, a flipped footer bit the Wrong... status.  D2 / D3: the Ok streams of a call were all finished by the path under test
    -- inflate_paths() shows none handed on -- and with a wrong footer none was (D2: all handed on: it saw the mismatch itself).

    Output slot offsets (inflate_cases): every case of up to 1024 x 5552 + 1 bytes with its slot at each of the offsets 0..15.
    The cases of 268 MB each at ONE offset, a different one per case and every one of 1..15 among them (sixteen times 268 MB per
    case and path is minutes of one-wave decoding; what depends on the offset -- the head and tail handling of a share -- does
    not depend on the length).  The wrong-footer streams: one offset a call, rotating.

    No case is left out for a path: k_inflate_par with FLATE_HIP_INFLATE_PAR=1 takes every stream.  The span path leaves a CALL
    in which it finds no place to cut to the other kernels whole (alone in their calls, the stored streams of up to 65537 bytes
    are all handed on), so every call of the D3 runs carries one stream of seven stored blocks beside its cases; then the span
    path finishes all of them, the empty stream included."""
    choose(monkeypatch, path)
    eng = engine()
    kind = path[:2]
    items = []
    for name, c, n in inflate_case_list(container):
        plain = K.make(c, n)
        items.append((name, K.stored_stream(plain), plain))
    plain = K.make("random", 6 * K.BLOCK + 5)
    companion = ("companion", K.stored_stream(plain), plain)
    filler = ("filler", K.stored_stream(b"\xff"), b"\xff")
    n_big = 0
    for call, part in enumerate(batches(items)):
        big = len(part[0][2]) >= BIG - 1 and len(part) == 1
        if big:  # one offset per call (a call holds one such case)
            n_big += 1
            offsets = [1 + (n_big - 1) % 15]
        else:
            offsets = list(K.OFFSETS)
        part = [filler] + part  # (the first slot of a call is at offset 0 whatever its out_off: a one-byte case goes there)
        if kind == "D3":
            part = part + [companion]
        good = [(name, K.wrap(container, raw, plain), plain) for name, raw, plain in part]
        for slot_offset in offsets:
            outs, st = inflate_cases(eng, container, good, slot_offset)
            paths = eng.inflate_paths()
            for (name, _, plain), o, s in zip(good, outs, st):
                assert s == 0 and o == plain, (path, name, slot_offset, s, len(o))
            if kind == "D2":
                assert paths["par_handed_on"] == 0 and paths["par_done"] == len(good), (path, slot_offset, paths, [g[0] for g in good])
            elif kind == "D3":
                assert paths["span_handed_on"] == 0 and paths["span_done"] == len(good), (path, slot_offset, paths, [g[0] for g in good])
            else:
                assert paths["par_done"] == paths["span_done"] == 0, (path, paths)
        bad = [(name, K.wrap(container, raw, plain, flip_bit=(7 * k + call) % 32), plain) for k, (name, raw, plain) in enumerate(part)]
        outs, st = inflate_cases(eng, container, bad, offsets[call % len(offsets)])
        paths = eng.inflate_paths()
        for (name, _, _), s in zip(bad, st):
            assert s == WRONG[container], (path, name, s)
        if kind == "D2":
            assert paths["par_done"] == 0 and paths["par_handed_on"] == len(bad), (path, paths)
        elif kind == "D3":
            assert paths["span_done"] == 0, (path, paths)
    assert n_big == (18 if container == GZIP else 6)


@pytest.mark.parametrize("path", ["D2-k_inflate_par", "D3-spans-symbols"])
def test_d23_huffman_streams_are_finished_by_the_path(path, monkeypatch):
    """the same with Huffman blocks (zlib.compressobj output, raw) where a path's decode differs from its copy of stored bytes:
    random bytes and the single-odd-byte contents at the lengths above 65535, gzip and zlib"""
    choose(monkeypatch, path)
    eng = engine()
    for container in (GZIP, ZLIB):
        items = []
        for name, c, n in K.cases(lo=K.BLOCK + 1, hi=65 * K.BLOCK, contents=("random", "one_last", "ff_zero_mid")):
            plain = K.make(c, n)
            co = pyzlib.compressobj(1, pyzlib.DEFLATED, -15)
            items.append((name, co.compress(plain) + co.flush(), plain))
        for part in batches(items):
            good = [(name, K.wrap(container, raw, plain), plain) for name, raw, plain in part]
            outs, st = inflate_cases(eng, container, good, 0)
            paths = eng.inflate_paths()
            for (name, _, plain), o, s in zip(good, outs, st):
                assert s == 0 and o == plain, (path, name, s)
            # (what the path hands on here it hands on for the STREAM's sake -- a stream it cannot cut, more than 32 bytes out of
            # a byte in -- never for its checksum: with a right footer and a decode that ran through, nothing may be handed on)
            done, handed = (paths["par_done"], paths["par_handed_on"]) if path.startswith("D2") else (paths["span_done"], paths["span_handed_on"])
            print(path, container, [g[0] for g in good], paths)
            assert done + handed == len(good)
            bad = [(name, K.wrap(container, raw, plain, flip_bit=k % 32), plain) for k, (name, raw, plain) in enumerate(part)]
            outs, st = inflate_cases(eng, container, bad, 0)
            assert st == [WRONG[container]] * len(bad)
            p2 = eng.inflate_paths()
            # a stream the path finished with the right footer is handed on with the wrong one, and only for that
            if path.startswith("D2"):
                assert p2["par_done"] == 0 and p2["par_handed_on"] == len(bad)
            else:
                assert p2["span_done"] == 0
            assert handed == 0, (path, container, paths)


# ------------------------------------------------------------------ D4: the resumable inflater, one fold per feed
def feed_cuts(plain, counts):
    """a stored stream of `plain` and the input positions behind which exactly counts[0], counts[0] + counts[1], ... plain bytes
    have been seen (five header bytes before every 65535)"""
    cuts, done = [], 0
    for c in counts:
        done += c
        assert done <= len(plain)
        cuts.append(done + 5 * ((done + K.BLOCK - 1) // K.BLOCK if done else 0))
    return cuts


@pytest.mark.parametrize("container", [GZIP, ZLIB])
@pytest.mark.parametrize("content", ["ff", "random"])
def test_d4_inflater_per_feed_counts(content, container):
    """a stream of stored blocks fed in pieces that end right behind 1, 64 x 5552 - 1, 64 x 5552 + 1, 65521, 65536, ... plain bytes:
    every feed's output count (asserted) is the n of one fold; the last feed brings the footer: right -> Ok, one bit flipped ->
    Wrong..."""
    eng = engine()
    counts = [1, 64 * 5552 - 1, 64 * 5552 + 1, 65521, 65536, 64 * 5552, 1, 5552, 65535, 5553, 2]
    plain = K.make(content, sum(counts) + 777)
    raw = K.stored_stream(plain)
    hdr = len(K.GZ_HEADER if container == GZIP else K.ZL_HEADER)
    cuts = [hdr + c for c in feed_cuts(plain, counts)]
    for flip in (None, 13):
        stream = K.wrap(container, raw, plain, flip_bit=flip)
        inf = eng.inflater(1, container)
        try:
            pos, got, lens = 0, bytearray(), []
            for cut in cuts + [len(stream)]:
                final = cut == len(stream)
                o, s, c = inf.feed([stream[pos:cut]], final=final, caps=1 << 20)
                assert c[0] == cut - pos - (4 if final and flip is not None and container == GZIP else 0), (cut, c)  # (a wrong CRC-32 stops in front of ISIZE)
                got += o[0]
                lens.append(len(o[0]))
                pos = cut
                assert s[0] == (104 if not final else (0 if flip is None else WRONG[container])), (cut, s)
            assert lens == counts + [777], lens
            assert bytes(got) == plain
        finally:
            inf.close()


@pytest.mark.parametrize("content", ["ff", "random"])
def test_d4_inflater_slot_of_1gib(content):
    """one feed into a slot of 1 GiB that it fills exactly (a fold over 2^30 bytes: a lane's share is 16 MiB), gzip and zlib"""
    eng = engine()
    n = 1 << 30
    plain = K.make(content, n)
    raw = K.stored_stream(plain)
    for container in (GZIP, ZLIB):
        for flip in (None, 31):
            inf = eng.inflater(1, container)
            try:
                o, s, c = inf.feed([K.wrap(container, raw, plain, flip_bit=flip)], final=True, caps=n)
                assert s[0] == (0 if flip is None else WRONG[container]), (container, flip, s)
                assert len(o[0]) == n and (flip is not None or o[0] == plain)
            finally:
                inf.close()


@pytest.mark.parametrize("container", [GZIP, ZLIB])
def test_d4_inflater_one_feed_past_4gib(container):
    """tests/_big_member.py's member (4.36 GiB of 'a'): 4 KiB of it first (so that the running checksum is no longer the empty
    one), then all the rest in ONE feed with a slot that holds it: the fold of a feed whose n has more than 32 bits (x^(8n),
    n % 65521 times the running a, the bytes behind a lane's share)"""
    import _big_inflate_job as J
    eng = engine()
    n = B.output_size(GROUPS_4G)
    stream = J.member(container, GROUPS_4G)
    inf = eng.inflater(1, container)
    try:
        o, s, c = inf.feed([stream[:4096]], final=False, caps=1 << 20)
        assert s[0] == 104 and c[0] == 4096 and 0 < len(o[0]) < (1 << 20) and o[0].count(b"a") == len(o[0]), (s, c, len(o[0]))
        first = len(o[0])
        assert n - first > 1 << 32
        o, s, c = inf.feed([stream[4096:]], final=True, caps=n + 64)
        assert s[0] == 0, s
        assert len(o[0]) == n - first and o[0].count(b"a") == n - first
    finally:
        inf.close()


# ------------------------------------------------------------------ D5: a member that inflates to more than 4 GiB in one call
GROUPS_256M = (256 << 20) // 2064
GROUPS_4G = ((1 << 32) * 64 // 63) // 2064 + 40  # output_size just over 2^32 x 64 / 63: lane 0 of 64 has 2^32 bytes behind it
D5_KNOBS = {"default": {}, "k_inflate": PATHS["D1-k_inflate-ring32768"], "k_inflate_par": PATHS["D2-k_inflate_par"]}


def big_inflate(container, groups, knobs, timeout):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_big_inflate_job.py"), str(container), str(groups)],
                       capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(container, groups, knobs, res)
    return res


@pytest.mark.parametrize("container", [GZIP, ZLIB])
@pytest.mark.parametrize("knobs", sorted(D5_KNOBS))
def test_d5_member_of_256_mib_in_one_call(knobs, container):
    """the member of tests/_big_member.py at 256 MiB of output, one decompress call with an explicit slot: the timing run of the
    4 GiB case below, and the same checks at a size every path takes"""
    engine()
    res = big_inflate(container, GROUPS_256M, D5_KNOBS[knobs], 600)
    assert res["status"] == 0 and res["out_len"] == B.output_size(GROUPS_256M) and res["all_a"], res
    if knobs == "k_inflate_par":
        assert res["paths"]["par_handed_on"] == 0 and res["paths"]["par_done"] == 1, res


# seconds of the 256 MiB call on an MI355X (gzip / zlib), as the child reports them for the call alone: default 1.83 / 1.85 (the
# span path cannot cut a member of one block and hands it on; k_inflate_par finishes it), k_inflate 2.45 / 2.32, k_inflate_par
# 1.86 / 1.84.  Times 17.45 for 4.36 GiB: 32, 43 and 32 seconds -- under two minutes, so all three run at full size (measured
# then: 33, 50 and 33).  The full-size call may take three times the extrapolation.  (The child also builds the member, makes an
# engine and checks 4.36 GiB of output in slices: its own time limit is there to end a hang, it is not the bound.)
D5_CALL_LIMIT = {"default": 3 * 32, "k_inflate": 3 * 43, "k_inflate_par": 3 * 32}
D5_CHILD_LIMIT = 600


@pytest.mark.parametrize("container", [GZIP, ZLIB])
@pytest.mark.parametrize("knobs", sorted(D5_KNOBS))
def test_d5_member_past_4gib_in_one_call(knobs, container):
    """output_size just over 2^32 x 64 / 63 (4.36 GiB of 'a' from 27.5 MB), ONE decompress call with an explicit slot; knobs at
    their defaults, forced to k_inflate (lane 0 of 64 has more than 2^32 bytes behind its share) and to k_inflate_par (thread 0 of
    1024 likewise): Ok, out_len, every byte an 'a' (checked in slices in the child process).  The zlib member: Adler-32 with
    n % 65521 and a 64-bit count of the bytes behind a lane's share.
    Before fl_crc_xpow8n wrapped its table index the gzip member came back WrongGzipChecksum from k_inflate, and k_inflate_par
    handed it on to k_inflate, which then said the same (the default knobs end in k_inflate_par too: see above)."""
    engine()
    n = B.output_size(GROUPS_4G)
    assert n > (1 << 32) * 64 // 63 and n * 1023 // 1024 > 1 << 32
    res = big_inflate(container, GROUPS_4G, D5_KNOBS[knobs], D5_CHILD_LIMIT)
    assert res["status"] == 0 and res["out_len"] == n and res["all_a"], res
    assert res["seconds"] <= D5_CALL_LIMIT[knobs], res
    if knobs != "k_inflate":
        assert res["paths"]["par_handed_on"] == 0 and res["paths"]["par_done"] == 1, res
