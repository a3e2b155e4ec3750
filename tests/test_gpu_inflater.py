"""GPU tests of the resumable inflater (flate_hip_inflater_*, k_inflater): fed piece by piece, every stream ends with the
status, the output and the consumed count of the one-shot flate_hip_decompress_batch of its whole input (and the
oracle's status)."""
import io
import random
import zlib as pyzlib

import numpy as np
import pytest

import _big_member as B
import _deflate_synth as S
import _inflate_edge_cases as E
import _oracle as O
from conftest import golden
from gpu_util import engine
from test_oracle_inflate_pins import FUZZ

pytestmark = pytest.mark.gpu

NEED_INPUT, NEED_OUTPUT = 104, 105


def one_shot(eng, streams, container, flags=0):
    caps = [max(1 << 16, len(s) * 1100 + 1024) for s in streams]
    return eng.decompress_many(streams, container, flags, caps)


def splits(n):
    if n <= 12000:
        return list(range(n + 1))
    return sorted(set(range(300)) | set(range(n - 300, n + 1)) | set(range(0, n, max(1, n // 600))))


def run_two_feeds(eng, data, container, flags=0):
    """one stream per split point k: data[:k] (not final), then the unabsorbed rest (final).  Against the one-shot
    decode of the whole input: the same status always; on success the same output and total consumed.  On an error
    the output of the one-shot decode comes first and, but for EndOfStream, is all of it (a stream that ends inside a
    stored block has handed out the part of the body it had), and the total consumed is the one-shot's -- or more,
    when the first feed already absorbed the bytes of the unit that failed (NeedInput means all input absorbed)."""
    ks = splits(len(data))
    want, wst, wcons = one_shot(eng, [data], container, flags)
    ost, oout, _ = O.decompress(data, container, flags=flags)
    assert O.STATUS[wst[0]] == ost
    if wst[0] == 0:
        assert want[0] == oout
    cap = len(want[0]) + 1024
    inf = eng.inflater(len(ks), container, flags)
    try:
        o1, s1, c1 = inf.feed([data[:k] for k in ks], final=False, caps=cap)
        o2, s2, c2 = inf.feed([data[c:] for c in c1], final=True, caps=cap)
    finally:
        inf.close()
    for j, k in enumerate(ks):
        assert s1[j] in (NEED_INPUT, wst[0]), (k, s1[j])
        assert s2[j] == wst[0], (k, s2[j], wst[0])
        got = o1[j] + o2[j]
        if wst[0] == 0:
            assert got == want[0], k
            assert c1[j] + c2[j] == wcons[0], k
        else:
            assert got[:len(want[0])] == want[0], k
            if wst[0] != 1:
                assert got == want[0], k
            absorbed = c1[j] if s1[j] == NEED_INPUT else 0
            assert c1[j] + c2[j] == max(absorbed, wcons[0]), (k, c1[j], c2[j], wcons[0])
    return wst[0]


TEXT = golden("rfc1951.txt")[:8000]


@pytest.mark.parametrize("container", [0, 1, 2])
@pytest.mark.parametrize("mode", [4, 6, 9, O.HUFFMAN, O.STORE])
def test_every_split_point_rfc1951(container, mode):
    eng = engine()
    data = O.compress(TEXT, container, mode)
    assert run_two_feeds(eng, data, container) == 0


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_every_split_point_edge_cases(name):
    eng = engine()
    data = E.CASES[name]
    st = run_two_feeds(eng, data, 0)
    want_st, _, _ = O.decompress(data, 0)
    assert O.STATUS[st] == want_st


@pytest.mark.parametrize("name", S.SMALL)
def test_every_split_point_synth_cases(name):
    """tests/_deflate_synth.py, the cases of at most 12000 bytes (splits() is exhaustive): codes at the tables' edges, 48-bit
    tokens, degenerate trees, header fields at their limits -- the split points inside the longest header among them --, tiny
    blocks, and the streams cut inside headers and long tokens.  The status is the oracle's, by the name written next to the
    case; the bytes are the generator's."""
    eng = engine()
    data, want = S.CASES[name]
    assert len(data) <= 12000
    st = run_two_feeds(eng, data, 0)
    assert O.STATUS[st] == (S.INFO[name]["error"] or "Ok")
    if want is not None:
        assert one_shot(eng, [data], 0)[0][0] == want


@pytest.mark.parametrize("flags", [0, 1])
def test_synth_long_streams_in_random_pieces(flags):
    """Families 5 (thousands of tiny blocks) and 8 (big random streams), and the random sweep: 8 copies of every long stream and
    one of every random stream, each in four pieces cut at random places, into slots of random sizes.  Reference-strict
    (flags = 1): the streams with a repeat across the two length lists end with InvalidDynamicBlockHeader, as the oracle says."""
    eng = engine()
    info = []
    items = [(n,) + S.CASES[n] + (S.INFO[n]["q6"],) for n in S.LARGE + ["tiny_blocks_60"] for _ in range(8)]
    items += [("seed %d" % (6000 + k), s, want, q6) for k, ((s, want), (q6, _)) in
              enumerate(zip(S.random_streams(6000, 100, info), info))]
    items.append(("fixed seams",) + E.fixed_seam_stream() + (False,))
    outs, st, used = feed_random_pieces(eng, [it[1] for it in items], random.Random(11 + flags), flags=flags)
    n_q6 = 0
    for (name, stream, want, q6), o, s_, u in zip(items, outs, st, used):
        wname = O.decompress(stream, 0, flags, cap=len(want) + 8)[0]
        assert wname == ("InvalidDynamicBlockHeader" if flags and q6 else "Ok"), name
        assert O.STATUS.get(s_, s_) == wname, (name, s_, wname)
        if wname == "Ok":
            assert o == want and u == len(stream), name
        n_q6 += wname != "Ok"
    assert (n_q6 > 0) == (flags == 1)


@pytest.mark.parametrize("flags", [0, 1])
def test_every_split_point_fuzz_corpus(flags):
    eng = engine()
    for name, err, _ in FUZZ:
        d = golden("fuzz", name + ".input")
        st = run_two_feeds(eng, d, 0, flags)
        assert O.STATUS[st] == (err or "Ok"), name
        assert O.STATUS[st] == O.decompress(d, 0, flags=flags)[0], name


def gzip_with_fields(payload, fextra=b"", fname=None, fcomment=None, fhcrc=False):
    flg = (4 if fextra else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | (2 if fhcrc else 0)
    h = bytes([0x1F, 0x8B, 8, flg, 0, 0, 0, 0, 0, 3])
    if fextra:
        h += len(fextra).to_bytes(2, "little") + fextra
    if fname is not None:
        h += fname + b"\0"
    if fcomment is not None:
        h += fcomment + b"\0"
    if fhcrc:
        h += (pyzlib.crc32(h) & 0xFFFF).to_bytes(2, "little")
    co = pyzlib.compressobj(6, pyzlib.DEFLATED, -15)
    body = co.compress(payload) + co.flush()
    return h + body + pyzlib.crc32(payload).to_bytes(4, "little") + (len(payload) & 0xFFFFFFFF).to_bytes(4, "little")


def short_streams():
    p = TEXT[:700]
    g = [gzip_with_fields(p, fextra=b"xy" * 40, fname=b"name.txt", fcomment=b"a comment", fhcrc=True),
         gzip_with_fields(p, fname=b"n"), gzip_with_fields(b""), gzip_with_fields(p, fextra=b"\0", fhcrc=True),
         O.compress(p, 1, 6), O.compress(p, 1, O.STORE), O.compress(p, 1, O.HUFFMAN)]
    return g


def feed_bytewise(eng, streams, container, caps=None, step=1):
    n = len(streams)
    inf = eng.inflater(n, container)
    pos, outs, st = [0] * n, [b""] * n, [NEED_INPUT] * n
    try:
        while any(s in (NEED_INPUT, NEED_OUTPUT) for s in st):
            pieces, fin = [], []
            for i in range(n):
                if st[i] in (NEED_INPUT, NEED_OUTPUT):
                    pieces.append(streams[i][pos[i]:pos[i] + step])
                    fin.append(pos[i] + step >= len(streams[i]))
                else:
                    pieces.append(None)
                    fin.append(False)
            o, s, c = inf.feed(pieces, final=fin, caps=caps)
            for i in range(n):
                if pieces[i] is not None:
                    outs[i] += o[i]
                    pos[i] += c[i]
                    st[i] = s[i]
    finally:
        inf.close()
    return outs, st, pos


def test_one_byte_pieces_with_gzip_header_fields():
    eng = engine()
    streams = short_streams()
    want, wst, wcons = one_shot(eng, streams, 1)
    assert wst == [0] * len(streams)
    outs, st, used = feed_bytewise(eng, streams, 1)
    assert st == wst and outs == want and used == wcons
    for s, o in zip(streams, outs):
        assert o == pyzlib.decompress(s, 31)


@pytest.mark.parametrize("cap", [258, 300, 1000])
def test_output_bound(cap):
    eng = engine()
    streams = [O.compress(TEXT, c, m) for c in (1,) for m in (4, 6, 9, O.HUFFMAN, O.STORE)] + short_streams()
    want, wst, wcons = one_shot(eng, streams, 1)
    outs, st, used = feed_bytewise(eng, streams, 1, caps=cap, step=1 << 30)  # whole input, small slots
    assert st == wst and outs == want and used == wcons
    outs, st, used = feed_bytewise(eng, streams[5:], 1, caps=cap, step=1)  # and 1-byte pieces
    assert st == wst[5:] and outs == want[5:] and used == wcons[5:]


def test_truncated_sticky_skipped_and_members():
    eng = engine()
    full = O.compress(TEXT, 1, 6)
    inf = eng.inflater(4, 1)
    try:
        # 0: truncated; 1: skipped at first; 2: an error; 3: two concatenated members
        bad = bytearray(full)
        bad[12] ^= 0xFF
        two = full + O.compress(TEXT[:3000], 1, 9)
        o, s, c = inf.feed([full[:-5], None, bytes(bad), two[:400]], final=[False, False, True, False], caps=1 << 16)
        assert s[0] == NEED_INPUT and c[0] == len(full) - 5
        assert s[1] == NEED_INPUT and c[1] == 0 and o[1] == b""
        err = s[2]
        assert err in range(1, 15)
        assert O.STATUS[err] == O.decompress(bytes(bad), 1)[0]
        assert s[3] == NEED_INPUT and c[3] == 400
        out3 = o[3]
        o, s2, c2 = inf.feed([b"", full[:100], b"more bytes", two[400:]], final=[True, False, True, True], caps=1 << 16)
        assert s2[0] == 1  # EndOfStream
        assert s2[2] == err and c2[2] == 0 and o[2] == b""  # sticky: nothing absorbed
        assert s2[3] == 0 and 400 + c2[3] == len(full)
        out3 += o[3]
        assert out3 == TEXT
        assert s2[1] == NEED_INPUT and c2[1] == 100
        o1 = o[1]
        o, s3, c3 = inf.feed([None, full[100:], None, two[len(full):]], final=[False, True, False, True], caps=1 << 16)
        assert s3[3] == 0 and c3[3] == 0 and o[3] == b""  # complete: nothing more until reset
        assert s3[1] == 0 and o1 + o[1] == TEXT
        assert s3[0] == 1 and s3[2] == err  # skipped streams keep their status
        inf.reset([3])
        o, s4, c4 = inf.feed([None, None, None, two[len(full):]], final=[False, False, False, True], caps=1 << 16)
        assert s4[3] == 0 and c4[3] == len(two) - len(full) and o[3] == TEXT[:3000]
    finally:
        inf.close()


def _config2(eng):
    from flate_amd import synth
    n, size = 16385, 65535
    text = synth.text(synth.SEED_TEXT, n * size).tobytes()
    chunks = [text[i * size:(i + 1) * size] for i in range(n)]
    comp, st = eng.compress_many(chunks, O.RAW, 6)
    assert st == [0] * n
    return chunks, comp


def feed_random_pieces(eng, comp, rng, cuts=3, container=0, flags=0):
    """every stream in cuts + 1 pieces cut at random places, into output slots of random sizes: a piece that is absorbed gives way
    to the next, the last one is final.  Returns (outputs, statuses, consumed bytes in all)."""
    n = len(comp)
    where = [sorted(rng.randint(0, len(c)) for _ in range(cuts)) for c in comp]
    pieces = [[c[a:b] for a, b in zip([0] + k, k + [len(c)])] for c, k in zip(comp, where)]
    inf = eng.inflater(n, container, flags)
    outs = [[] for _ in range(n)]
    which, rest = [0] * n, [p[0] for p in pieces]
    st, used = [NEED_INPUT] * n, [0] * n
    try:
        while any(s in (NEED_INPUT, NEED_OUTPUT) for s in st):
            for i in range(n):  # a piece that is absorbed gives way to the next
                if st[i] == NEED_INPUT and not rest[i] and which[i] < cuts:
                    which[i] += 1
                    rest[i] = pieces[i][which[i]]
            live = [s in (NEED_INPUT, NEED_OUTPUT) for s in st]
            fin = [which[i] == cuts for i in range(n)]
            caps = [rng.randint(258, 70000) for _ in range(n)]
            o, s, c = inf.feed([rest[i] if live[i] else None for i in range(n)], final=fin, caps=caps)
            for i in range(n):
                if live[i]:
                    outs[i].append(o[i])
                    rest[i] = rest[i][c[i]:]
                    used[i] += c[i]
                    st[i] = s[i]
    finally:
        inf.close()
    return [b"".join(o) for o in outs], st, used


def test_scale_config2_four_random_pieces():
    eng = engine()
    chunks, comp = _config2(eng)
    n = len(chunks)
    outs, st, _ = feed_random_pieces(eng, comp, random.Random(7))
    assert st == [0] * n
    for i in range(n):
        assert outs[i] == chunks[i], i


def test_scale_config2_device_memory():
    import torch
    eng = engine()
    chunks, comp = _config2(eng)
    n = len(chunks)
    rng = random.Random(11)
    cuts = [sorted(rng.randint(0, len(c)) for _ in range(3)) for c in comp]
    dev = torch.device("cuda", eng.device)
    stream = torch.cuda.Stream(dev)
    inf = eng.inflater(n, 0)
    keep, results = [], []
    slot = 1 << 16
    eng.set_stream(stream.cuda_stream)
    eng.set_sync(0)
    try:
        with torch.cuda.stream(stream):
            out_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * slot
            for f in range(4):
                ps = [c[([0] + k)[f]:(k + [len(c)])[f]] for c, k in zip(comp, cuts)]
                off = np.zeros(n + 1, dtype=np.uint64)
                np.cumsum([len(p) for p in ps], out=off[1:])
                blob = np.frombuffer(b"".join(ps) or b"\0", dtype=np.uint8)
                d_in = torch.from_numpy(blob.copy()).to(dev)
                d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
                d_fin = torch.full((n,), 1 if f == 3 else 0, dtype=torch.uint8, device=dev)
                d_out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
                d_len = torch.empty(n, dtype=torch.int64, device=dev)
                d_cons = torch.empty(n, dtype=torch.int64, device=dev)
                d_st = torch.empty(n, dtype=torch.int32, device=dev)
                eng.inflater_feed_device(inf, d_in.data_ptr(), d_off.data_ptr(), d_fin.data_ptr(), d_out.data_ptr(),
                                         out_off.data_ptr(), d_len.data_ptr(), d_cons.data_ptr(), d_st.data_ptr())
                keep += [d_in, d_off, d_fin]
                results.append((d_out, d_len, d_cons, d_st, ps))
        stream.synchronize()  # the one wait
    finally:
        eng.set_sync(1)
        eng.set_stream(0)
        inf.close()
    got = [[] for _ in range(n)]
    for f, (d_out, d_len, d_cons, d_st, ps) in enumerate(results):
        out, ln, cons, st = d_out.cpu().numpy(), d_len.cpu().numpy(), d_cons.cpu().numpy(), d_st.cpu().numpy()
        # (a member whose last piece is empty completes one feed early; then the last feed absorbs nothing)
        assert (st == 0).all() if f == 3 else np.isin(st, (0, NEED_INPUT)).all(), (f, np.unique(st))
        assert (cons == np.array([len(p) for p in ps])).all()
        for i in range(n):
            got[i].append(out[i * slot: i * slot + int(ln[i])].tobytes())
    for i in range(n):
        assert b"".join(got[i]) == chunks[i], i


def test_bounded_decompressor_past_4gib():
    from flate_amd import gzip
    groups = 2081000
    piece = 1 << 20
    holder = {}

    def on_read(rd):
        d = holder.get("d")
        if d is not None:  # everything read before has been absorbed
            assert not d._in

    rd = B.ChunkReader(B.gzip_chunks(groups), on_read)
    d = gzip.decompressor(rd, piece=piece)
    holder["d"] = d

    class Sink:
        n, crc = 0, 0

        def write(self, b):
            self.n += len(b)
            self.crc = pyzlib.crc32(b, self.crc)

    w = Sink()
    d.decompress(w)  # raises on any error status
    assert w.n == B.output_size(groups) and w.n > 1 << 32
    assert w.crc == B.crc_of_output(groups)
    assert not d.more_input()


@pytest.mark.parametrize("piece", [4096, 1 << 20])
def test_bounded_decompressor_takes_from_the_reader_what_the_stream_needs(piece):
    from flate_amd import gzip, synth

    class CountingReader:
        def __init__(self, data):
            self.data, self.pos = data, 0

        def read(self, n=-1):
            if n is None or n < 0:
                n = len(self.data) - self.pos
            out = self.data[self.pos:self.pos + n]
            self.pos += len(out)
            return out

    parts = [synth.text(synth.SEED_TEXT + 40 + i, n).tobytes() for i, n in enumerate((300000, 10, 70000))]
    members = []
    for part in parts:
        c = io.BytesIO()
        gzip.compress(io.BytesIO(part), c, gzip.Options())
        members.append(c.getvalue())
    blob = b"".join(members) + bytes(8 << 20)
    rd = CountingReader(blob)
    d = gzip.decompressor(rd, piece=piece)
    got = []
    for i in range(3):
        pieces = []
        while True:
            buf = d.next()
            if buf is None:
                break
            assert len(buf) <= 65536
            pieces.append(buf)
        got.append(b"".join(pieces))
        if i < 2:
            assert d.more_input()
            d.reset()
    assert got == parts
    assert rd.pos <= len(b"".join(members)) + piece
    # a truncated stream is EndOfStream once the reader has nothing more
    from flate_amd.api import EndOfStream
    with pytest.raises(EndOfStream):
        gzip.decompressor(io.BytesIO(members[0][:-3]), piece=piece).read()


def test_host_feed_leaves_the_rest_of_every_slot():
    """host memory, more than 16 streams: only out_len[i] bytes of a slot are written"""
    from flate_amd import _capi
    eng = engine()
    n, cap = 20, 4096
    streams = [O.compress(TEXT[:100 * (i + 1)], 0, 6) for i in range(n)]
    inf = eng.inflater(n, 0)
    try:
        in_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in streams], out=in_off[1:])
        blob = np.frombuffer(b"".join(streams), dtype=np.uint8)
        fin = np.ones(n, dtype=np.uint8)
        out_off = np.arange(n + 1, dtype=np.uint64) * cap
        out = np.full(n * cap, 0xAB, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        cons = np.zeros(n, dtype=np.uint64)
        st = np.zeros(n, dtype=np.int32)
        rc = eng._L.flate_hip_inflater_feed(eng._h, inf._s, blob.ctypes.data, in_off.ctypes.data, fin.ctypes.data,
                                            out.ctypes.data, out_off.ctypes.data, out_len.ctypes.data,
                                            cons.ctypes.data, st.ctypes.data, _capi.MEM_HOST)
        assert rc == 0 and (st == 0).all()
        for i in range(n):
            k = int(out_len[i])
            assert out[i * cap: i * cap + k].tobytes() == TEXT[:100 * (i + 1)]
            assert (out[i * cap + k:(i + 1) * cap] == 0xAB).all(), i
    finally:
        inf.close()
