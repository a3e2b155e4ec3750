"""GPU tests of the size probe (flate_hip_decompressed_sizes / Engine.decompressed_sizes): for every stream the probe's
status is what decompress reports with a slot that is large enough -- footer checks excepted, the probe has no bytes to
sum --, its size is the oracle's output length, its consumed count the oracle's; long streams are cut into spans whose
chain must close, and nothing but the three result arrays is written."""
import zlib as pyzlib

import numpy as np
import pytest

import _big_member as B
import _deflate_synth as S
import _inflate_edge_cases as E
import _oracle as O
from conftest import golden
from flate_amd import synth
from gpu_util import engine
from test_oracle_inflate_pins import FUZZ, GZ_HDR

pytestmark = pytest.mark.gpu

N_RANDOM, RANDOM_SEED = 200, 5000  # the seeds of test_gpu_inflate_synth
GARBAGE = bytes([0xA5, 0x00, 0xFF, 0x1F, 0x8B, 0x78, 0x9C])
BATCH = 256


def wrap(raw, out, container):
    """a raw deflate stream that expands to `out`, in a container"""
    if container == O.GZIP:
        return GZ_HDR + raw + pyzlib.crc32(out).to_bytes(4, "little") + (len(out) & 0xFFFFFFFF).to_bytes(4, "little")
    if container == O.ZLIB:
        return bytes([0x78, 0x9C]) + raw + pyzlib.adler32(out).to_bytes(4, "big")
    return raw


_raw = []


def raw_candidates():
    """(name, raw deflate stream) of everything test 1 draws from; which of them are valid is the oracle's verdict"""
    if not _raw:
        _raw.extend(("seed %d" % (RANDOM_SEED + k), s) for k, (s, _) in enumerate(S.random_streams(RANDOM_SEED, N_RANDOM)))
        for n in (0, 1, 257, 65535, 200000):
            text = synth.text(synth.SEED_TEXT, n).tobytes()
            _raw.extend(("text %d mode %d" % (n, m), O.compress(text, O.RAW, m)) for m in (0, 1, 4, 6, 9))
        _raw.extend(("edge " + n, E.CASES[n]) for n in sorted(E.CASES))
        _raw.extend(("synth " + n, S.CASES[n][0]) for n in sorted(S.CASES))
    return _raw


_verdict = {}


def verdict(raw, flags):
    """the oracle on a raw stream: (status name, output, consumed), once"""
    if (raw, flags) not in _verdict:
        _verdict[raw, flags] = O.decompress(raw, O.RAW, flags)
    return _verdict[raw, flags]


def valid_streams(container, flags):
    """(name, stream in the container, output length, consumed) of every candidate the oracle accepts"""
    out = []
    for name, raw in raw_candidates():
        st, data, used = verdict(raw, flags)
        if st != "Ok":
            continue
        s = wrap(raw[:used], data, container)
        out.append((name, s, len(data), len(s)))
    return out


def probe(eng, streams, container, flags=0):
    sizes, st, used = [], [], []
    for k in range(0, len(streams), BATCH):
        a, b, c = eng.decompressed_sizes(streams[k:k + BATCH], container, flags)
        sizes += a
        st += b
        used += c
    return sizes, st, used


def probe_status_of(decompress_status):
    return 0 if decompress_status in (4, 5, 6) else decompress_status


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("container", [O.RAW, O.GZIP, O.ZLIB])
def test_valid_streams(container, flags):
    """1: status 0, the oracle's size and consumed count; 7 bytes of garbage behind the stream move nothing"""
    eng = engine()
    items = valid_streams(container, flags)
    assert len(items) >= N_RANDOM // 2 + 25 + len(S.VALID) // 2
    # the container and the wrapper agree with the oracle (a few: the oracle is not what is under test)
    for name, s, n, used in items[::37]:
        assert O.decompress(s, container, flags)[0::2] == ("Ok", used), name
    for tail in (b"", GARBAGE):
        sizes, st, used = probe(eng, [it[1] + tail for it in items], container, flags)
        bad = [(it[0], s_, z, it[2], u, it[3]) for it, z, s_, u in zip(items, sizes, st, used)
               if s_ != 0 or z != it[2] or u != it[3]]
        assert not bad, (container, flags, len(tail), len(bad), bad[:8])


def cuts(s):
    return sorted({len(s) // 3, 2 * len(s) // 3, len(s) - 1} - {len(s)})


@pytest.mark.parametrize("container", [O.RAW, O.GZIP, O.ZLIB])
def test_bad_streams_report_what_decompress_reports(container):
    """2: the fuzz corpus, the error cases of the generators and every valid stream cut at three places: the probe's status
    is decompress's, footer mismatches excepted.  (The slot of a cut stream is its whole stream's output + 8: a prefix
    cannot make more; everything else gets decompress_many's worst case.)"""
    eng = engine()
    streams, caps = [], []
    if container == O.RAW:
        for name, err, out in FUZZ:
            streams.append(golden("fuzz", name + ".input"))
            caps.append(None)
        for name, raw in raw_candidates():
            if verdict(raw, 0)[0] != "Ok":
                streams.append(raw)
                caps.append(None)
    for name, s, n, used in valid_streams(container, 0):
        for c in cuts(s):
            streams.append(s[:c])
            caps.append(n + 8)
    if container != O.RAW:
        s, n = next((it[1], it[2]) for it in valid_streams(container, 0) if it[0] == "text 257 mode 6")
        flipped = bytearray(s)
        flipped[-1] ^= 0x10
        streams += [bytes(flipped), s[:-1]]
        caps += [n + 8, n + 8]
    worst = [max(1 << 16, len(s) * 1100 + 1024) for s in streams]
    caps = [w if c is None else c for c, w in zip(caps, worst)]
    want = []
    for k in range(0, len(streams), BATCH):
        want += eng.decompress_many(streams[k:k + BATCH], container, 0, caps=caps[k:k + BATCH])[1]
    assert 100 not in want
    _, st, _ = probe(eng, streams, container)
    bad = [(i, len(streams[i]), st[i], want[i]) for i in range(len(streams)) if st[i] != probe_status_of(want[i])]
    assert not bad, (container, len(bad), bad[:8])
    assert sum(1 for w in want if w != 0) >= len(streams) // 2
    if container != O.RAW:
        assert want[-2] in (4, 5, 6) and st[-2] == 0  # one flipped footer bit
        assert want[-1] == 1 and st[-1] == 1          # the footer cut by a byte


@pytest.mark.parametrize("k", [1, 2, 258, 32768])
def test_invalid_match_at_the_edge(k):
    """3: a match of distance k behind exactly k - 1 bytes is InvalidMatch, behind k bytes it is fine"""
    eng = engine()
    lits = [("L", (i * 7) & 255) for i in range(k)]
    short = E.fixed_block(lits[:k - 1] + [("M", 3, k)])
    exact = E.fixed_block(lits + [("M", 3, k)])
    sizes, st, used = eng.decompressed_sizes([short, exact], O.RAW)
    assert st == [11, 0] and sizes[1] == k + 3 and used[1] == len(exact)
    assert O.decompress(short, O.RAW)[0] == "InvalidMatch" and len(O.decompress(exact, O.RAW)[1]) == k + 3


def one_block_stream(n_out):
    """n_out bytes as ONE dynamic block: no block start behind the first, nowhere to cut"""
    s = S.Stream(4242)
    ll, dl = s.random_code(15, .5)
    lits = [x for x in range(256) if ll[x]]
    toks, have = [("L", lits[0])] * 8, 8
    for t in s.pick(ll, dl, 3 * n_out // 64, p_match=.9):
        ln = 1 if t[0] == "L" else t[1]
        if have + ln > n_out:
            break
        toks.append(t if t[0] == "L" or t[2] <= have else ("L", lits[0]))
        have += 1 if toks[-1][0] == "L" else ln
    toks += [("L", lits[0])] * (n_out - have)
    s.dynamic(ll, dl, toks, final=1)
    stream, want = s.done()
    assert want is not None and len(want) == n_out
    return stream


def need_hist_pair():
    """about 40 KiB of empty stored blocks, then a fixed block that starts with a match of distance 1 (A: InvalidMatch),
    or with a literal and that match (B: 4 bytes)"""
    empty = b"".join(E.stored(b"", 0) for _ in range(8192))
    return empty + E.fixed_block([("M", 3, 1)]), empty + E.fixed_block([("L", 65), ("M", 3, 1)])


def test_long_streams_are_cut_into_spans(monkeypatch):
    """4: a long stream's size comes from a closed chain of spans (size_paths says so: a silent fallback to one wave fails
    here), a stream with nowhere to cut is counted whole, a match that reaches before its span's stream is refused."""
    eng = engine()
    text = synth.text(synth.SEED_TEXT, 4 << 20).tobytes()
    cut = [O.compress(text, O.RAW, 6), O.compress(text, O.RAW, O.HUFFMAN), O.compress(text, O.RAW, O.STORE)]
    whole = one_block_stream(2 << 20)
    assert len(whole) >= 65536
    a, b = need_hist_pair()
    batch = cut + [whole, a, b]
    want = ([len(text)] * 3 + [2 << 20, None, 4], [0, 0, 0, 0, 11, 0], [len(s) for s in batch])
    monkeypatch.setenv("FLATE_HIP_INFLATE_SPANS", "32768")
    seams, seam_text = E.fixed_seam_stream()  # spans that run through fixed blocks whose matches reach before the span
    assert seam_text == text
    for s in cut + [seams]:
        assert eng.decompressed_sizes([s], O.RAW) == ([len(text)], [0], [len(s)])
        assert eng.size_paths() == (1, 0)
    assert eng.decompressed_sizes([whole], O.RAW) == ([2 << 20], [0], [len(whole)])
    assert eng.size_paths() == (0, 1)
    sizes, st, used = eng.decompressed_sizes([a, b], O.RAW)
    assert st == [11, 0] and sizes[1] == 4 and used[1] == len(b)
    assert eng.size_paths() == (1, 1)  # B's chain closes; A's last span needs a byte of history that is not there
    got = eng.decompressed_sizes(batch, O.RAW)
    assert eng.size_paths() == (4, 2)
    # gzip: the footer and consumed belong to the span that sees BFINAL
    gz = wrap(cut[0], text, O.GZIP)
    assert eng.decompressed_sizes([gz + GARBAGE], O.GZIP) == ([len(text)], [0], [len(gz)])
    assert eng.size_paths() == (1, 0)
    monkeypatch.setenv("FLATE_HIP_INFLATE_SPANS", "0")
    same = eng.decompressed_sizes(batch, O.RAW)
    assert eng.size_paths() == (0, len(batch))
    assert eng.decompressed_sizes([seams], O.RAW) == ([len(text)], [0], [len(seams)])
    assert eng.size_paths() == (0, 1)
    for r in (got, same):
        assert r[1] == want[1]
        assert [z for z, s_ in zip(r[0], r[1]) if s_ == 0] == [z for z in want[0] if z is not None]
        assert [u for u, s_ in zip(r[2], r[1]) if s_ == 0] == [u for u, s_ in zip(want[2], want[1]) if s_ == 0]


def test_beyond_4_gib():
    """5: a member whose output is just above 2^32 bytes: the size is 64-bit, gzip's ISIZE is the size mod 2^32, and no
    output buffer exists anywhere"""
    eng = engine()
    groups = (1 << 32) // 2064 + 1
    n = B.output_size(groups)
    assert (1 << 32) < n < (1 << 32) + 4096
    raw = b"".join(B.raw_chunks(groups))
    assert eng.decompressed_sizes([raw], O.RAW) == ([n], [0], [len(raw)])
    gz = b"".join(B.gzip_chunks(groups))
    assert int.from_bytes(gz[-4:], "little") == n - (1 << 32)
    assert eng.decompressed_sizes([gz], O.GZIP) == ([n], [0], [len(gz)])


def test_device_memory(monkeypatch):
    """6: device arrays, input offsets of every residue mod 8, set_sync(0): the host call's results, and nothing written
    but sizes[0..n), status[0..n), consumed[0..n)"""
    import torch
    eng = engine()
    monkeypatch.delenv("FLATE_HIP_INFLATE_SPANS", raising=False)
    short = [it for it in valid_streams(O.ZLIB, 0) if len(it[1]) < 60000]  # (none that the probe would cut)
    items = short[:40] + short[-6:]
    streams, off = [], 0
    for k, it in enumerate(items):  # garbage behind each stream brings the next one to offset k + 1 (mod 8)
        s = it[1]
        s += GARBAGE * 2
        s = s[:len(it[1]) + ((k + 1 - off - len(it[1])) % 8)]
        streams.append(s)
        off += len(s)
    streams.append(streams[3][:len(streams[3]) // 2])  # and one that fails
    n = len(streams)
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum([len(s) for s in streams], out=offs[1:])
    assert {int(o) % 8 for o in offs[:-1]} == set(range(8))
    want = eng.decompressed_sizes(streams, O.ZLIB)
    assert want[1][:-1] == [0] * (n - 1) and want[1][-1] != 0
    blob = np.frombuffer(b"".join(streams), np.uint8).copy()
    d_in = torch.from_numpy(blob).cuda()
    d_off = torch.from_numpy(offs.view(np.int64)).cuda()
    SENT = 0x5A5A5A5A5A5A5A5A
    for with_consumed in (True, False):
        d_sizes = torch.full((n + 1,), SENT, dtype=torch.int64, device="cuda")
        d_used = torch.full((n + 1,), SENT, dtype=torch.int64, device="cuda")
        d_st = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        eng.set_sync(0)
        try:
            eng.decompressed_sizes_device(d_in.data_ptr(), d_off.data_ptr(), n, O.ZLIB, 0, d_sizes.data_ptr(),
                                          d_st.data_ptr(), d_used.data_ptr() if with_consumed else None)
            torch.cuda.synchronize()
        finally:
            eng.set_sync(1)
        assert eng.size_paths() == (0, n)
        sizes, st, used = d_sizes.cpu().tolist(), d_st.cpu().tolist(), d_used.cpu().tolist()
        assert st[:n] == want[1] and st[n] == 0x5A5A5A5A
        assert [z for z, s_ in zip(sizes[:n], st) if s_ == 0] == [z for z, s_ in zip(want[0], want[1]) if s_ == 0]
        assert sizes[n] == SENT and used[n] == SENT
        if with_consumed:
            assert used[:n] == want[2]
        else:
            assert used == [SENT] * (n + 1)
        assert np.array_equal(d_in.cpu().numpy(), blob)


def test_decompress_many_measure(monkeypatch):
    """7: measure=True sizes the slots with the probe: the same bytes, statuses and consumed counts as measure=False"""
    eng = engine()
    monkeypatch.delenv("FLATE_HIP_INFLATE_SPANS", raising=False)
    texts = [synth.text(synth.SEED_TEXT + k, n).tobytes() for k, n in enumerate((0, 1, 300, 70000, 200000))]
    for container in (O.RAW, O.ZLIB, O.GZIP):
        streams = [O.compress(t, container, 6) for t in texts]
        corrupt = bytearray(streams[3])
        corrupt[len(corrupt) // 2] ^= 0x55
        streams.append(bytes(corrupt))
        if container == O.GZIP:
            # two members: ISIZE at the end of the file is the second member's, too small for the first
            streams.append(O.compress(texts[4], container, 6) + O.compress(texts[2], container, 6))
        plain = eng.decompress_many(streams, container)
        assert plain[1][:5] == [0] * 5 and plain[0][:5] == texts
        if container == O.GZIP:
            assert plain[1][-1] == 0 and plain[0][-1] == texts[4]
        measured = eng.decompress_many(streams, container, measure=True)
        assert measured == plain, container
    raw = [O.compress(t, O.RAW, 6) for t in texts]
    eng.decompress_many(raw, O.RAW, measure=True)
    paths = eng.inflate_paths()
    sizes = eng.decompressed_sizes(raw, O.RAW)[0]
    eng.decompress_many(raw, O.RAW, caps=[z + 8 for z in sizes])
    assert paths == eng.inflate_paths()
    eng.decompressed_sizes(raw, O.RAW)
    assert paths == eng.inflate_paths()  # the probe leaves decompress's counters alone
