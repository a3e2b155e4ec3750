"""GPU tests of flate_hip_decompress_members (Engine.decompress_members): every member of concatenated gzip / zlib / raw
streams in one call.  The expectation is the loop a caller writes today -- one member at a time from where the last one
ended, into what is left of the slot -- run on the CPU with the oracle's decompress and its consumed count; for gzip files
whose members are all valid, Python's gzip.decompress is a second opinion.  Both memory kinds, with and without the two
optional result arrays; the scan for member starts at its tile and load edges, false candidates, every error as a middle
and as a last member, tight slots, and the knobs that choose between the scan and the walk."""
import ctypes as C
import gzip as pygzip
import os
import zlib as pyzlib

import numpy as np
import pytest

import _member_plan as M
import _oracle as O
from flate_amd import _capi, synth
from gpu_util import engine

pytestmark = pytest.mark.gpu

CODE = {v: k for k, v in O.STATUS.items()}
CONTAINERS = [O.RAW, O.GZIP, O.ZLIB]
MEMKINDS = [_capi.MEM_HOST, _capi.MEM_DEVICE]
# bytes of slot beyond what a stream's good members produce, where the slot is not the point: more than any failing member
# here writes before it fails (they are made from 3000 bytes of text), so that it fails with its own status, not with 100
SLACK = 4096


def text(n, seed=0):
    return synth.text(synth.SEED_TEXT + seed, n).tobytes()


_expect = {}


def expect(stream, container, cap=None, flags=0):
    """the caller's loop on the CPU: (output, status, consumed, members), counting the members before the first failure;
    cap None: a slot that holds whatever the stream produces"""
    key = (bytes(stream), container, cap, flags)
    if key not in _expect:
        s = np.frombuffer(bytes(stream), dtype=np.uint8)
        pos = members = 0
        out = []
        produced = 0
        while True:
            st, data, used = O.decompress(s[pos:], container, flags, cap=None if cap is None else cap - produced)
            if CODE[st] != 0:
                _expect[key] = (b"".join(out), CODE[st], pos, members)
                break
            out.append(data)
            produced += len(data)
            pos += used
            members += 1
            if pos == len(s):
                _expect[key] = (b"".join(out), 0, pos, members)
                break
    return _expect[key]


def call(eng, streams, container, caps, memkind, flags=0, extras=True):
    """flate_hip_decompress_members -> (outputs, statuses, consumed or None, members or None)"""
    eng._sync_env()
    n = len(streams)
    blob, in_off = eng._host_input(streams)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.array(caps, dtype=np.uint64), out=out_off[1:])
    total = int(out_off[-1])
    L = eng._L
    if memkind == _capi.MEM_HOST:
        out = np.full(total + 8, 0xEE, dtype=np.uint8)
        out_len = np.zeros(n, dtype=np.uint64)
        status = np.full(n, -1, dtype=np.int32)
        used = np.zeros(n, dtype=np.uint64)
        mem = np.zeros(n, dtype=np.uint32)
        rc = L.flate_hip_decompress_members(eng._h, blob.ctypes.data, in_off.ctypes.data, n, container, flags, out.ctypes.data,
                                            out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data,
                                            used.ctypes.data if extras else None, mem.ctypes.data if extras else None, memkind)
        eng._check(rc, "flate_hip_decompress_members")
        assert bytes(out[total:]) == b"\xEE" * 8, "bytes behind the last slot were written"
    else:
        import torch
        dev = "cuda:0"
        t_in = torch.from_numpy(blob.copy()).to(dev)
        t_inoff = torch.from_numpy(in_off.view(np.int64).copy()).to(dev)
        t_outoff = torch.from_numpy(out_off.view(np.int64).copy()).to(dev)
        t_out = torch.full((total + 8,), 0xEE, dtype=torch.uint8, device=dev)
        t_len = torch.zeros(n, dtype=torch.int64, device=dev)
        t_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        t_used = torch.zeros(n, dtype=torch.int64, device=dev)
        t_mem = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rc = L.flate_hip_decompress_members(eng._h, t_in.data_ptr(), t_inoff.data_ptr(), n, container, flags, t_out.data_ptr(),
                                            t_outoff.data_ptr(), t_len.data_ptr(), t_st.data_ptr(),
                                            t_used.data_ptr() if extras else None, t_mem.data_ptr() if extras else None, memkind)
        eng._check(rc, "flate_hip_decompress_members")
        torch.cuda.synchronize()
        out = t_out.cpu().numpy()
        out_len = t_len.cpu().numpy().view(np.uint64)
        status = t_st.cpu().numpy()
        used = t_used.cpu().numpy().view(np.uint64)
        mem = t_mem.cpu().numpy().view(np.uint32)
        assert bytes(out[total:]) == b"\xEE" * 8, "bytes behind the last slot were written"
    for i in range(n):
        assert int(out_len[i]) <= caps[i], "stream %d: out_len %d beyond its slot %d" % (i, out_len[i], caps[i])
    outs = [out[int(out_off[i]): int(out_off[i]) + int(out_len[i])].tobytes() for i in range(n)]
    return (outs, [int(s) for s in status], [int(u) for u in used] if extras else None,
            [int(m) for m in mem] if extras else None)


def check(eng, streams, container, memkind, caps=None, flags=0, extras=True):
    """one call against the loop; returns what the call returned"""
    if caps is None:
        caps = [len(expect(s, container, None, flags)[0]) + SLACK for s in streams]
    got = call(eng, streams, container, caps, memkind, flags, extras)
    for i, s in enumerate(streams):
        out, st, used, members = expect(s, container, caps[i], flags)
        what = "stream %d of %d (%d bytes, container %d, memkind %d)" % (i, len(streams), len(s), container, memkind)
        assert got[1][i] == st, "%s: status %d, the loop says %d" % (what, got[1][i], st)
        assert got[0][i] == out, "%s: %d bytes, the loop has %d" % (what, len(got[0][i]), len(out))
        if extras:
            assert got[2][i] == used, "%s: consumed %d, the loop says %d" % (what, got[2][i], used)
            assert got[3][i] == members, "%s: %d members, the loop says %d" % (what, got[3][i], members)
    return got


def gz_member(data, mode=6, name=None):
    """a gzip member, with an FNAME field when asked for (container.zig writes none)"""
    m = O.compress(data, O.GZIP, mode)
    if name is None:
        return m
    assert 0 not in name
    return m[:3] + bytes([m[3] | 0x08]) + m[4:10] + name + b"\0" + m[10:]


MAGIC = bytes([0x1F, 0x8B, 0x08])


# ---- 1: one member per stream -------------------------------------------------------------------------------------
@pytest.mark.parametrize("memkind", MEMKINDS)
@pytest.mark.parametrize("container", CONTAINERS)
def test_one_member_per_stream_is_decompress_batch(container, memkind):
    eng = engine()
    datas = [text(n, k) for k, n in enumerate((0, 1, 100, 4097, 70000))]
    streams = [O.compress(d, container, m) for d in datas for m in (0, 1, 6)]
    caps = [len(d) + 8 for d in datas for _ in range(3)]
    outs, st, used, mem = check(eng, streams, container, memkind, caps)
    b_outs, b_st, b_used = eng.decompress_many(streams, container, 0, caps)
    assert (outs, st, used) == (b_outs, b_st, b_used)
    assert st == [0] * len(streams) and mem == [1] * len(streams)
    if container == O.GZIP:
        assert eng.member_paths()[:2] == (len(streams), 0)


# ---- 2: three members -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extras", [True, False])
@pytest.mark.parametrize("memkind", MEMKINDS)
@pytest.mark.parametrize("container", CONTAINERS)
def test_three_members_of_three_modes(container, memkind, extras):
    eng = engine()
    parts = [text(5000, 1), text(70001, 2), text(33333, 3)]
    one = b"".join(O.compress(p, container, m) for p, m in zip(parts, (0, 1, 6)))
    two = b"".join(O.compress(p, container, m) for p, m in zip(parts[::-1], (6, 0, 1)))
    got = check(eng, [one, two], container, memkind, extras=extras)
    assert got[1] == [0, 0] and got[0] == [b"".join(parts), b"".join(parts[::-1])]
    if extras:
        assert got[3] == [3, 3] and got[2] == [len(one), len(two)]
    if container == O.GZIP:
        assert pygzip.decompress(one) == got[0][0]


# ---- 3: more members than a wave has lanes ------------------------------------------------------------------------
@pytest.mark.parametrize("memkind", MEMKINDS)
def test_seventy_empty_members_then_text(memkind):
    eng = engine()
    empty = O.compress(b"", O.GZIP, 6)
    assert len(empty) == 20
    tail = text(3000, 4)
    s = empty * 70 + O.compress(tail, O.GZIP, 6)
    outs, st, used, mem = check(eng, [s, empty * 70, s], O.GZIP, memkind)
    assert st == [0, 0, 0] and mem == [71, 70, 71] and outs[0] == tail == pygzip.decompress(s) and outs[1] == b""


def test_more_members_than_a_tile_of_successors():
    """the chain of one stream is followed from LDS a tile of successors at a time; the second stream's candidates lie
    behind the first's 5000 in the call's list"""
    eng = engine()
    n = 2 * M.lds_tile() + 904
    empty = O.compress(b"", O.GZIP, 6)
    tail = text(1000, 40)
    s = empty * n + O.compress(tail, O.GZIP, 1)
    outs, st, used, mem = check(eng, [s, s[20:]], O.GZIP, _capi.MEM_DEVICE)
    assert st == [0, 0] and mem == [n + 1, n] and outs == [tail, tail]
    assert eng.member_paths() == (2, 0, 0)


# ---- 4: the magic at every offset around a scan tile's edge, a step's and a 16-byte load's ----------------------
def edge_streams():
    """streams of two members laid out back to back so that the second member's 1f 8b 08 starts at edge + d of the batch for
    every d in -3 .. 1: the first member's FNAME is padded for it.  The batch starts at an aligned address (a device
    allocation), so an offset into the batch is an offset into the scan's tiles."""
    T = M.scan_tile()
    first, second = text(300, 5), text(500, 6)
    bare = len(gz_member(first, 6, b"x")) - 1
    b = O.compress(second, O.GZIP, 6)
    streams, at = [], 0
    for edge in (T, 1024, 16 * 37):
        for d in range(-3, 2):
            want = (edge + d) % T  # where the second member starts, modulo the tile
            start = at + bare + 1
            pad = (want - start) % T + 1
            a = gz_member(first, 6, b"a" * pad)
            assert (at + len(a)) % T == want
            streams.append(a + b)
            at += len(a) + len(b)
    return streams, first + second


@pytest.mark.parametrize("memkind", MEMKINDS)
def test_member_starts_around_tile_and_load_edges(memkind):
    eng = engine()
    streams, both = edge_streams()
    outs, st, used, mem = check(eng, streams, O.GZIP, memkind)
    assert st == [0] * len(streams) and mem == [2] * len(streams) and outs == [both] * len(streams)
    assert eng.member_paths()[:2] == (len(streams), 0)


def test_a_match_may_not_straddle_two_streams():
    """stream 0 ends in 1f 8b, stream 1 begins with 08: neither has a member there"""
    eng = engine()
    m = O.compress(text(200, 7), O.GZIP, 6)
    streams = [m + MAGIC[:2], MAGIC[2:] + m, m + MAGIC[:1], MAGIC[1:] + m, m]
    outs, st, used, mem = check(eng, streams, O.GZIP, _capi.MEM_HOST)
    assert st == [1, 2, 1, 2, 0] and mem == [1, 0, 1, 0, 1]


# ---- 5: false candidates ----------------------------------------------------------------------------------------
def false_candidate_streams():
    inner = O.compress(text(1000, 8), O.GZIP, 6) + O.compress(text(10, 9), O.GZIP, 1)
    real = O.compress(text(2000, 10), O.GZIP, 6)
    nested = gz_member(inner, 0) + real          # a store-only member whose payload is a two-member gzip file
    named = gz_member(text(700, 11), 6, b"a" + MAGIC + b"b" + MAGIC) + real
    many = gz_member(MAGIC * 1000, 0) + real
    return [nested, named, many], [inner + text(2000, 10), text(700, 11) + text(2000, 10), MAGIC * 1000 + text(2000, 10)]


@pytest.mark.parametrize("memkind", MEMKINDS)
def test_false_candidates_are_never_reached(memkind):
    eng = engine()
    streams, outputs = false_candidate_streams()
    for k in range(3):
        outs, st, used, mem = check(eng, [streams[k]], O.GZIP, memkind)
        assert (outs, st, mem) == ([outputs[k]], [0], [2])
        assert pygzip.decompress(streams[k]) == outputs[k]
        scanned, walked, off_chain = eng.member_paths()
        assert (scanned, walked) == (1, 0)
        assert off_chain >= (2, 2, 1000)[k]
    check(eng, streams, O.GZIP, memkind)


# ---- 6: errors ----------------------------------------------------------------------------------------------------
def flipped(member, container):
    """the member with the first single bit flipped that makes the oracle report a code-level error (7 .. 14)"""
    for bit in range(8 * 12, 8 * len(member) - 64):
        bad = bytearray(member)
        bad[bit >> 3] ^= 1 << (bit & 7)
        if 7 <= CODE[O.decompress(bytes(bad), container)[0]] <= 14:
            return bytes(bad)
    raise AssertionError("no bit of the member breaks its codes")


_bad = {}


def bad_members(container):
    """name -> (a member that fails, the status it fails with when it is the last one)"""
    if container not in _bad:
        good = O.compress(text(3000, 12), container, 6)
        foot = {O.RAW: 0, O.GZIP: 8, O.ZLIB: 4}[container]
        r = {"truncated block": (good[:len(good) - foot - 5], 1)}
        bad = flipped(good, container)
        r["flipped bit"] = (bad, CODE[O.decompress(bad, container)[0]])
        if foot:
            r["truncated footer"] = (good[:-2], 1)
        if container == O.GZIP:
            r["wrong crc"] = (good[:-8] + bytes([good[-8] ^ 1]) + good[-7:], 4)
            r["wrong isize"] = (good[:-4] + bytes([good[-4] ^ 1]) + good[-3:], 5)
        if container == O.ZLIB:
            r["wrong adler"] = (good[:-1] + bytes([good[-1] ^ 1]), 6)
        _bad[container] = r
    return _bad[container]


def error_streams(container):
    a, c = O.compress(text(1500, 13), container, 6), O.compress(text(800, 14), container, 1)
    streams, last_status = [], []
    for name, (bad, status) in sorted(bad_members(container).items()):
        streams += [a + bad + c, a + c + bad]
        last_status += [None, status]
    for fill in (0x00, 0xFF):
        for k in (1, 9, 10, 64):
            streams.append(a + c + bytes([fill]) * k)
            last_status.append(None)
    streams.append(b"")
    last_status.append(1)
    return streams, last_status


@pytest.mark.parametrize("memkind", MEMKINDS)
@pytest.mark.parametrize("container", CONTAINERS)
def test_errors_in_the_middle_and_at_the_end(container, memkind):
    eng = engine()
    streams, last_status = error_streams(container)
    outs, st, used, mem = check(eng, streams, container, memkind)
    for i, want in enumerate(last_status):
        if want is not None:
            assert st[i] == want, (i, st[i], want)
    assert st[-1] == 1 and mem[-1] == 0 and used[-1] == 0  # the empty stream
    if container == O.GZIP:  # trailing bytes behind two good members: the header rule
        trailing = st[-9:-1]
        assert trailing == [1, 1, 2, 2] * 2 and mem[-9:-1] == [2] * 8
    # every stream on its own says the same (a batch of one has other tables)
    for i in (0, 1, len(streams) - 2, len(streams) - 1):
        check(eng, [streams[i]], container, memkind)


# ---- 7: slots -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memkind", MEMKINDS)
@pytest.mark.parametrize("container", CONTAINERS)
def test_slots_exact_short_and_zero(container, memkind):
    eng = engine()
    parts = [text(4000, 15), text(100, 16), text(9000, 17)]
    s = b"".join(O.compress(p, container, 6) for p in parts)
    total = sum(map(len, parts))
    outs, st, used, mem = check(eng, [s, s, s, s], container, memkind, caps=[total, total - 1, 0, len(parts[0])])
    assert st == [0, 100, 100, 100] and mem == [3, 2, 0, 1]
    assert outs[1] == parts[0] + parts[1] and outs[3] == parts[0]
    empty = O.compress(b"", container, 6) * 3
    assert check(eng, [empty], container, memkind, caps=[0])[3] == [3]


# ---- 8: a mixed batch -----------------------------------------------------------------------------------------------
_mixed = {}


def mixed_batch():
    """33 gzip streams of 1 .. 40 members; some fail; one member has 300 KiB of input (the inner decode cuts it) and lies at
    an odd offset between members of 64 KiB of input"""
    if not _mixed:
        rng = np.random.RandomState(33)
        small = [O.compress(text(int(n), 20 + k), O.GZIP, (0, 1, 6)[k % 3]) for k, n in enumerate(rng.randint(0, 3000, 24))]
        noise = rng.randint(0, 256, 1 << 16).astype(np.uint8).tobytes()
        mid = O.compress(noise[:65536 - 23], O.GZIP, 0)
        assert len(mid) == 65536  # 64 KiB of input
        big_text = text(600 << 10, 18)
        big = O.compress(big_text, O.GZIP, 1)
        assert len(big) >= 300 << 10
        bad = sorted(bad_members(O.GZIP).items())
        streams = []
        for i in range(33):
            k = 1 + (i * 11) % 40
            members = [small[(i + j) % len(small)] for j in range(k)]
            if i % 5 == 1:  # a failing member, in the middle or last
                members[(i * 3) % k if i % 2 else k - 1] = bad[i % len(bad)][1][0]
            if i == 17:
                lead = next(m for m in small if len(m) % 2 == 1)
                members = [lead, mid, big, mid, small[2]]
                assert (len(lead) + len(mid)) % 2 == 1
            streams.append(b"".join(members))
        _mixed["streams"] = streams
    return _mixed["streams"]


@pytest.mark.parametrize("memkind", MEMKINDS)
def test_mixed_batch(memkind):
    eng = engine()
    streams = mixed_batch()
    outs, st, used, mem = check(eng, streams, O.GZIP, memkind)
    assert st[17] == 0 and mem[17] == 5 and outs[17] == pygzip.decompress(streams[17])
    assert sorted(set(mem)) != [1] and any(s != 0 for s in st) and max(mem) == 40
    paths = eng.inflate_paths()
    assert paths["span_done"] + paths["par_done"] >= 1, paths  # the long member was not left to one wave


# ---- 9: the knobs ---------------------------------------------------------------------------------------------------
def with_env(eng, name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old
        eng._sync_env()


def test_scan_off_walks_with_identical_results():
    eng = engine()
    streams = mixed_batch()[:12] + false_candidate_streams()[0] + error_streams(O.GZIP)[0]
    caps = [len(expect(s, O.GZIP)[0]) + SLACK for s in streams]
    scanned = call(eng, streams, O.GZIP, caps, _capi.MEM_DEVICE)
    assert eng.member_paths()[:2] == (len(streams), 0)

    def walk():
        got = check(eng, streams, O.GZIP, _capi.MEM_DEVICE, caps)
        assert eng.member_paths() == (0, len(streams), 0)
        return got
    assert with_env(eng, "FLATE_HIP_MEMBER_SCAN", "0", walk) == scanned
    call(eng, streams[:1], O.GZIP, caps[:1], _capi.MEM_HOST)
    assert eng.member_paths()[:2] == (1, 0)  # ... and back


def test_too_many_candidates_walk_with_identical_results():
    eng = engine()
    streams, outputs = false_candidate_streams()
    caps = [len(o) + SLACK for o in outputs]
    scanned = call(eng, streams, O.GZIP, caps, _capi.MEM_HOST)
    assert eng.member_paths()[:2] == (3, 0)

    def few():
        got = check(eng, streams, O.GZIP, _capi.MEM_HOST, caps)
        assert eng.member_paths() == (0, 3, 0)
        # eight candidates are allowed: two members of two streams stay on the scan
        small = [O.compress(text(50, 30), O.GZIP, 6) * 2] * 4
        check(eng, small, O.GZIP, _capi.MEM_HOST)
        assert eng.member_paths() == (4, 0, 0)
        return got
    assert with_env(eng, "FLATE_HIP_MEMBER_CANDIDATES", "8", few) == scanned
    assert scanned[0] == outputs


@pytest.mark.parametrize("container", [O.RAW, O.ZLIB])
def test_zlib_and_raw_are_always_walked(container):
    eng = engine()
    s = b"".join(O.compress(text(n, 31), container, 6) for n in (10, 2000, 0, 300))
    py = pyzlib.compress(text(777, 32), 9) if container == O.ZLIB else pyzlib.compress(text(777, 32), 9)[2:-4]
    outs, st, used, mem = check(eng, [s, py + s, b""], container, _capi.MEM_DEVICE)
    assert st == [0, 0, 1] and mem == [4, 5, 0] and outs[1] == text(777, 32) + outs[0]
    assert eng.member_paths() == (0, 3, 0)
