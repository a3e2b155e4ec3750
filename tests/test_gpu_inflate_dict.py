"""GPU tests of inflate with preset dictionaries: flate_hip_decompress_batch_dict (k_inflate_dict, both LDS rings), the
resumable inflater with flate_hip_inflater_set_dictionary, and the zdict= keyword of the Python mirror.  The inputs and
what they must decode to are tests/_dict_cases.py, whose expectations tests/test_dict_cases_cpu.py holds against stdlib
zlib; every case that file accepts is run here."""
import io
import zlib as pyzlib

import numpy as np
import pytest

import _dict_cases as dc
from gpu_util import engine

pytestmark = pytest.mark.gpu

NEED_INPUT, NEED_OUTPUT, NEED_DICT, WRONG_DICT = 104, 105, 106, 107
SLACK = 264  # room behind the expected bytes: a failing stream never fails for want of room


def tables(cases):
    """(dicts, dict_of) of a batch: every distinct dictionary once"""
    index, dicts, of = {}, [], []
    for c in cases:
        if c.zdict is None:
            of.append(None)
            continue
        if c.zdict not in index:
            index[c.zdict] = len(dicts)
            dicts.append(c.zdict)
        of.append(index[c.zdict])
    return dicts, of


def check(cases, outs, st, cons):
    for c, o, s, u in zip(cases, outs, st, cons):
        assert s == c.status, (c.name, s, c.status)
        assert len(o) == len(c.out), (c.name, len(o), len(c.out))
        assert o == c.out, c.name
        if c.consumed is not None:
            assert u == c.consumed, (c.name, u, c.consumed)


EMPTY = {0: b"\x03\x00", 2: pyzlib.compress(b"")}  # a stream of no bytes: its slot is the gap between two slots under test


def run_device(eng, cases, container, dicts, of, starts, caps, fill=0xAA):
    """flate_hip_decompress_batch_dict on device memory with slots at out[starts[i] .. + caps[i]).  The C ABI's slot i ends where
    slot i + 1 starts, so a gap between two slots is given to an empty stream of its own, which writes nothing.  Returns
    (outs, statuses, consumed, the whole output buffer)."""
    import torch
    n = len(cases)
    streams, d_of, out_off, real = [], [], [], []
    for i, c in enumerate(cases):
        real.append(len(streams))
        streams.append(c.stream)
        d_of.append(0xffffffff if of is None or of[i] is None else of[i])
        out_off.append(starts[i])
        if i + 1 < n and starts[i] + caps[i] != starts[i + 1]:
            assert starts[i] + caps[i] < starts[i + 1]
            streams.append(EMPTY[container])
            d_of.append(0xffffffff)
            out_off.append(starts[i] + caps[i])
    out_off.append(starts[-1] + caps[-1])
    m = len(streams)

    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()  # (a copy: frombuffer arrays are read-only)

    def offsets(lens):
        off = np.zeros(len(lens) + 1, np.int64)
        off[1:] = np.cumsum(lens)
        return off

    blob = np.frombuffer(b"".join(streams) + b"\0", np.uint8)
    dblob = np.frombuffer(b"".join(dicts) + b"\0", np.uint8)
    t_in, t_inoff, t_dict, t_doff = dev(blob), dev(offsets([len(z) for z in streams])), dev(dblob), dev(offsets([len(d) for d in dicts]))
    t_outoff = dev(np.array(out_off, np.int64))
    t_of = None if of is None else dev(np.array(d_of, np.uint32).view(np.int32))
    t_out = torch.full((int(out_off[-1]) + 64,), fill, dtype=torch.uint8, device="cuda")
    t_len, t_cons = torch.zeros(m, dtype=torch.int64, device="cuda"), torch.zeros(m, dtype=torch.int64, device="cuda")
    t_st = torch.full((m,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.decompress_dict_device(t_in.data_ptr(), t_inoff.data_ptr(), m, container, 0, t_out.data_ptr(), t_outoff.data_ptr(),
                               t_len.data_ptr(), t_st.data_ptr(), t_cons.data_ptr(), t_dict.data_ptr(), t_doff.data_ptr(),
                               len(dicts), None if t_of is None else t_of.data_ptr())
    torch.cuda.synchronize()
    out, ln, st, cons = t_out.cpu().numpy(), t_len.cpu().numpy(), t_st.cpu().numpy(), t_cons.cpu().numpy()
    assert all(int(st[j]) == 0 and int(ln[j]) == 0 for j in set(range(m)) - set(real))  # the gaps' streams
    outs = [out[starts[i]: starts[i] + int(ln[j])].tobytes() for i, j in enumerate(real)]
    return outs, [int(st[j]) for j in real], [int(cons[j]) for j in real], out


def packed_slots(cases, slack=SLACK):
    caps = [(len(c.out) + slack + 7) & ~7 for c in cases]
    starts = [0] * len(cases)
    for i in range(1, len(cases)):
        starts[i] = starts[i - 1] + caps[i - 1]
    return starts, caps


# ---------------------------------------------------------------- every case, both rings

@pytest.mark.parametrize("container", [0, 2])
@pytest.mark.parametrize("ring", [2048, 32768])
def test_every_case(monkeypatch, ring, container):
    """Families Z, S and H through Engine.decompress_many_dict, with FLATE_HIP_INFLATE_RING forcing each instantiation."""
    monkeypatch.setenv("FLATE_HIP_INFLATE_RING", str(ring))
    eng = engine()
    cases = [c for c in dc.CASES if c.container == container]
    assert cases
    dicts, of = tables(cases)
    outs, st, cons = eng.decompress_many_dict([c.stream for c in cases], dicts, of, container,
                                              caps=[len(c.out) + SLACK for c in cases])
    check(cases, outs, st, cons)


@pytest.mark.parametrize("container", [0, 2])
@pytest.mark.parametrize("ring", [2048, 32768])
def test_every_case_device_memory(monkeypatch, ring, container):
    monkeypatch.setenv("FLATE_HIP_INFLATE_RING", str(ring))
    eng = engine()
    cases = [c for c in dc.CASES if c.container == container]
    dicts, of = tables(cases)
    starts, caps = packed_slots(cases)
    outs, st, cons, _ = run_device(eng, cases, container, dicts, of, starts, caps)
    check(cases, outs, st, cons)


# ---------------------------------------------------------------- the record shape

def record_batch(container, n=1500, rlen=200):
    d = dc.TEXT[:32768]
    wbits = -15 if container == 0 else 15
    cases = []
    for i in range(n):
        off = (i * 131) % (32768 - rlen)
        r = dc.TEXT[off:off + rlen]
        z = dc.deflate(r, 6, wbits, d)
        cases.append(dc.Case("rec%d" % i, container, z, d, 0, r, len(z)))
    return cases, d


@pytest.mark.parametrize("container", [0, 2])
def test_record_batch_one_shared_dictionary(container):
    """about 1500 records of 200 bytes, one 32 KiB dictionary, dict_of = NULL: the small ring by the library's own rule"""
    eng = engine()
    cases, d = record_batch(container)
    assert sum(len(c.stream) for c in cases) < 0.5 * sum(len(c.out) for c in cases)  # (the dictionary is doing the work)
    outs, st, cons = eng.decompress_many_dict([c.stream for c in cases], [d], None, container, caps=[len(c.out) + 8 for c in cases])
    check(cases, outs, st, cons)
    starts, caps = packed_slots(cases, slack=0)
    outs, st, cons, _ = run_device(eng, cases, container, [d], None, starts, caps)
    check(cases, outs, st, cons)


def mixed_batch(container):
    wbits = -15 if container == 0 else 15
    tag = "w%d" % wbits
    cases = [c for c in dc.CASES if c.name.startswith("Z_l6_" + tag + "_d") and len(c.zdict) in (2048, 32768, 40000)]
    plain = [dc.TEXT[7000 + 50 * k: 7000 + 50 * k + 900] for k in range(6)]
    for k, r in enumerate(plain):  # streams without a dictionary, between the others
        z = dc.deflate(r, 6, wbits, b"") if container == 0 else pyzlib.compress(r, 6)
        cases.insert(3 * k, dc.Case("plain%d" % k, container, z, None, 0, r, len(z)))
    return cases


@pytest.mark.parametrize("container", [0, 2])
def test_three_dictionaries_and_none(container):
    eng = engine()
    cases = mixed_batch(container)
    dicts, of = tables(cases)
    assert len(dicts) == 3 and of.count(None) == 6
    outs, st, cons = eng.decompress_many_dict([c.stream for c in cases], dicts, of, container, caps=[len(c.out) + SLACK for c in cases])
    check(cases, outs, st, cons)
    starts, caps = packed_slots(cases)
    outs, st, cons, _ = run_device(eng, cases, container, dicts, of, starts, caps)
    check(cases, outs, st, cons)


# ---------------------------------------------------------------- slots

SLOT_CASES = ["S_p0_dist1_len258_fixed", "S_p0_dist1_len258_dyn", "S_p0_dist_hist_dyn", "S_straddle_near_fixed", "S_straddle_near_dyn",
              "S_straddle_far_small_fixed", "S_straddle_far_small_dyn", "S_stored10_dist15_dyn", "S_stored3000_dist3100_dyn",
              "S_round_over_260_dyn", "S_round_over_260_far_dyn", "S_two_in_a_round_dyn", "Z_l6_w-15_d2048_r4096", "Z_l9_w-15_d32768_r200",
              "Z_l6_w-15_d1789_r3"]


@pytest.mark.parametrize("ring", [2048, 32768])
def test_exact_fit_slots_at_every_residue(monkeypatch, ring):
    """Every slot exactly as long as its output, starting at each of the 8 residues of its address (the ring's bias meets the
    seeding of the ring here); the bytes between the slots stay as they were."""
    monkeypatch.setenv("FLATE_HIP_INFLATE_RING", str(ring))
    eng = engine()
    cases, starts, caps, at = [], [], [], 0
    for name in SLOT_CASES:
        for r in range(8):
            c = dc.BY_NAME[name]
            at = (at + 24 + 7) // 8 * 8 + r  # (torch's allocations are 8-byte aligned and more)
            cases.append(c)
            starts.append(at)
            caps.append(len(c.out))
            at += len(c.out)
    dicts, of = tables(cases)
    outs, st, cons, buf = run_device(eng, cases, 0, dicts, of, starts, caps)
    check(cases, outs, st, cons)
    keep = np.ones(len(buf), bool)
    for s, n in zip(starts, caps):
        keep[s:s + n] = False
    assert (buf[keep] == 0xAA).all()


@pytest.mark.parametrize("ring", [2048, 32768])
def test_slot_one_byte_short(monkeypatch, ring):
    monkeypatch.setenv("FLATE_HIP_INFLATE_RING", str(ring))
    eng = engine()
    cases = [dc.BY_NAME[n] for n in SLOT_CASES]
    dicts, of = tables(cases)
    caps = [len(c.out) - 1 for c in cases]
    starts = [0] * len(cases)
    for i in range(1, len(cases)):
        starts[i] = (starts[i - 1] + caps[i - 1] + 16 + 7) // 8 * 8 + i % 8
    outs, st, _, buf = run_device(eng, cases, 0, dicts, of, starts, caps)
    for c, o, s, cap in zip(cases, outs, st, caps):
        assert s == 100, (c.name, s)
        assert len(o) <= cap and o == c.out[:len(o)], c.name
    keep = np.ones(len(buf), bool)
    for s, n in zip(starts, caps):
        keep[s:s + n] = False
    assert (buf[keep] == 0xAA).all()


# ---------------------------------------------------------------- argument errors

def test_gzip_and_bad_tables_are_refused():
    eng = engine()
    with pytest.raises(ValueError):
        eng.decompress_many_dict([b"\x03\x00"], [b"abc"], None, 1)
    with pytest.raises(ValueError):
        eng.decompress_many_dict([b"\x03\x00"], [b"abc", b"def"], None, 0)
    z = np.frombuffer(b"\x03\x00", np.uint8)
    off, ooff, doff = np.array([0, 2], np.uint64), np.array([0, 64], np.uint64), np.array([0, 3, 6], np.uint64)
    d, out = np.frombuffer(b"abcdef", np.uint8), np.zeros(64, np.uint8)
    ln, st, of = np.zeros(1, np.uint64), np.zeros(1, np.int32), np.array([5], np.uint32)

    def call(container, n_dicts, dict_of):
        return eng._L.flate_hip_decompress_batch_dict(eng._h, z.ctypes.data, off.ctypes.data, 1, container, 0, out.ctypes.data,
                                                      ooff.ctypes.data, ln.ctypes.data, st.ctypes.data, None, 0, d.ctypes.data,
                                                      doff.ctypes.data, n_dicts, dict_of)
    assert call(1, 1, None) == -2          # gzip
    assert call(0, 2, None) == -2          # NULL dict_of with two dictionaries
    assert call(0, 2, of.ctypes.data) == -2  # index out of range
    assert call(0, 1, None) == 0 and st[0] == 0 and ln[0] == 0


# ---------------------------------------------------------------- the resumable inflater

def small_cases(container):
    return [c for c in dc.CASES if c.container == container and len(c.stream) <= 12000]


def give_dicts(inf, cases):
    """every stream its case's dictionary; True where it was applied"""
    groups = {}
    for i, c in enumerate(cases):
        if c.zdict is not None:
            groups.setdefault(c.zdict, []).append(i)
    for d, idx in groups.items():
        assert inf.set_dictionary(idx, d) == [True] * len(idx)


def feed_all(inf, cases, first):
    """first[i] bytes (not final), then the rest (final); returns (outputs, final statuses)"""
    cap = [len(c.out) + SLACK for c in cases]
    o1, s1, c1 = inf.feed([c.stream[:k] for c, k in zip(cases, first)], final=False, caps=cap)
    o2, s2, c2 = inf.feed([c.stream[u:] for c, u in zip(cases, c1)], final=True, caps=cap)
    for c, a, k, u in zip(cases, s1, first, c1):
        assert a in (NEED_INPUT, c.status), (c.name, a)
        assert u <= k
    return [a + b for a, b in zip(o1, o2)], s2


def check_fed(cases, outs, st, what):
    for c, o, s in zip(cases, outs, st):
        assert s == c.status, (c.name, what, s, c.status)
        if c.status == 1:  # (a stream that ends early has handed out what it had)
            assert o[:len(c.out)] == c.out, (c.name, what)
        else:
            assert o == c.out, (c.name, what)


@pytest.mark.parametrize("container", [0, 2])
def test_inflater_whole_and_every_early_split(container):
    """the cases of at most 12000 bytes: fed whole, and cut at every point of header + DICTID + the first 64 bytes"""
    eng = engine()
    cases = small_cases(container)
    assert len(cases) > 100 and any(c.status == WRONG_DICT for c in cases) == (container == 2)
    everyone = list(range(len(cases)))
    inf = eng.inflater(len(cases), container, flags=2)  # (FLATE_HIP_INFLATER_NEED_DICT: H_fdict_no_dictionary is 106)
    try:
        for k in [1 << 20] + list(range(1, 2 + 4 + 64 + 1)):
            give_dicts(inf, cases)
            outs, st = feed_all(inf, cases, [min(k, len(c.stream)) for c in cases])
            check_fed(cases, outs, st, k)
            inf.reset(everyone)
    finally:
        inf.close()


@pytest.mark.parametrize("container", [0, 2])
def test_inflater_one_byte_pieces_then_1000_byte_pieces_into_258_byte_slots(container):
    eng = engine()
    cases = small_cases(container)
    n = len(cases)
    inf = eng.inflater(n, container, flags=2)
    try:
        give_dicts(inf, cases)
        pos, outs, st = [0] * n, [b""] * n, [NEED_INPUT] * n
        for step in range(600):
            piece = 1 if step < 8 else 1000  # the first 8 bytes one at a time: header and DICTID cut everywhere
            live = [st[i] in (NEED_INPUT, NEED_OUTPUT) for i in range(n)]
            if not any(live):
                break
            pieces = [cases[i].stream[pos[i]:pos[i] + piece] if live[i] else None for i in range(n)]
            final = [live[i] and pos[i] + piece >= len(cases[i].stream) for i in range(n)]
            o, s, u = inf.feed(pieces, final=final, caps=258)
            for i in range(n):
                if live[i]:
                    outs[i] += o[i]
                    pos[i] += u[i]
                    st[i] = s[i]
        assert not any(s in (NEED_INPUT, NEED_OUTPUT) for s in st)
        check_fed(cases, outs, st, "pieces")
    finally:
        inf.close()


def test_inflater_set_dictionary_only_before_the_first_byte_and_reset_drops_it():
    eng = engine()
    need = dc.BY_NAME["Z_l6_w-15_d2048_r200"]    # raw: its first match reaches into the dictionary
    plain = dc.deflate(need.out, 6, -15, b"")    # the same record without one
    inf = eng.inflater(3, 0)
    try:
        # stream 0 takes the dictionary; streams 1 and 2 have absorbed a byte: refused, and they go on as they were
        o, s, u = inf.feed([None, plain[:1], need.stream[:1]], final=False, caps=[None, 1024, 1024])
        assert u[1:] == [1, 1] and s[1:] == [NEED_INPUT, NEED_INPUT]
        assert inf.set_dictionary([0, 1, 2], need.zdict) == [True, False, False]
        o, s, u = inf.feed([need.stream, plain[1:], need.stream[1:]], final=True, caps=1024)
        assert s == [0, 0, 11] and o[0] == need.out and o[1] == need.out
        # reset drops the dictionary of stream 0
        inf.reset([0, 1, 2])
        o, s, u = inf.feed([need.stream, plain, None], final=[True, True, False], caps=[1024, 1024, None])
        assert s[:2] == [11, 0] and o[1] == need.out
        # ... and a stream that is reset takes one again
        inf.reset([0, 1, 2])
        assert inf.set_dictionary([2], need.zdict) == [True]
        o, s, u = inf.feed([None, None, need.stream], final=[False, False, True], caps=[None, None, 1024])
        assert s[2] == 0 and o[2] == need.out
    finally:
        inf.close()


def test_inflater_need_dict_only_with_the_create_flag():
    eng = engine()
    c = dc.BY_NAME["H_right_id"]
    today, today_st, _ = eng.decompress_many([c.stream], 2, 0, [4096])  # FDICT ignored, DICTID taken for deflate data
    assert today_st[0] not in (0, NEED_DICT, WRONG_DICT)
    for flags, want in ((0, today_st[0]), (2, NEED_DICT)):
        inf = eng.inflater(1, 2, flags=flags)
        try:
            o, s, u = inf.feed([c.stream], final=True, caps=4096)
            assert s == [want], (flags, s)
            if flags:
                assert o == [b""]
                o, s, u = inf.feed([b"abc"], final=True, caps=4096)  # sticky
                assert s == [NEED_DICT] and u == [0] and o == [b""]
        finally:
            inf.close()
    # a wrong dictionary is sticky too
    inf = eng.inflater(1, 2)
    try:
        assert inf.set_dictionary([0], b"not the one") == [True]
        o, s, u = inf.feed([c.stream[:3]], final=False, caps=4096)
        assert s == [NEED_INPUT]
        o, s, u = inf.feed([c.stream[3:]], final=False, caps=4096)
        assert s == [WRONG_DICT] and o == [b""]
        o, s, u = inf.feed([c.stream], final=True, caps=4096)
        assert s == [WRONG_DICT] and u == [0]
    finally:
        inf.close()


# ---------------------------------------------------------------- the Python mirror

@pytest.mark.parametrize("piece", [None, 64, 1000])
def test_zdict_keyword(piece):
    from flate_amd import api, flate, gzip, zlib
    engine()
    for mod, tag in ((flate, "w-15"), (zlib, "w15")):
        for name in ("Z_l6_%s_d32768_r4096" % tag, "Z_l9_%s_d40000_r70000" % tag, "Z_l1_%s_d257_r200" % tag, "Z_l6_%s_d0_r200" % tag):
            c = dc.BY_NAME[name]
            d = mod.decompressor(io.BytesIO(c.stream), piece=piece, zdict=c.zdict)
            assert d.read() == c.out, name
            if piece is None:
                w = io.BytesIO()
                mod.decompress(c.stream, w, zdict=bytearray(c.zdict))
                assert w.getvalue() == c.out, name
    c = dc.BY_NAME["H_right_id"]
    with pytest.raises(api.WrongDict):
        zlib.decompressor(c.stream, piece=piece, zdict=b"some other dictionary").read()
    plain = dc.BY_NAME["H_no_fdict_with_dictionary"]
    assert zlib.decompressor(plain.stream, piece=piece, zdict=plain.zdict).read() == plain.out
    with pytest.raises(ValueError):
        gzip.decompressor(b"", piece=piece, zdict=b"abc")
    with pytest.raises(ValueError):
        gzip.decompress(b"", io.BytesIO(), zdict=b"abc")
