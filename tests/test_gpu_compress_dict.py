"""GPU tests of compressing records against preset dictionaries: flate_hip_compress_batch_dict on device and on host
memory, byte for byte against tests/_dict_compress_cases.py (whose expectations tests/test_dict_compress_cases_cpu.py
holds against stdlib zlib), back through flate_hip_decompress_batch_dict, the tokenizer's tokens against the oracle's
log, the errors of the call, and zdict= of the Python mirror's compress()."""
import io
import zlib as pyzlib

import numpy as np
import pytest

import _dict_compress_cases as dc
import _oracle as O
from gpu_util import engine

pytestmark = pytest.mark.gpu

NONE = 0xffffffff
FILL = 0xA5


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


def offsets(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


def run_device(eng, recs, dicts, of, container, mode, caps, n_dicts=None, with_of=True):
    """flate_hip_compress_batch_dict on device memory, slot i of caps[i] bytes.  Returns (rc, outs, statuses, whole buffer)."""
    import torch

    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()

    n = len(recs)
    t_in = dev(np.frombuffer(b"".join(recs) + b"\0", np.uint8))
    t_dict = dev(np.frombuffer(b"".join(dicts) + b"\0", np.uint8))
    t_inoff, t_doff, t_outoff = dev(offsets([len(r) for r in recs])), dev(offsets([len(d) for d in dicts])), dev(offsets(caps))
    t_of = dev(np.array([NONE if d is None else d for d in of], np.uint32).view(np.int32)) if with_of else None
    t_out = torch.full((int(sum(caps)) + 64,), FILL, dtype=torch.uint8, device="cuda")
    t_len = torch.zeros(n, dtype=torch.int64, device="cuda")
    t_st = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = eng.compress_dict_device(t_in.data_ptr(), t_inoff.data_ptr(), n, container, mode, t_out.data_ptr(), t_outoff.data_ptr(),
                                  t_len.data_ptr(), t_st.data_ptr(), t_dict.data_ptr(), t_doff.data_ptr(),
                                  len(dicts) if n_dicts is None else n_dicts, None if t_of is None else t_of.data_ptr())
    torch.cuda.synchronize()
    out, ln, st, off = t_out.cpu().numpy(), t_len.cpu().numpy(), t_st.cpu().numpy(), offsets(caps)
    outs = [out[int(off[i]): int(off[i]) + int(ln[i])].tobytes() for i in range(n)]
    return rc, outs, [int(s) for s in st], out


def slots(eng, recs, container, mode):
    return [(eng.compress_bound(len(r), container, mode) + 4 + 7) & ~7 for r in recs]


def check(names, outs, st, want):
    for name, o, s, w in zip(names, outs, st, want):
        assert s == 0, (name, s)
        assert len(o) == len(w), (name, len(o), len(w))
        assert o == w, name


def inflate_back(eng, outs, dicts, of, container, recs, names):
    """every output through flate_hip_decompress_batch_dict: the record, status 0, every byte consumed"""
    back, st, used = eng.decompress_many_dict(outs, dicts, of, container, caps=[len(r) + 8 for r in recs])
    for name, b, s, u, r, o in zip(names, back, st, used, recs, outs):
        assert s == 0 and b == r and u == len(o), (name, s, u, len(o))


# ---------------------------------------------------------------- every case, both tokenizer families, both memories

@pytest.mark.parametrize("container", dc.CONTAINERS)
@pytest.mark.parametrize("level", dc.LEVELS)
def test_every_case_on_device_memory(level, container):
    eng = engine()
    cases = dc.CASES
    names, recs = [c.name for c in cases], [c.rec for c in cases]
    dicts, of = tables(cases)
    want = [dc.expected(c.zdict, c.rec, level, container) for c in cases]
    rc, outs, st, _ = run_device(eng, recs, dicts, of, container, level, slots(eng, recs, container, level))
    assert rc == 0
    check(names, outs, st, want)
    inflate_back(eng, outs, dicts, of, container, recs, names)


@pytest.mark.parametrize("container", dc.CONTAINERS)
@pytest.mark.parametrize("level", dc.LEVELS)
def test_every_case_on_host_memory(level, container):
    eng = engine()
    cases = dc.CASES
    dicts, of = tables(cases)
    outs, st = eng.compress_many_dict([c.rec for c in cases], dicts, of, container, level)
    check([c.name for c in cases], outs, st, [dc.expected(c.zdict, c.rec, level, container) for c in cases])


@pytest.mark.parametrize("windows", ["0", "1"])
@pytest.mark.parametrize("level", [4, 6])
def test_every_case_on_the_windows_and_on_the_tiles(monkeypatch, level, windows):
    """levels 4..7 take the windows of k_lz_parse<true> or the sort / match tiles by an estimate: each of them forced"""
    monkeypatch.setenv("FLATE_HIP_STREAM_WINDOWS", windows)
    eng = engine()
    cases = dc.CASES
    dicts, of = tables(cases)
    outs, st = eng.compress_many_dict([c.rec for c in cases], dicts, of, O.RAW, level)
    check([c.name for c in cases], outs, st, [dc.expected(c.zdict, c.rec, level, O.RAW) for c in cases])


@pytest.mark.parametrize("level", [4, 6])
def test_tokens_are_the_oracles_from_the_flush_on(level):
    """flate_hip_debug_tokens after the call: the tokens of every stream are the oracle's log from the flush on -- nothing
    is emitted for the dictionary"""
    eng = engine()
    cases = dc.CASES
    dicts, of = tables(cases)
    _, st = eng.compress_many_dict([c.rec for c in cases], dicts, of, O.RAW, level)
    assert st == [0] * len(cases)
    for i, c in enumerate(cases):
        got, want = eng.debug_tokens(i), dc.expected_tokens(c.zdict, c.rec, level)
        assert len(got) == len(want) and (got == want).all(), c.name


# ---------------------------------------------------------------- the record shape, more streams than a pass holds

def test_records_against_one_shared_dictionary_over_two_passes():
    """2500 records of 200 bytes, one 32 KiB dictionary, dict_of = NULL: 2048 staged streams in the first pass, the rest
    in a second one"""
    eng = engine()
    d = dc.TEXT[20000:20000 + dc.WINDOW]
    recs = [d[(131 * i) % (dc.WINDOW - 200):][:200] for i in range(2500)]
    distinct = {r: dc.expected(d, r, 6, O.RAW) for r in set(recs)}
    rc, outs, st, _ = run_device(eng, recs, [d], [0] * len(recs), O.RAW, 6, slots(eng, recs, O.RAW, 6), with_of=False)
    assert rc == 0 and st == [0] * len(recs)
    assert all(o == distinct[r] for o, r in zip(outs, recs))
    assert sum(map(len, outs)) * 10 < sum(map(len, recs))  # (the dictionary is doing the work)


# ---------------------------------------------------------------- the mixed batch

@pytest.mark.parametrize("container", dc.CONTAINERS)
@pytest.mark.parametrize("level", [6, 9])
def test_mixed_batch(level, container):
    """dictionary 0, dictionary 1, none and the empty dictionary in one call: the streams without a dictionary are those
    of flate_hip_compress_batch"""
    eng = engine()
    recs, dicts, of = dc.mixed_batch()
    names = ["mixed%d" % i for i in range(len(recs))]
    want = [O.compress(r, container, level) if o is None else dc.expected(dicts[o], r, level, container) for r, o in zip(recs, of)]
    rc, outs, st, _ = run_device(eng, recs, dicts, of, container, level, slots(eng, recs, container, level))
    assert rc == 0
    check(names, outs, st, want)
    plain, pst = eng.compress_many([r for r, o in zip(recs, of) if o is None], container, level)
    assert plain == [x for x, o in zip(outs, of) if o is None] and pst == [0] * len(plain)
    if container == O.ZLIB:
        assert all((x[:2] == b"\x78\x9c") == (o is None) for x, o in zip(outs, of))
    inflate_back(eng, outs, dicts, of, container, recs, names)
    houts, hst = eng.compress_many_dict(recs, dicts, of, container, level)
    check(names, houts, hst, want)


# ---------------------------------------------------------------- errors

def test_errors():
    eng = engine()
    d = dc.TEXT[:4096]
    recs = [dc.TEXT[5000:5300], dc.TEXT[6000:6100]]
    caps = slots(eng, recs, O.RAW, 6)

    def untouched(buf):
        return (buf == FILL).all()

    rc, _, st, buf = run_device(eng, recs, [d], [0, 0], O.GZIP, 6, caps)
    assert rc == -2 and untouched(buf) and st == [-77, -77]  # gzip
    for mode in (0, 1):
        rc, _, st, buf = run_device(eng, recs, [d], [0, 0], O.RAW, mode, caps)
        assert rc == -2 and untouched(buf)
    rc, _, _, buf = run_device(eng, recs, [d, d], [0, 1], O.RAW, 6, caps, with_of=False)
    assert rc == -2 and untouched(buf)                       # dict_of == NULL with two dictionaries
    rc, _, _, buf = run_device(eng, recs, [d], [0, 1], O.RAW, 6, caps)
    assert rc == -2 and untouched(buf)                       # index out of range
    # min(dictionary, 32768) + record = 65536: the whole call does nothing
    for dl in (4096, 32768, 40000):
        dd = dc.TEXT[:dl]
        long_ = [recs[0], dc.TEXT[100:100 + 65536 - min(dl, 32768)]]
        lcaps = slots(eng, long_, O.ZLIB, 6)
        rc, _, st, buf = run_device(eng, long_, [dd], [0, 0], O.ZLIB, 6, lcaps)
        assert rc == -5 and untouched(buf) and st == [-77, -77], dl
        ok = [recs[0], long_[1][:-1]]                         # one byte less: it goes
        rc, outs, st, _ = run_device(eng, ok, [dd], [0, 0], O.ZLIB, 6, lcaps)
        assert rc == 0 and st == [0, 0] and outs[1] == dc.expected(dd, ok[1], 6, O.ZLIB)
        rc, outs, st, _ = run_device(eng, long_, [dd], [0, None], O.ZLIB, 6, lcaps)  # without a dictionary any length goes
        assert rc == 0 and st == [0, 0] and outs[1] == O.compress(long_[1], O.ZLIB, 6)
    with pytest.raises(ValueError):
        eng.compress_many_dict(recs, [d], None, O.GZIP, 6)
    with pytest.raises(ValueError):
        eng.compress_many_dict(recs, [d, d], None, O.RAW, 6)
    assert eng.compress_many_dict([], [d], None, O.RAW, 6) == ([], [])


@pytest.mark.parametrize("container", dc.CONTAINERS)
def test_tight_slots(container):
    """a slot exactly as long as its stream takes it; one byte less is status 100, nothing counted, and the neighbours'
    bytes are their own"""
    eng = engine()
    cases = [dc.BY_NAME[n] for n in ("shape_d16319_n300", "shape_d32768_n4", "straddle_k2", "no_match_noise", "shape_d0_n3", "same_byte_both")]
    recs = [c.rec for c in cases]
    dicts, of = tables(cases)
    want = [dc.expected(c.zdict, c.rec, 6, container) for c in cases]
    exact = [(len(w) + 3) & ~3 for w in want]
    rc, outs, st, _ = run_device(eng, recs, dicts, of, container, 6, exact)
    assert rc == 0
    check([c.name for c in cases], outs, st, want)
    # (every other slot short: a multiple of 4 below the stream's length -- the slot starts stay where the exact ones were
    # aligned --, and no room at all)
    for short in ([(len(w) - 1) & ~3 for w in want], [0 for w in want]):
        caps = [s if i % 2 == 0 else e for i, (s, e) in enumerate(zip(short, exact))]
        rc, outs, st, _ = run_device(eng, recs, dicts, of, container, 6, caps)
        assert rc == 0
        for i, (o, s, w) in enumerate(zip(outs, st, want)):
            if i % 2 == 0:
                assert s == 100 and o == b"", (cases[i].name, s)
            else:
                assert s == 0 and o == w, (cases[i].name, s)


# ---------------------------------------------------------------- the Python mirror

def test_zdict_keyword_of_compress():
    from flate_amd import api, flate, gzip, zlib
    engine()
    d = dc.TEXT[20000:20000 + 40000]
    for level in (api.Level.level_4, api.Level.default, api.Level.best):
        for rec in (b"", dc.TEXT[30000:30200], dc.TEXT[90000:90000 + 32767]):
            w = io.BytesIO()
            flate.compress(io.BytesIO(rec), w, api.Options(level), zdict=d)
            assert w.getvalue() == dc.expected(d, rec, int(level), O.RAW)
            o = pyzlib.decompressobj(-15, zdict=d[-32768:])
            assert o.decompress(w.getvalue()) == rec and o.eof
            w = io.BytesIO()
            zlib.compress(rec, w, api.Options(level), zdict=bytearray(d))
            assert w.getvalue() == dc.expected(d, rec, int(level), O.ZLIB)
            o = pyzlib.decompressobj(15, zdict=d)
            assert o.decompress(w.getvalue()) == rec and o.eof
            back = io.BytesIO()
            zlib.decompress(w.getvalue(), back, zdict=d)
            assert back.getvalue() == rec
    with pytest.raises(ValueError):
        gzip.compress(b"abc", io.BytesIO(), zdict=d)
    with pytest.raises(ValueError, match="65535"):
        flate.compress(dc.TEXT[:32768], io.BytesIO(), zdict=d)
    w = io.BytesIO()
    zlib.compress(b"abc", w)  # (without zdict= nothing has changed)
    assert w.getvalue() == O.compress(b"abc", O.ZLIB, 6)
