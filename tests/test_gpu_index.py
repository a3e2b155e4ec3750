"""GPU tests of the seek index: flate_hip_index_build (k_index_walk, k_index_windows), flate_hip_decompress_ranges
(k_inflate_range on both LDS rings, k_range_pack), export / import and the Python mirror, through ctypes on device and on
host memory.  The inputs, where their blocks start and the ranges asked of them are tests/_index_cases.py, whose expectations
tests/test_index_cases_cpu.py holds against stdlib zlib."""
import ctypes as C
import zlib as pyzlib

import numpy as np
import pytest

import _index_cases as ic
from gpu_util import engine

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1
E_INVALID_ARG = -2
SLACK = 264
FILL = 0xAA


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


def offsets(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.array(lens, np.uint64))
    return off


def cap_of(c):
    return (len(c.full) + SLACK + 7) & ~7 if c.status == 0 else 50000 + SLACK


class Batch:
    """the streams of some cases in memory of one kind, with output slots that hold them"""

    def __init__(self, cases, kind):
        self.cases, self.mem, self.n = cases, Mem(kind), len(cases)
        self.in_off = offsets([len(c.stream) for c in cases])
        self.out_off = offsets([cap_of(c) for c in cases])
        self.h_in, self.p_in = self.mem.put(np.frombuffer(b"".join(c.stream for c in cases) + b"\0", np.uint8))
        self.h_inoff, self.p_inoff = self.mem.put(self.in_off)
        self.h_outoff, self.p_outoff = self.mem.put(self.out_off)

    def results(self):
        m = self.mem
        return (m.put(np.full(int(self.out_off[-1]) + 64, FILL, np.uint8)), m.put(np.zeros(self.n, np.uint64)),
                m.put(np.full(self.n, -77, np.int32)), m.put(np.zeros(self.n, np.uint64)))

    def fetch(self, res):
        m = self.mem
        m.sync()
        return (m.get(res[0][0], np.uint8), m.get(res[1][0], np.uint64), m.get(res[2][0], np.int32), m.get(res[3][0], np.uint64))

    def decompress(self, eng, container):
        res = self.results()
        rc = eng._L.flate_hip_decompress_batch(eng._h, self.p_in, self.p_inoff, self.n, container, 0, res[0][1], self.p_outoff,
                                               res[1][1], res[2][1], res[3][1], self.mem.kind)
        assert rc == 0
        return self.fetch(res)

    def build(self, eng, container, spacing):
        res = self.results()
        ix = eng.index_build_device(self.p_in, self.p_inoff, self.n, container, 0, res[0][1], self.p_outoff, res[1][1], res[2][1],
                                    res[3][1], spacing, self.mem.kind)
        return ix, self.fetch(res)

    def ranges(self, eng, ix, ranges, caps, n_streams=None, in_off=None):
        """ranges: [(stream, begin, len)], caps: the slots' sizes -> (rc, out, out_len, status, slot starts)"""
        m, n = self.mem, len(ranges)
        starts = offsets(caps)
        rs = m.put(np.array([r[0] for r in ranges] + [0], np.uint32))
        rb = m.put(np.array([r[1] for r in ranges] + [0], np.uint64))
        rl = m.put(np.array([r[2] for r in ranges] + [0], np.uint64))
        so = m.put(starts)
        out = m.put(np.full(int(starts[-1]) + 64, FILL, np.uint8))
        ln = m.put(np.full(n + 1, 12345, np.uint64))
        st = m.put(np.full(n + 1, -77, np.int32))
        p_inoff = self.p_inoff if in_off is None else m.put(in_off)
        if in_off is not None:
            self._keep, p_inoff = p_inoff
        m.sync()
        rc = eng.decompress_ranges_device(ix, self.p_in, p_inoff, self.n if n_streams is None else n_streams, n, rs[1], rb[1], rl[1],
                                          out[1], so[1], ln[1], st[1], m.kind)
        m.sync()
        return rc, m.get(out[0], np.uint8), m.get(ln[0], np.uint64), m.get(st[0], np.int32), starts


def groups(container):
    """the cases of a container by spacing"""
    by = {}
    for c in ic.CASES:
        if c.container == container:
            by.setdefault(c.spacing, []).append(c)
    return sorted(by.items())


_baseline = {}


def baseline(eng, container, spacing, kind):
    """what flate_hip_decompress_batch writes for a group's batch: computed once, never changed"""
    key = (container, spacing, kind)
    if key not in _baseline:
        cases = dict(groups(container))[spacing]
        _baseline[key] = tuple(a.copy() for a in Batch(cases, kind).decompress(eng, container))
    return _baseline[key]


def check_points(eng, ix, cases, spacing):
    for i, c in enumerate(cases):
        size, st, npts = eng.index_info(ix, i)
        got = eng.index_points(ix, i)
        assert st == c.status, (c.name, st)
        if c.status != 0:
            assert (size, npts, got) == (0, 0, []), c.name
            continue
        assert size == len(c.full), c.name
        which = ic.point_rule(c.block_pos, spacing)
        assert [p for _, p in got] == [c.block_pos[k] for k in which], c.name
        assert len(got) <= 1 + size // spacing
        if c.block_starts:
            assert got == [c.block_starts[k] for k in which], c.name
        else:  # the bits are not known: each must be a block start by the shift-and-reinflate property
            for bit, pos in got:
                assert ic.shift_and_reinflate(c.stream, bit, pos, c.full), (c.name, bit, pos)


def expected_range(c, begin, length, cap):
    """(status, bytes) of one range of a case"""
    if c.status != 0:
        return c.status, b""
    want = c.full[begin:begin + length] if begin < len(c.full) else b""
    if len(want) > cap:
        return 100, b""
    return 0, want


def check_ranges(eng, batch, ix, cases, tight=0):
    """every case's ranges in one call: slots at every alignment, fenced by the fill; tight = 1: every third slot of a range
    that delivers something is one byte too small"""
    ranges, caps, want = [], [], []
    for i, c in enumerate(cases):
        for b, n in c.ranges:
            lp = len(expected_range(c, b, n, 1 << 62)[1])
            cap = lp + (len(ranges) * 7) % 18  # (slot starts take every residue mod 16)
            if tight and lp and len(ranges) % 3 == 0:
                cap = lp - 1
            ranges.append((i, b, n))
            caps.append(cap)
            want.append(expected_range(c, b, n, cap))
    rc, out, ln, st, starts = batch.ranges(eng, ix, ranges, caps)
    assert rc == 0
    assert set(int(s) & 15 for s in starts[:-1]) == set(range(16)) or len(ranges) < 64
    clean = np.full(out.size, FILL, np.uint8)
    for j, (r, (status, data)) in enumerate(zip(ranges, want)):
        assert int(st[j]) == status and int(ln[j]) == len(data), (cases[r[0]].name, r, int(st[j]), int(ln[j]), status, len(data))
        a = int(starts[j])
        assert out[a:a + len(data)].tobytes() == data, (cases[r[0]].name, r)
        clean[a:a + len(data)] = out[a:a + len(data)]
    assert np.array_equal(out, clean), "a byte outside the delivered bytes of a slot was written"
    assert int(ln[len(ranges)]) == 12345 and int(st[len(ranges)]) == -77


# ---------------------------------------------------------------- build

@pytest.mark.parametrize("kind", [DEVICE, HOST])
@pytest.mark.parametrize("container", [0, 1, 2])
def test_build_is_decompress_plus_the_expected_points(container, kind):
    """Per spacing one batch of all the container's cases with it: out, out_len, status and consumed are what
    flate_hip_decompress_batch writes for the batch; synthesized cases have exactly the expected points, zlib-made ones the
    expected positions at bits that are block starts; failing streams have none."""
    eng = engine()
    for spacing, cases in groups(container):
        base = baseline(eng, container, spacing, kind)
        batch = Batch(cases, kind)
        ix, got = batch.build(eng, container, spacing)
        try:
            for a, b in zip(got[1:], base[1:]):
                assert np.array_equal(a, b), (spacing, a, b)
            for i, c in enumerate(cases):  # the decoded bytes (beyond out_len a slot is unspecified)
                lo = int(batch.out_off[i])
                assert np.array_equal(got[0][lo:lo + int(got[1][i])], base[0][lo:lo + int(base[1][i])]), c.name
                if c.status == 0:
                    assert got[0][lo:lo + len(c.full)].tobytes() == c.full and int(got[3][i]) == len(c.stream), c.name
            check_points(eng, ix, cases, spacing)
        finally:
            eng.index_destroy(ix)


@pytest.mark.parametrize("container", [0, 1, 2])
def test_one_batch_of_all_cases(container):
    """every case of a container side by side under one spacing that is none of their own"""
    eng = engine()
    cases = [c for c in ic.CASES if c.container == container]
    assert len(cases) >= 8
    batch = Batch(cases, DEVICE)
    ix, got = batch.build(eng, container, 3000)
    try:
        assert [int(s) for s in got[2]] == [c.status for c in cases]
        check_points(eng, ix, cases, 3000)
        check_ranges(eng, batch, ix, cases)
    finally:
        eng.index_destroy(ix)


def test_default_spacing_and_empty_batch():
    eng = engine()
    c = ic.BY_NAME["S_big_random_0"]
    batch = Batch([c], DEVICE)
    ix, _ = batch.build(eng, c.container, 0)
    try:
        which = ic.point_rule(c.block_pos, 1 << 20)
        assert eng.index_points(ix, 0) == [c.block_starts[k] for k in which]
    finally:
        eng.index_destroy(ix)
    # no streams: an empty index (the pointers are looked at as flate_hip_decompress_batch looks at them)
    m = Mem(DEVICE)
    z64, z32 = m.put(np.zeros(1, np.uint64)), m.put(np.zeros(1, np.int32))
    ix = eng.index_build_device(None, z64[1], 0, 1, 0, None, z64[1], z64[1], z32[1], None, 0, DEVICE)
    assert len(eng.index_export(ix)) == 48
    assert eng.decompress_ranges_device(ix, None, z64[1], 0, 0, None, None, None, None, None, None, None, DEVICE) == 0
    eng.index_destroy(ix)


# ---------------------------------------------------------------- spans

@pytest.mark.parametrize("kind", [DEVICE, HOST])
def test_long_stream_is_walked_by_spans(monkeypatch, kind):
    """One stream just long enough for the size probe's rule to cut it in two (32 KiB compressed, FLATE_HIP_INFLATE_SPANS
    lowered to that), made of Z_BLOCK cuts so that its block positions are known: the points of the span walk are those of
    the walk by one wave, and the counter says which walk it was."""
    eng = engine()
    data = ic.TEXT[:150000]
    cuts = list(range(10000, 150000, 10000))
    stream, pos = ic.zlib_segments(data, cuts, [pyzlib.Z_BLOCK] * len(cuts), 6, 31)
    assert 32768 <= len(stream) < 2 * 32768 and len(pos) == 15
    spacing = 16384
    pts = [pos[k] for k in ic.point_rule(pos, spacing)]
    c = ic.Case("Z_spans", 1, stream, data, spacing, 0, None, pos, ic.make_ranges(pts, len(data)))
    batch = Batch([c], kind)
    got = {}
    for knob in ("0", "32768"):
        monkeypatch.setenv("FLATE_HIP_INFLATE_SPANS", knob)
        ix, res = batch.build(eng, 1, spacing)
        try:
            assert int(res[2][0]) == 0 and res[0][:len(data)].tobytes() == data
            assert eng.index_paths() == ((0, 1) if knob == "0" else (1, 0))
            check_points(eng, ix, [c], spacing)
            got[knob] = eng.index_points(ix, 0)
            check_ranges(eng, batch, ix, [c])
        finally:
            eng.index_destroy(ix)
    assert got["0"] == got["32768"] and len(got["0"]) == len(pts) >= 5


# ---------------------------------------------------------------- ranges

@pytest.mark.parametrize("ring", [2048, 32768])
@pytest.mark.parametrize("kind", [DEVICE, HOST])
@pytest.mark.parametrize("container", [0, 1, 2])
def test_ranges_of_every_case(monkeypatch, container, kind, ring):
    """Every case's ranges, per spacing in one call, on both instances of k_inflate_range (FLATE_HIP_INFLATE_RING): exactly
    full[b : b + L'], the right out_len and status (a failed stream's build status), nothing written outside the delivered
    bytes."""
    monkeypatch.setenv("FLATE_HIP_INFLATE_RING", str(ring))
    eng = engine()
    for spacing, cases in groups(container):
        batch = Batch(cases, kind)
        ix, _ = batch.build(eng, container, spacing)
        try:
            check_ranges(eng, batch, ix, cases)
        finally:
            eng.index_destroy(ix)


@pytest.mark.parametrize("kind", [DEVICE, HOST])
def test_slot_one_byte_too_small(kind):
    eng = engine()
    for container in (0, 1):
        spacing, cases = groups(container)[0]
        batch = Batch(cases, kind)
        ix, _ = batch.build(eng, container, spacing)
        try:
            check_ranges(eng, batch, ix, cases, tight=1)
        finally:
            eng.index_destroy(ix)


def test_argument_errors():
    eng = engine()
    cases = [ic.BY_NAME["S_dist32768"], ic.BY_NAME["S_grid_edges"]]
    batch = Batch(cases, DEVICE)
    ix, _ = batch.build(eng, 0, 1000)
    try:
        ok = [(0, 5, 10), (1, 5, 10)]
        assert batch.ranges(eng, ix, ok, [10, 10])[0] == 0
        assert batch.ranges(eng, ix, ok, [10, 10], n_streams=1)[0] == E_INVALID_ARG
        assert batch.ranges(eng, ix, ok, [10, 10], n_streams=3)[0] == E_INVALID_ARG
        off = batch.in_off.copy()
        off[1] -= 1  # the same bytes cut elsewhere: both lengths differ from the index's
        assert batch.ranges(eng, ix, ok, [10, 10], in_off=off)[0] == E_INVALID_ARG
        assert batch.ranges(eng, ix, [(2, 0, 1)], [1])[0] == E_INVALID_ARG
        assert batch.ranges(eng, ix, [(0, 0, 1), (0xffffffff, 0, 1)], [1, 1])[0] == E_INVALID_ARG
        rc, out, ln, st, _ = batch.ranges(eng, ix, [], [])
        assert rc == 0 and int(ln[0]) == 12345 and np.all(out == FILL)
    finally:
        eng.index_destroy(ix)


def test_many_ranges_in_passes_under_a_small_budget(monkeypatch):
    """FLATE_HIP_INDEX_PASS_BYTES: a call whose ranges need more scratch than a pass may hold runs in several passes, with
    the same results; the scratch is workspace of the handle."""
    eng = engine()
    c = ic.BY_NAME["S_big_random_0"]
    batch = Batch([c], DEVICE)
    ix, _ = batch.build(eng, c.container, 8192)
    try:
        size = len(c.full)
        rng = np.random.default_rng(5)
        ranges = [(0, int(b), 3000) for b in rng.integers(0, size - 3000, 200)]
        one = batch.ranges(eng, ix, ranges, [3000] * len(ranges))
        assert one[0] == 0 and eng.index_passes() == 1
        monkeypatch.setenv("FLATE_HIP_INDEX_PASS_BYTES", str(256 * 1024))
        many = batch.ranges(eng, ix, ranges, [3000] * len(ranges))
        assert many[0] == 0 and eng.index_passes() >= 3
        for j, (_, b, n) in enumerate(ranges):
            assert int(many[3][j]) == 0 and int(many[2][j]) == n
            assert many[1][3000 * j:3000 * j + n].tobytes() == c.full[b:b + n]
        assert np.array_equal(one[1], many[1])
        # one range alone beyond the budget is a pass of its own, and the handle's workspace holds its scratch
        monkeypatch.setenv("FLATE_HIP_INDEX_PASS_BYTES", "4096")
        big = batch.ranges(eng, ix, [(0, 10, 100000), (0, 50, 100000)], [100000, 100000])
        assert big[0] == 0 and eng.index_passes() == 2 and [int(x) for x in big[3][:2]] == [0, 0]
        assert big[1][:100000].tobytes() == c.full[10:100010] and big[1][100000:200000].tobytes() == c.full[50:100050]
        assert eng.workspace_bytes() >= 100000
    finally:
        eng.index_destroy(ix)


def test_the_skip_may_be_long():
    """S_one_long_fixed: one block of 264 KiB, spacing 4096, one point: a range at the end decodes all of it"""
    eng = engine()
    c = ic.BY_NAME["S_one_long_fixed"]
    batch = Batch([c], DEVICE)
    ix, _ = batch.build(eng, 0, c.spacing)
    try:
        assert eng.index_points(ix, 0) == [(0, 0)]
        n = len(c.full)
        rc, out, ln, st, _ = batch.ranges(eng, ix, [(0, n - 300, 300)], [300])
        assert rc == 0 and int(st[0]) == 0 and int(ln[0]) == 300 and out[:300].tobytes() == c.full[-300:]
        assert eng.workspace_bytes() >= n
    finally:
        eng.index_destroy(ix)


# ---------------------------------------------------------------- export / import

def test_export_import_on_a_fresh_handle():
    from flate_amd import Engine
    from flate_amd._capi import FlateHipError
    eng = engine()
    cases = [c for c in ic.CASES if c.container == 1]
    batch = Batch(cases, DEVICE)
    ix, _ = batch.build(eng, 1, 2000)
    info = [eng.index_info(ix, i) for i in range(len(cases))]
    pts = [eng.index_points(ix, i) for i in range(len(cases))]
    blob = eng.index_export(ix)
    eng.index_destroy(ix)
    assert len(blob) == 48 + 32 * len(cases) + 24 * sum(map(len, pts)) + sum(min(p, 32768) for q in pts for _, p in q)
    other = Engine(0)
    try:
        ix2 = other.index_import(blob)
        assert [other.index_info(ix2, i) for i in range(len(cases))] == info
        assert [other.index_points(ix2, i) for i in range(len(cases))] == pts
        assert other.index_export(ix2) == blob
        check_ranges(other, batch, ix2, cases)
        # host memory on the fresh handle: nothing of the streams is on its device yet, and only what the decodes can consume
        # is staged -- a byte too few and a range does not decode
        check_ranges(other, Batch(cases, HOST), ix2, cases)
        other.index_destroy(ix2)
        for bad in (blob[:-1], blob[:47], blob[:100], b"", blob + b"\0",
                    blob[:4] + bytes([blob[4] ^ 1]) + blob[5:],    # the version
                    blob[:3] + bytes([blob[3] ^ 0x40]) + blob[4:]):  # the magic
            with pytest.raises(FlateHipError, match="-2"):
                other.index_import(bad)
    finally:
        other.close()


# ---------------------------------------------------------------- the Python mirror

def test_cli_index_and_range(tmp_path, capfdbinary):
    """tools/gunzip.py --index FILE writes the index beside the normal output, and with --range reads from it"""
    import importlib.util
    import os
    from conftest import ROOT
    engine()
    spec = importlib.util.spec_from_file_location("gunzip_cli", os.path.join(ROOT, "tools", "gunzip.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    data = ic.TEXT[:200000]
    gz, idx = tmp_path / "a.txt.gz", tmp_path / "a.idx"
    gz.write_bytes(_gzip(data))
    assert cli.main(["--index", str(idx), str(gz)]) == 0
    assert (tmp_path / "a.txt").read_bytes() == data and idx.stat().st_size >= 48
    capfdbinary.readouterr()
    assert cli.main(["--index", str(idx), "--range", "150000:1234", str(gz)]) == 0
    assert capfdbinary.readouterr().out == data[150000:151234]
    assert cli.main(["--index", str(idx), "--range", "x:1", str(gz)]) == 2
    (tmp_path / "a.txt").unlink()  # the index is there and no range is asked for: a normal decode
    assert cli.main(["--index", str(idx), str(gz)]) == 0 and (tmp_path / "a.txt").read_bytes() == data


def _gzip(data):
    co = pyzlib.compressobj(6, pyzlib.DEFLATED, 31)
    return co.compress(data) + co.flush()


def test_python_mirror():
    from flate_amd import flate, gzip, zlib as fzlib
    engine()
    data = ic.TEXT[:700000]
    for mod, wbits in ((gzip, 31), (fzlib, 15), (flate, -15)):
        co = pyzlib.compressobj(6, pyzlib.DEFLATED, wbits)
        z = co.compress(data) + co.flush()
        ix = mod.build_index(z, spacing=65536)
        assert ix.size == len(data)
        pts = ix.points()
        assert pts[0][1] == 0 and 2 <= len(pts) <= 1 + len(data) // 65536
        for a, b in ((0, 10), (65536, 65546), (123457, 400001), (len(data) - 5, len(data) + 100), (len(data), len(data) + 1)):
            assert ix.read_at(a, b - a) == data[a:b]
        assert ix.read_ranges([(5, 5), (600000, 70000)]) == [data[5:10], data[600000:670000]]
        again = mod.index_from_bytes(ix.to_bytes(), z)
        assert again.size == ix.size and again.points() == pts and again.to_bytes() == ix.to_bytes()
        assert again.read_at(300000, 1000) == data[300000:301000]
        ix.close()
        again.close()
