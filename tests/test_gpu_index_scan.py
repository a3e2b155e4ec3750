"""GPU tests of flate_hip_index_scan (k_index_scan, index_scan_plan.h): the fresh points of streams written elsewhere, found
without decoding, through ctypes on device and on host memory -- and what the rest of the seek index makes of the result
(export / import, flate_hip_decompress_ranges on the parts path).  The inputs, their marks and the expected points are
tests/_index_scan_cases.py, whose expectations tests/test_index_scan_cases_cpu.py holds against stdlib zlib."""
import ctypes as C
import zlib as pyzlib

import numpy as np
import pytest

import _index_cases as ic
import _index_scan_cases as sc
import _index_scan_plan as sp
import _joined_cases as jc
from gpu_util import engine
from test_gpu_seekable import DEVICE, E_INVALID_ARG, HOST, Mem, check_ranges, compress_indexed, count_parts, offsets

pytestmark = pytest.mark.gpu


class Batch:
    """streams back to back in memory of one kind"""

    def __init__(self, streams, kind):
        self.streams, self.kind, self.m, self.n = list(streams), kind, Mem(kind), len(streams)
        self.t_in = self.m.put(np.frombuffer(b"".join(self.streams) + b"\0", np.uint8))
        self.t_off = self.m.put(offsets([len(s) for s in self.streams]))

    def _results(self):
        m, n = self.m, self.n
        return m.put(np.full(n + 1, 777, np.uint64)), m.put(np.full(n + 1, -77, np.int32)), m.put(np.full(n + 1, 555, np.uint64))

    def _fetch(self, res):
        self.m.sync()
        return tuple([int(x) for x in self.m.get(r[0], d)] for r, d in zip(res, (np.uint64, np.int32, np.uint64)))

    def probe(self, eng, container):
        """what flate_hip_decompressed_sizes writes for the batch (the entry behind the last stays as it was)"""
        res = self._results()
        self.m.sync()
        eng._sync_env()
        rc = eng._L.flate_hip_decompressed_sizes(eng._h, self.t_in[1], self.t_off[1], self.n, container, 0, res[0][1], res[1][1],
                                                 res[2][1], self.kind)
        assert rc == 0
        return self._fetch(res)

    def scan(self, eng, container, spacing):
        res = self._results()
        self.m.sync()
        ix = eng.scan_index_device(self.t_in[1], self.t_off[1], self.n, container, 0, res[0][1], res[1][1], res[2][1], spacing, self.kind)
        return ix, self._fetch(res)


def groups(container):
    by = {}
    for c in sc.CASES:
        if c.container == container:
            by.setdefault(c.spacing, []).append(c)
    return sorted(by.items())


def check_index(eng, ix, cases, kind):
    """the points; export / import / export; the ranges around the points, fenced; the parts of the whole streams"""
    n = len(cases)
    for i, c in enumerate(cases):
        assert eng.index_info(ix, i) == (len(c.full), 0, len(c.points)), c.name
        assert eng.index_points(ix, i) == c.points, c.name
    blob = eng.index_export(ix)
    assert blob[4:8] == b"\x02\0\0\0" and len(blob) == 48 + 32 * n + 24 * sum(len(c.points) for c in cases)
    again = eng.index_import(blob)
    try:
        assert eng.index_export(again) == blob
        assert [eng.index_points(again, i) for i in range(n)] == [c.points for c in cases]
    finally:
        eng.index_destroy(again)
    comp, datas = [c.stream for c in cases], [c.full for c in cases]
    ranges = [(i, b, ln) for i, c in enumerate(cases) for b, ln in ic.make_ranges([p for _, p in c.points], len(c.full))]
    check_ranges(eng, ix, comp, datas, kind, ranges)
    whole = [(i, 0, len(c.full)) for i, c in enumerate(cases)]
    check_ranges(eng, ix, comp, datas, kind, whole)
    want = [count_parts([p for _, p in c.points], len(c.full), 0, len(c.full)) for c in cases]
    assert eng.index_parts() == (sum(d for d, _ in want), 0) and all(s == 0 for _, s in want)
    return max(d for d, _ in want)


# ---------------------------------------------------------------- every case

@pytest.mark.parametrize("kind", [DEVICE, HOST])
@pytest.mark.parametrize("container", [0, 1, 2])
def test_scan_gives_the_expected_points_and_the_probes_results(container, kind):
    """Per spacing one batch of all the container's cases with it: sizes, status and consumed are what
    flate_hip_decompressed_sizes writes for the batch, the points are block 0 and the fresh kept marks, bit and position;
    the blob is version 2 and survives a round trip; every range around the points delivers exactly full[b : b + L'] and
    nothing is written outside the delivered bytes; a range over several points is decoded in direct parts.  The batches
    at spacing 1 have room for more entries than are copied back unpacked, the others do not: both ways home run."""
    eng = engine()
    most, ways = 0, set()
    for spacing, cases in groups(container):
        # (every stream here is walked whole: the room for the lists says whether they come home as they are or packed)
        room = sum(sp.walk_entries(1 + len(c.full) // spacing, 8 * len(c.stream)) for c in cases)
        ways.add(room <= sp.copy_whole())
        batch = Batch([c.stream for c in cases], kind)
        base = batch.probe(eng, container)
        ix, got = batch.scan(eng, container, spacing)
        try:
            assert got == base, spacing
            assert got[0][:-1] == [len(c.full) for c in cases] and got[1][:-1] == [0] * len(cases)
            assert got[2][:-1] == [len(c.stream) for c in cases]
            most = max(most, check_index(eng, ix, cases, kind))
        finally:
            eng.index_destroy(ix)
    assert most >= 3 and ways == {True, False}


def test_host_and_device_memory_give_the_same_index():
    eng = engine()
    cases = [c for c in sc.CASES if c.container == 1 and c.spacing == 1]
    blobs = []
    for kind in (HOST, DEVICE):
        ix, _ = Batch([c.stream for c in cases], kind).scan(eng, 1, 1)
        blobs.append(eng.index_export(ix))
        eng.index_destroy(ix)
    assert blobs[0] == blobs[1]


# ---------------------------------------------------------------- spans

@pytest.mark.parametrize("kind", [DEVICE, HOST])
def test_long_stream_is_scanned_by_spans(monkeypatch, kind):
    """One gzip stream just long enough for the size probe's rule to cut it in two (FLATE_HIP_INFLATE_SPANS lowered to
    32 KiB), a sync flush every 2000 bytes and a full flush in each half: whichever block the cut lands on, a mark that is
    not fresh lies within 32 KiB in front of the second walk, whose matches reach in front of its start.  The points of the
    span walk are those of the walk by one wave and the expected ones, and the counter says which walk it was."""
    eng = engine()
    c = sc.span_case()
    batch = Batch([c.stream], kind)
    got = {}
    for knob in ("0", "32768"):
        monkeypatch.setenv("FLATE_HIP_INFLATE_SPANS", knob)
        base = batch.probe(eng, 1)
        ix, res = batch.scan(eng, 1, 1)
        try:
            assert res == base and res[0][0] == len(c.full) and res[1][0] == 0
            assert eng.index_paths() == ((0, 1) if knob == "0" else (1, 0))
            got[knob] = eng.index_points(ix, 0)
            check_index(eng, ix, [c], kind)
        finally:
            eng.index_destroy(ix)
    assert got["0"] == got["32768"] == c.points and 3 <= len(c.points) < len(c.marks)


# ---------------------------------------------------------------- joined streams

@pytest.mark.parametrize("container", jc.CONTAINERS)
def test_scan_of_a_joined_stream_finds_the_points_of_its_fresh_index(container):
    """the streams flate_hip_compress_joined_indexed wrote, scanned at the same spacing: every piece start behind the first is
    a mark, all of them are fresh, and the rule over the marks is the rule over the piece starts"""
    eng = engine()
    for piece in (4096, 7) if container == 1 else (4096,):
        names, streams = zip(*jc.batch(piece))
        for spacing in (1, 65535, 0):
            rc, jx, outs, st, _ = compress_indexed(eng, streams, piece, container, 6, spacing, DEVICE)
            assert rc == 0 and st == [0] * len(streams)
            ix, res = Batch(outs, DEVICE).scan(eng, container, spacing)
            try:
                assert res[0][:-1] == [len(s) for s in streams] and res[1][:-1] == [0] * len(streams)
                for i, name in enumerate(names):
                    assert eng.index_points(ix, i) == eng.index_points(jx, i), (name, piece, spacing)
                    assert eng.index_info(ix, i) == eng.index_info(jx, i), (name, piece, spacing)
                assert eng.index_export(ix) == eng.index_export(jx)
            finally:
                eng.index_destroy(ix)
                eng.index_destroy(jx)


# ---------------------------------------------------------------- failures and edges

def _invalid_match_behind_a_mark():
    """a good block, a marker, and behind it a match that reaches in front of the stream's first byte"""
    r = sc.Plant(99)
    r.history(300)
    r.marker()
    r.dynamic(sc.lits(r.s.rng, 40) + [("M", 5, 341)] + sc.lits(r.s.rng, 40), 1)
    raw, full = r.s.done()
    assert full is None
    return raw


@pytest.mark.parametrize("kind", [DEVICE, HOST])
def test_a_failing_stream_has_no_points_and_leaves_the_others_alone(kind):
    eng = engine()
    good = [sc.BY_NAME["P_two_marks_between_c0"], sc.BY_NAME["Z_c0_l6_s1"], sc.BY_NAME["P_far_dynamic_32768_c0"]]
    cut = sc.BY_NAME["Z_c0_l1_s1"].stream
    streams = [good[0].stream, cut[:len(cut) // 2], good[1].stream, _invalid_match_behind_a_mark(), good[2].stream, b""]
    batch = Batch(streams, kind)
    base = batch.probe(eng, 0)
    assert base[1][:-1] == [0, 1, 0, 11, 0, 1]  # EndOfStream, InvalidMatch
    ix, got = batch.scan(eng, 0, 1)
    try:
        assert got == base
        for i, c in ((0, good[0]), (2, good[1]), (4, good[2])):
            assert eng.index_info(ix, i) == (len(c.full), 0, len(c.points)) and eng.index_points(ix, i) == c.points, c.name
        for i in (1, 3, 5):
            assert eng.index_info(ix, i) == (0, base[1][i], 0) and eng.index_points(ix, i) == []
        blob = eng.index_export(ix)
        again = eng.index_import(blob)
        assert eng.index_export(again) == blob
        eng.index_destroy(again)
        datas = [good[0].full, b"", good[1].full, b"", good[2].full, b""]
        ranges = [(0, 5, 2000), (1, 0, 10), (2, 100000, 5000), (3, 0, 10), (4, 40000, 40000), (5, 0, 1)]
        check_ranges(eng, ix, streams, datas, kind, ranges, status_of=lambda j: base[1][j])
    finally:
        eng.index_destroy(ix)


def test_no_streams_and_no_index_pointer():
    eng = engine()
    m = Mem(DEVICE)
    z64, z32 = m.put(np.zeros(1, np.uint64)), m.put(np.zeros(1, np.int32))
    ix = eng.scan_index_device(None, z64[1], 0, 1, 0, z64[1], z32[1], None, 0, DEVICE)
    blob = eng.index_export(ix)
    assert len(blob) == 48 and blob[4:8] == b"\x02\0\0\0"
    assert eng.decompress_ranges_device(ix, None, z64[1], 0, 0, None, None, None, None, None, None, None, DEVICE) == 0
    eng.index_destroy(ix)
    c = sc.BY_NAME["P_two_marks_between_c0"]
    batch = Batch([c.stream], DEVICE)
    res = batch._results()
    rc = eng._L.flate_hip_index_scan(eng._h, batch.t_in[1], batch.t_off[1], 1, 0, 0, res[0][1], res[1][1], res[2][1], DEVICE, 1, None)
    assert rc == E_INVALID_ARG
    assert batch._fetch(res) == ([777, 777], [-77, -77], [555, 555])  # nothing ran
    ix = C.c_void_p(0xdead)
    rc = eng._L.flate_hip_index_scan(eng._h, batch.t_in[1], batch.t_off[1], 1, 3, 0, res[0][1], res[1][1], res[2][1], DEVICE, 1, C.byref(ix))
    assert rc == E_INVALID_ARG and not ix.value


# ---------------------------------------------------------------- the Python mirror and the tool

def _full_flushed_gzip(data, every):
    co = pyzlib.compressobj(6, pyzlib.DEFLATED, 31)
    out = b""
    for a in range(0, len(data), every):
        out += co.compress(data[a:a + every]) + co.flush(pyzlib.Z_FULL_FLUSH)
    return out + co.flush()


def test_python_mirror_and_cli(tmp_path, capfdbinary):
    """gzip.scan_index, and tools/gunzip.py --scan-index FILE, whose file --index FILE --range reads back; nothing is decoded
    into a file by the scan"""
    import importlib.util
    import os
    from conftest import ROOT
    from flate_amd import gzip
    engine()
    data = ic.TEXT[:300000]
    z = _full_flushed_gzip(data, 50000)
    ix = gzip.scan_index(z, spacing=60000)
    assert ix.size == len(data) and [p for _, p in ix.points()] == [0, 100000, 150000, 200000, 250000, 300000]
    assert ix.read_at(123456, 100000) == data[123456:223456] and ix.read_at(299990, 100) == data[299990:]
    blob = ix.to_bytes()
    again = gzip.index_from_bytes(blob, z)
    assert again.points() == ix.points() and again.read_at(5, 5) == data[5:10]
    ix.close()
    again.close()
    with pytest.raises(Exception):
        gzip.scan_index(z[:len(z) // 2])
    spec = importlib.util.spec_from_file_location("gunzip_cli_scan", os.path.join(ROOT, "tools", "gunzip.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    gz, idx = tmp_path / "a.txt.gz", tmp_path / "a.idx"
    gz.write_bytes(z)
    assert cli.main(["--scan-index", str(idx), "--spacing", "60000", str(gz)]) == 0
    assert idx.read_bytes() == blob and not (tmp_path / "a.txt").exists()
    capfdbinary.readouterr()
    assert cli.main(["--index", str(idx), "--range", "150000:1234", str(gz)]) == 0
    assert capfdbinary.readouterr().out == data[150000:151234]
    assert cli.main(["--scan-index", str(idx), "--spacing", "0", str(gz)]) == 2
