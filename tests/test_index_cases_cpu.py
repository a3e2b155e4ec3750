"""The seek index, the part that needs no GPU: the inputs of tests/test_gpu_index.py (tests/_index_cases.py) against stdlib
zlib, and the new names of the C ABI and its Python mirror."""
import os
import zlib

import _index_cases as ic
from conftest import ROOT

WBITS = {0: -15, 1: 31, 2: 15}


def inflate(c):
    d = zlib.decompressobj(WBITS[c.container])
    try:
        out = d.decompress(c.stream)
    except zlib.error:
        return None
    return out if d.eof else None


def all_points():
    """(case, bit or None, pos) of every expected point"""
    return [(c, b, p) for c in ic.CASES for b, p in ic.expected_points(c)]


def test_every_valid_case_is_what_zlib_inflates_it_to():
    for c in ic.CASES:
        if c.status == 0:
            assert inflate(c) == c.full, c.name
        else:
            assert inflate(c) is None and c.full == b"", c.name


def test_block_positions_are_stream_order():
    for c in ic.CASES:
        assert c.block_pos[0] == 0 and all(a <= b for a, b in zip(c.block_pos, c.block_pos[1:])), c.name
        assert c.block_pos[-1] <= len(c.full) or c.status != 0, c.name
        if c.block_starts:
            assert [p for _, p in c.block_starts] == c.block_pos, c.name
            bits = [b for b, _ in c.block_starts]
            assert bits[0] == 8 * ic.HEADER_BYTES[c.container] and all(a < b for a, b in zip(bits, bits[1:])), c.name
        pts = ic.expected_points(c)
        assert all(a[1] < b[1] for a, b in zip(pts, pts[1:])) and len(pts) <= 1 + len(c.full) // c.spacing, c.name
        assert (len(pts) == 0) == (c.status != 0), c.name


def test_every_point_with_known_bits_is_a_block_start_by_shift_and_reinflate():
    seen = 0
    for c, bit, pos in all_points():
        if bit is None:
            continue
        assert ic.shift_and_reinflate(c.stream, bit, pos, c.full), (c.name, bit, pos)
        seen += 1
    assert seen == sum(len(ic.expected_points(c)) for c in ic.CASES if c.block_starts) > 800
    # ... and the property tells: one bit off, it fails
    c = ic.BY_NAME["S_dist32768"]
    bit, pos = ic.expected_points(c)[1]
    assert not ic.shift_and_reinflate(c.stream, bit + 1, pos, c.full)
    assert not ic.shift_and_reinflate(c.stream, bit, pos + 1, c.full)


def test_point_rule_restatement():
    assert ic.point_rule([0], 5) == [0]
    assert ic.point_rule([0, 0, 0, 5, 5, 9, 10, 30], 5) == [0, 3, 6, 7]
    assert ic.point_rule([0, 4, 4, 6], 5) == [0, 3]
    assert ic.point_rule([0, 1, 1, 2], 1) == [0, 1, 3]


def test_what_the_cases_cover_together():
    pts = all_points()
    assert set(b & 7 for _, b, _ in pts if b is not None) == set(range(8))
    assert any(0 < p < ic.WINDOW for _, _, p in pts) and any(p > ic.WINDOW for _, _, p in pts)
    # a point followed at once by a match of distance 32768 (S_dist32768: built so) resp. of distance out_pos
    c = ic.BY_NAME["S_dist32768"]
    assert [p for _, p in ic.expected_points(c)] == [0, 40000, 80000, 120000]
    assert c.full[40000:40100] == c.full[40000 - 32768:40100 - 32768]
    assert c.full[80000:80200] == (c.full[80000 - 7:80000] * 30)[:200]  # distance 7, length 200: runs on into its own bytes
    c = ic.BY_NAME["S_dist_eq_pos"]
    assert [p for _, p in ic.expected_points(c)] == [0, 1000, 2000] and c.full[1000:1050] == c.full[:50]
    assert c.full[2000:2258] == (c.full[1997:2000] * 86)[:258]
    # a stored block that begins at a point; a sync flush's empty stored block that is the point
    c = ic.BY_NAME["S_stored_at_points"]
    assert [p for _, p in ic.expected_points(c)] == [0, 5000, 10000, 75535]
    for bit, pos in ic.expected_points(c)[1:]:
        assert (c.stream[bit >> 3] >> (bit & 7)) & 6 == 0  # BTYPE 00
    c = ic.BY_NAME["Z_sync_is_point"]
    assert c.block_pos == [0, 10000, 10000, 20000, 20000] and ic.point_rule(c.block_pos, c.spacing) == [0, 1, 3]
    # one long fixed block: only point 0, and a range at its end
    c = ic.BY_NAME["S_one_long_fixed"]
    assert len(c.full) == 264193 and c.spacing == 4096 and ic.expected_points(c) == [(0, 0)]
    assert (len(c.full) - 300, 300) in c.ranges
    # hundreds of blocks of a few bytes, spacing 1: every block behind a non-empty one is a point
    c = ic.BY_NAME["S_tiny300_c0"]
    assert len(c.block_pos) == 300 and c.spacing == 1
    assert len(ic.expected_points(c)) == 1 + sum(a < b for a, b in zip(c.block_pos, c.block_pos[1:])) > 200
    # grid edges, the empty stream, one block, wrong footers
    assert [p for _, p in ic.expected_points(ic.BY_NAME["S_grid_edges"])] == [0, 1000, 3001, 4000, 5000, 7000]
    for k in range(3):
        assert ic.BY_NAME["S_empty_c%d" % k].full == b"" and len(ic.expected_points(ic.BY_NAME["S_empty_c%d" % k])) == 1
    assert len(ic.BY_NAME["S_one_block"].block_pos) == 1
    assert ic.BY_NAME["Z_bad_crc"].status == 4 and ic.BY_NAME["Z_bad_adler"].status == 6
    # sizes: every stream stays under about 1 MiB of output
    assert max(len(c.full) for c in ic.CASES) <= 1 << 20
    assert sorted(set(c.container for c in ic.CASES)) == [0, 1, 2]


def test_ranges_of_every_case():
    for c in ic.CASES:
        size, pts = len(c.full), [p for _, p in ic.expected_points(c)]
        assert len(c.ranges) <= 300, c.name
        begins = set(b for b, _ in c.ranges)
        assert {0, size, size + 100} <= begins and any(n == 0 for _, n in c.ranges) and (0, size) in c.ranges, c.name
        for p in pts[:3]:
            assert p in begins and p + 1 in begins and (p == 0 or p - 1 in begins), c.name
        if size:
            assert size - 1 in begins, c.name
        if len(pts) >= 4:  # one range crosses at least three points
            assert any(sum(b < p < b + n for p in pts) >= 3 for b, n in c.ranges), c.name


def test_zlib_made_streams_hold_one_marker_per_sync_or_full_flush():
    """Every sync or full flush of a Family Z stream leaves its empty stored block, 00 00 ff ff, in the stream, and nothing
    else does: the markers are counted against the flushes of every Z case.  (That a segment is ONE block is not checked
    here -- stdlib zlib does not show block boundaries; it rests on zlib closing a block by itself only when 16383
    symbols are used up, and is confirmed where the GPU build returns points at exactly these positions whose bits pass
    shift_and_reinflate.)"""
    assert len(ic.Z_FLUSHES) >= 7
    for name, n in ic.Z_FLUSHES.items():
        assert ic.BY_NAME[name].stream.count(b"\x00\x00\xff\xff") == n, name
    assert ic.Z_FLUSHES["Z_sync_is_point"] == 2 and sum(ic.Z_FLUSHES.values()) > 100


def test_new_symbols_and_python_surface():
    from flate_amd import _capi, flate, gzip, zlib as fzlib
    from flate_amd.engine import Engine
    L = _capi.lib()
    for s in ("flate_hip_index_build", "flate_hip_index_destroy", "flate_hip_index_stream_info", "flate_hip_index_points",
              "flate_hip_index_export_size", "flate_hip_index_export", "flate_hip_index_import", "flate_hip_decompress_ranges"):
        assert s in _capi.SYMBOLS and hasattr(L, s), s
    hdr = open(os.path.join(ROOT, "include", "flate_hip.h")).read()
    for text in ("Not covered:", "NO CHECKSUM", "WAITS ON THE HOST", "FLATE_HIP_INDEX_PASS_BYTES"):
        assert text in hdr, text
    for mod in (flate, gzip, fzlib):
        assert callable(mod.build_index) and callable(mod.index_from_bytes)
    for name in ("build_index", "index_from_bytes"):
        assert hasattr(Engine, name), name
