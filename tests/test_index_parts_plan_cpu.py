"""flate_amd/csrc/index_parts_plan.h, the host decisions of the fresh seek index, through
tests/cpu_shim/index_parts_plan_shim.cpp: the points of a joined stream against a restatement of the rule, the cut of a range
into parts, the part table's passes, and the version-2 blob."""
import random
import struct

import pytest

import _index_parts_plan as pp
import _index_plan as ip

M64 = (1 << 64) - 1
SLACK, ALIGN = 258, 16


def slot_bytes(need):
    return (need + SLACK + ALIGN - 1) // ALIGN * ALIGN


def rule_pieces(n, piece, spacing):
    """piece 0; piece k >= 1 iff a grid line g * S lies in ((k - 1) * piece, k * piece]; spacing 0 is 1 MiB"""
    s = spacing or (1 << 20)
    pieces = 1 if n == 0 else -(-n // piece)
    return [k for k in range(pieces) if k == 0 or (k * piece) // s > ((k - 1) * piece) // s]


def test_constants():
    assert [pp.const(n) for n in pp.CONSTS] == [2, (1 << 31) - 1]


@pytest.mark.parametrize("piece", [7, 1001, 65535])
def test_points_of_a_joined_stream(piece):
    for n in (0, 1, piece - 1, piece, piece + 1, 3 * piece + 5):
        for spacing in (0, 1, piece, 2 * piece + 1, 1 << 20):
            got = pp.point_pieces(n, piece, spacing)
            assert got == rule_pieces(n, piece, spacing), (n, piece, spacing)
            assert got[0] == 0 and len(got) <= 1 + n // (spacing or (1 << 20))
            if spacing == 1:
                assert got == list(range(max(1, -(-n // piece))))
            place = [10 + 3 * k for k in got]
            assert pp.points(got, place, piece) == [(8 * p, k * piece, 0) for k, p in zip(got, place)]


def test_points_of_a_stream_with_more_pieces_than_one_stretch():
    """the rule is fed 4096 piece starts at a time: the seams between the stretches must not show"""
    for piece, spacing in ((1, 1), (1, 3), (3, 7), (5, 4096), (2, 4095)):
        for n in (4095 * piece, 4096 * piece, 4097 * piece + 1, 3 * 4096 * piece + 2):
            assert pp.point_pieces(n, piece, spacing) == rule_pieces(n, piece, spacing), (n, piece, spacing)


def a_stream(size, piece, spacing, in_len=None):
    """(in_len, size, status, [(in_bit, out_pos)]) of a stream whose piece k lies 7 * k + 2 bytes in"""
    which = rule_pieces(size, piece, spacing)
    pts = [(8 * (7 * k + 2), k * piece) for k in which]
    return (in_len if in_len is not None else 7 * (max(which) + 1) + 20, size, 0, pts)


def expect_cut(stream, begin, length, cap):
    """the definition, restated: (L', status, [(point, skip, len, dst, direct)])"""
    in_len, size, status, pts = stream
    if status != 0 or not pts:
        return 0, status or 1, []
    lp = 0 if begin >= size else min(length, size - begin)
    if lp > cap:
        return 0, 100, []
    if lp == 0:
        return 0, 0, []
    pos = [p for _, p in pts]
    sel = lambda b: max(k for k in range(len(pos)) if pos[k] <= b)  # noqa: E731
    parts = []
    for k in range(sel(begin), sel(begin + lp - 1) + 1):
        nxt = pos[k + 1] if k + 1 < len(pos) else size
        a, b = max(begin, pos[k]), min(begin + lp, nxt)
        parts.append((k, a - pos[k], b - a, a - begin, int(a == pos[k] and b == nxt)))
    return lp, 0, parts


def check_call(streams, ranges, caps, budget=1 << 40):
    c = pp.plan_call(streams, ranges, caps, budget)
    assert c is not None and len(c["ranges"]) == len(ranges)
    point0 = [sum(len(s[3]) for s in streams[:i]) for i in range(len(streams))]
    at = 0
    for j, ((si, begin, length), cap) in enumerate(zip(ranges, caps)):
        lp, status, want = expect_cut(streams[si], begin, length, cap)
        r = c["ranges"][j]
        assert (r["len"], r["status"], r["n_parts"]) == (lp, status, len(want)), (j, r)
        assert r["part0"] == at or not want
        got = c["parts"][at:at + len(want)]
        assert [(p["point"] - point0[si], p["skip"], p["len"], p["dst"], p["direct"]) for p in got] == want, (j, got, want)
        # the parts tile [begin, begin + L') exactly, in order; at most the first and the last go through scratch
        assert [p["dst"] for p in got] == [sum(q["len"] for q in got[:k]) for k in range(len(got))]
        assert sum(p["len"] for p in got) == lp and all(p["len"] > 0 and p["range"] == j for p in got)
        assert all(p["direct"] for p in got[1:-1]) and sum(1 - p["direct"] for p in got) <= 2
        in_len, pts = streams[si][0], streams[si][3]
        for p in got:
            k = p["point"] - point0[si]
            assert p["in_lo"] == pts[k][0] >> 3 and p["in_lo"] < p["in_hi"] <= in_len
            if k + 1 < len(pts):
                assert p["in_hi"] >= min(in_len, (pts[k + 1][0] >> 3) + 1)  # up to the next point at least
            else:
                assert p["in_hi"] == in_len
        at += len(want)
    assert at == len(c["parts"])
    assert c["n_direct"] == sum(p["direct"] for p in c["parts"]) and c["n_scratch"] == len(c["parts"]) - c["n_direct"]
    return c


@pytest.mark.parametrize("piece,spacing", [(7, 1), (7, 15), (1001, 1), (1001, 2003), (65535, 1), (65535, 0)])
def test_the_cut_of_a_range(piece, spacing):
    size = 5 * piece + 3
    st = a_stream(size, piece, spacing)
    pos = [p for _, p in st[3]]
    ranges = [(0, 0, size), (0, 0, M64), (0, 0, 0), (0, size, 5), (0, size + 1, 5), (0, size - 1, 5), (0, M64, M64), (0, 3, M64 - 1)]
    for p in pos + [size]:
        for b in (p - 1, p, p + 1):
            if b < 0:
                continue
            ranges += [(0, b, 1), (0, b, piece), (0, b, 2 * piece + 1), (0, b, M64 - b), (0, b, M64)]  # (the last: begin + len past 2^64)
            for e in (p - 1, p, p + 1):  # ends on a point and one byte either side of it
                for b2 in (0, 1, pos[len(pos) // 2]):
                    if e > b2:
                        ranges.append((0, b2, e - b2))
    caps = [min(r[2], size + 8) for r in ranges]
    c = check_call([st], ranges, caps)
    assert c["n_direct"] and c["n_scratch"]
    # the whole stream: every part is direct
    whole = check_call([st], [(0, 0, size)], [size])
    assert whole["n_scratch"] == 0 and whole["n_direct"] == len(pos) and whole["scratch"] == 0 and whole["pass_first"] == [0, len(pos)]
    # a slot one byte too small: 100, no parts
    small = check_call([st], [(0, 0, size), (0, 1, 10)], [size - 1, 9])
    assert [r["status"] for r in small["ranges"]] == [100, 100] and not small["parts"]


def test_the_cut_over_several_streams_failed_and_empty_ones_among_them():
    rng = random.Random(5)
    streams = [a_stream(40, 7, 1), (50, 0, 102, []), a_stream(0, 7, 1), a_stream(1, 7, 1), a_stream(3000, 1001, 2003), (9, 0, 100, [])]
    ranges = [(rng.randrange(len(streams)), rng.choice((0, 1, 6, 7, 8, 14, 1000, 1001, 1002, 2999, 3000)),
               rng.choice((0, 1, 6, 7, 8, 1001, 2002, 5000, M64))) for _ in range(300)]
    caps = [rng.choice((0, 1, 7, 4096)) for _ in ranges]
    c = check_call(streams, ranges, caps)
    assert [r["status"] for r, q in zip(c["ranges"], ranges) if q[0] == 1] == [102] * sum(q[0] == 1 for q in ranges)
    assert any(r["status"] == 100 for r in c["ranges"]) and c["n_direct"] and c["n_scratch"]


def test_passes_over_the_parts():
    piece = 1001
    st = a_stream(10 * piece, piece, 1)
    # direct parts only: one pass, no scratch, whatever the budget
    c = check_call([st], [(0, 0, 10 * piece), (0, piece, 3 * piece)], [10 * piece, 3 * piece], budget=1)
    assert c["pass_first"] == [0, 13] and c["scratch"] == 0 and c["n_scratch"] == 0
    # a budget smaller than one scratch part: every scratch part opens a pass of its own, direct parts ride along
    ranges = [(0, 5, 3 * piece), (0, 2 * piece + 1, 10), (0, piece, piece), (0, 7, piece)]
    c = check_call([st], ranges, [r[2] for r in ranges], budget=100)
    slots = [0 if p["direct"] else slot_bytes(p["skip"] + p["len"]) for p in c["parts"]]
    assert ip.passes(slots, 100) == (c["pass_first"], [p["slot_off"] for p in c["parts"]], c["scratch"])
    assert len(c["pass_first"]) - 1 == c["n_scratch"] == 5 and c["scratch"] == max(slots)
    assert all(p["slot_off"] == 0 for p in c["parts"] if not p["direct"])
    # a roomy budget: one pass, the scratch parts side by side
    c = check_call([st], ranges, [r[2] for r in ranges], budget=1 << 30)
    assert c["pass_first"] == [0, len(c["parts"])] and c["scratch"] == sum(slots)
    offs = [p["slot_off"] for p in c["parts"] if not p["direct"]]
    assert offs == sorted(offs) and all(o % ALIGN == 0 for o in offs)
    # no range decodes anything: no parts, no pass
    c = check_call([st], [(0, 10 * piece, 4), (0, 0, 0)], [4, 0])
    assert c["parts"] == [] and c["scratch"] == 0


def test_too_many_parts_for_one_call():
    """2^31 parts are one too many for a call (they are counted before any of them is made)"""
    n = 1 << 20
    st = (8 * n + 8, n, 0, [(8 * k, k) for k in range(n)])  # every byte a point
    assert pp.plan_call([st], [(0, 0, n)] * 2048, [n] * 2048, 1 << 30, room_parts=0) is None
    streams = [a_stream(40, 7, 1)]
    assert pp.plan_call(streams, [(0, 0, 40)], [40], 1 << 30) is not None


STREAMS = [(900, 4000, 0, [(80, 0), (800, 1001), (1600, 2002), (4000, 3003)]), (7, 0, 102, []), (30, 0, 0, [(80, 0)]),
           (100, 1, 0, [(0, 0)])]


def test_version_2_blob_round_trip():
    assert pp.parse(pp.blob(1, 1 << 20, STREAMS)) is None  # (four points in 4000 bytes are more than that spacing allows)
    for container, spacing in ((0, 1), (1, 1000), (2, 1001)):
        b = pp.blob(container, spacing, STREAMS)
        assert len(b) == 48 + 32 * len(STREAMS) + 24 * sum(len(s[3]) for s in STREAMS)
        assert struct.unpack_from("<II", b) == (0x58444946, 2) and pp.version(b) == 2
        got = pp.parse(b)
        assert got == dict(container=container, spacing=spacing, win_bytes=0,
                           streams=[(s[0], s[1], s[2], [(bit, pos, 0) for bit, pos in s[3]]) for s in STREAMS])
    assert pp.parse(pp.blob(0, 1, [])) == dict(container=0, spacing=1, win_bytes=0, streams=[])


def test_each_parser_refuses_the_other_version():
    v2 = pp.blob(1, 1001, STREAMS)
    assert ip.parse(v2) is None and pp.parse(v2) is not None
    only_point0 = [(s[0], s[1], s[2], s[3][:1]) for s in STREAMS]  # (no windows: the two layouts differ in the version alone)
    v1 = ip.blob(1, 1001, only_point0)
    assert pp.version(v1) == 1 and ip.parse(v1) is not None and pp.parse(v1) is None
    assert len(v1) == len(pp.blob(1, 1001, only_point0))
    relabelled = v1[:4] + struct.pack("<I", 2) + v1[8:]
    assert pp.parse(relabelled) is not None and ip.parse(relabelled) is None
    v1w = ip.blob(1, 1001, STREAMS)  # with windows
    assert ip.parse(v1w) is not None and pp.parse(v1w) is None and pp.parse(v1w[:4] + struct.pack("<I", 2) + v1w[8:]) is None
    assert pp.version(b"") == 0 and pp.version(b"FIDX") == 0 and pp.version(b"XXXX\2\0\0\0") == 0


def test_version_2_refuses_any_window():
    b = pp.blob(0, 1001, STREAMS)
    pts_at = 48 + 32 * len(STREAMS)
    npts = sum(len(s[3]) for s in STREAMS)
    for k in range(npts):
        for v in (1, 1001, 32768, 1 << 31):
            at = pts_at + 24 * k + 16
            assert pp.parse(b[:at] + struct.pack("<I", v) + b[at + 4:]) is None, (k, v)
        at = pts_at + 24 * k + 20  # the padding word
        assert pp.parse(b[:at] + struct.pack("<I", 1) + b[at + 4:]) is None
    for v in (1, 24, 32768, M64):
        assert pp.parse(b[:32] + struct.pack("<Q", v) + b[40:]) is None
    # ... with the bytes to go with it
    grown = b[:32] + struct.pack("<Q", 8) + struct.pack("<Q", len(b) + 8) + b[48:] + bytes(8)
    assert pp.parse(grown) is None


def test_version_2_keeps_the_invariants_of_version_1():
    good = pp.blob(0, 1001, STREAMS)
    assert pp.parse(good) is not None
    pts_at = 48 + 32 * len(STREAMS)

    def put(at, fmt, v):
        return good[:at] + struct.pack(fmt, v) + good[at + struct.calcsize(fmt):]

    bad = [good[:-1], good + b"\0", good[:47], b"", put(0, "<I", 0x58444947), put(8, "<I", 3), put(16, "<Q", 0),
           put(12, "<I", 5), put(24, "<Q", 7), put(40, "<Q", len(good) - 1),
           put(48 + 16, "<i", 1),                   # a failed stream with points and a size
           put(48 + 32 + 24, "<Q", 1),              # a failed stream with a point
           put(48 + 32 + 8, "<Q", 5),               # ... with a size
           put(48 + 20, "<I", 1),                   # the padding of a stream record
           put(48 + 24, "<Q", 0),                   # a good stream without point 0
           put(48 + 8, "<Q", 3002),                 # more points than 1 + size / spacing; an out_pos beyond the size
           put(48, "<Q", 0xfffffff1),               # a stream longer than a decompress call takes
           put(48, "<Q", 500),                      # an in_bit outside the stream
           put(pts_at + 8, "<Q", 1),                # point 0 not at output byte 0
           put(pts_at + 24 + 8, "<Q", 0),           # out_pos does not ascend
           put(pts_at + 48 + 8, "<Q", 1001),        # ... strictly
           put(pts_at + 48, "<Q", 800),             # in_bit does not ascend strictly
           put(pts_at + 72, "<Q", 900 * 8)]         # in_bit at the stream's end
    for k, b in enumerate(bad):
        assert pp.parse(b) is None, k
