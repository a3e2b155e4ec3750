"""flate_amd/csrc/index_plan.h, the host decisions of the seek index, through tests/cpu_shim/index_plan_shim.cpp: the point
rule against a brute-force restatement, point selection and clipping, the passes under the scratch budget, the blob."""
import random

import _index_plan as ip

M64 = (1 << 64) - 1


def test_constants():
    assert [ip.const(n) for n in ip.CONSTS] == [32768, 1 << 20, 258, 16, 256 << 20, 48, 32, 24, 1, 16]
    L = ip.lib()
    assert L.shim_idx_spacing(0) == 1 << 20 and L.shim_idx_spacing(1) == 1 and L.shim_idx_spacing(M64) == M64
    assert [L.shim_idx_window_len(p) for p in (0, 1, 32767, 32768, 32769, 1 << 40)] == [0, 1, 32767, 32768, 32768, 32768]
    assert [L.shim_idx_max_points(n, s) for n, s in ((0, 1), (0, 5), (4, 5), (5, 5), (1 << 30, 1 << 20))] == [1, 1, 1, 2, 1025]
    assert all(L.shim_idx_args_ok(c, m) for c in (0, 1, 2) for m in (0, 1))
    assert not any(L.shim_idx_args_ok(c, m) for c, m in ((-1, 0), (3, 0), (0, 2), (0, -1)))


def brute_points(pos, spacing):
    """block k >= 1 is a point iff some multiple of the spacing lies in (pos[k - 1], pos[k]]; grid line by grid line"""
    out = [0]
    for k in range(1, len(pos)):
        g = (pos[k - 1] // spacing + 1) * spacing  # the first grid line behind pos[k - 1]
        if g <= pos[k]:
            out.append(k)
    return out


def test_point_rule_against_brute_force():
    rng = random.Random(1)
    for trial in range(400):
        spacing = rng.choice((1, 2, 7, 100, 4096, 1 << 20))
        pos, at = [0], 0
        for _ in range(rng.randint(0, 60)):
            r = rng.random()
            # runs of empty blocks, blocks of a few bytes, blocks that span many grid lines, blocks that end on a grid line
            step = 0 if r < .3 else rng.randint(1, 3) if r < .5 else rng.randint(1, 2 * spacing) if r < .8 else rng.randint(1, 40) * spacing
            if r > .95:
                step = spacing - at % spacing
            at += step
            pos.append(at)
        got = ip.point_rule(pos, spacing)
        assert got == brute_points(pos, spacing), (pos, spacing)
        pts = [pos[k] for k in got]
        assert all(a < b for a, b in zip(pts, pts[1:])) and len(pts) <= 1 + at // spacing
    assert ip.point_rule([0], 3) == [0] and ip.point_rule([0, 0, 0], 1) == [0]
    assert ip.point_rule([0, 1 << 63, M64], 1 << 62) == [0, 1, 2]


def test_select_and_clip():
    rng = random.Random(2)
    for trial in range(300):
        pts = sorted(set([0] + [rng.randrange(1 << rng.choice((4, 20, 60))) for _ in range(rng.randint(0, 40))]))
        for begin in [0, 1, M64] + [p + d for p in pts for d in (-1, 0, 1) if 0 <= p + d <= M64]:
            k = ip.select(pts, begin)
            assert pts[k] <= begin and (k + 1 == len(pts) or pts[k + 1] > begin)
    for begin, n, size, want in ((0, 0, 0, 0), (0, 5, 3, 3), (3, 5, 3, 0), (4, 5, 3, 0), (2, 1, 3, 1), (2, M64, 3, 1), (M64, M64, M64, 0),
                                 (M64 - 1, M64, M64, 1), (1 << 63, (1 << 63) - 1, M64, (1 << 63) - 1), (1 << 63, (1 << 63) + 5, M64, (1 << 63) - 1)):
        assert ip.clip(begin, n, size) == want, (begin, n, size)


def test_plan_range():
    pts = [0, 1000, 5000]
    r = ip.plan_range(6000, 0, pts, 1500, 100, 100)
    assert r == dict(point=1, skip=500, len=100, status=0, decode=1)
    assert ip.plan_range(6000, 0, pts, 5000, M64, 1000) == dict(point=2, skip=0, len=1000, status=0, decode=1)
    assert ip.plan_range(6000, 0, pts, 999, 2, 2)["point"] == 0
    assert ip.plan_range(6000, 0, pts, 1500, 100, 99) == dict(point=0, skip=0, len=0, status=100, decode=0)  # slot too small
    assert ip.plan_range(6000, 0, pts, 6000, 100, 0) == dict(point=0, skip=0, len=0, status=0, decode=0)     # nothing to deliver
    assert ip.plan_range(6000, 0, pts, M64, M64, 0)["decode"] == 0
    assert ip.plan_range(6000, 0, pts, 10, 0, 0)["decode"] == 0
    assert ip.plan_range(0, 4, [], 10, 10, 10) == dict(point=0, skip=0, len=0, status=4, decode=0)            # a failed stream
    for stream in (0, 2):
        assert ip.plan_range(6000, 0, pts, 1500, 100, 100, stream=stream)["point"] == 1


def test_input_bytes_a_range_can_consume():
    """from the byte of the range's point to a few bytes behind the first point at or behind the range's end (the decode stops
    there at the latest), the stream's end where there is no such point"""
    pts, bits, n = [0, 1000, 5000, 9000], [80, 8007, 40001, 70000], 10000
    spare = ip.const("in_spare")

    def span(begin, length):
        r = ip.plan_range(12000, 0, pts, begin, length, 1 << 40, in_bit=bits, in_len=n)
        return r["in_lo"], r["in_hi"]

    assert span(0, 1) == (10, 8007 // 8 + 1 + spare)
    assert span(0, 1000) == (10, 8007 // 8 + 1 + spare)          # ends where point 1 begins
    assert span(0, 1001) == (10, 40001 // 8 + 1 + spare)         # one byte into point 1's block
    assert span(999, 2) == (10, 40001 // 8 + 1 + spare)
    assert span(1000, 4000) == (8007 // 8, 40001 // 8 + 1 + spare)
    assert span(1500, 7500) == (1000, 70000 // 8 + 1 + spare)
    assert span(1500, 7501) == (1000, n) and span(9000, 1) == (8750, n) and span(0, 1 << 63) == (10, n)
    assert ip.plan_range(12000, 0, pts, 5, 5, 1 << 40, in_bit=bits, in_len=1010)["in_hi"] == 1010   # never beyond the stream
    rng = random.Random(9)
    for trial in range(300):
        begin = rng.randrange(12000)
        length = rng.randint(1, 12000 - begin)
        lo, hi = span(begin, length)
        k = max(i for i in range(4) if pts[i] <= begin)
        assert lo == bits[k] // 8 and lo < hi <= n
        behind = [i for i in range(4) if pts[i] >= begin + length]
        assert hi == (min(n, bits[behind[0]] // 8 + 1 + spare) if behind else n)


def test_merge_intervals():
    assert ip.merge([], 10) == [] and ip.merge([(5, 5), (7, 3)], 10) == []
    assert ip.merge([(50, 60), (0, 10), (10, 20), (31, 40)], 9) == [(0, 20), (31, 40), (50, 60)]
    assert ip.merge([(50, 60), (0, 10), (10, 20), (30, 40)], 10) == [(0, 60)]
    assert ip.merge([(0, 100), (10, 20), (99, 101)], 0) == [(0, 101)]
    assert ip.merge([(M64 - 5, M64), (0, 1)], M64) == [(0, M64)] and ip.merge([(M64 - 5, M64), (M64 - 9, M64 - 7)], 1) == [(M64 - 9, M64 - 7), (M64 - 5, M64)]
    rng = random.Random(4)
    for trial in range(200):
        ivs = [(a, a + rng.randint(0, 50)) for a in (rng.randrange(2000) for _ in range(rng.randint(0, 30)))]
        gap = rng.choice((0, 1, 20, 500))
        got = ip.merge(ivs, gap)
        assert all(a < b for a, b in got) and all(p[1] + gap < q[0] for p, q in zip(got, got[1:]))
        covered = set(x for a, b in got for x in range(a, b))
        assert set(x for a, b in ivs for x in range(a, b)) <= covered
        assert len(covered) <= sum(b - a for a, b in ivs) + gap * len(ivs)  # nothing but the bridged gaps is added


def test_slot_bytes():
    for need in (0, 1, 13, 14, 15, 16, 4096, (1 << 40) + 3):
        b = ip.slot_bytes(need)
        assert b % 16 == 0 and need + 258 <= b < need + 258 + 16


def test_passes():
    rng = random.Random(3)
    for trial in range(300):
        budget = rng.choice((1, 4096, 1 << 20))
        slots = [0 if rng.random() < .2 else ip.slot_bytes(rng.randrange(1, rng.choice((100, 3 * budget + 10)))) for _ in range(rng.randint(0, 80))]
        first, off, most = ip.passes(slots, budget)
        if not slots:
            assert first == [0] and most == 0
            continue
        # every range is in exactly one pass, in order
        assert first[0] == 0 and first[-1] == len(slots) and all(a < b for a, b in zip(first, first[1:]))
        worst = 0
        for a, b in zip(first, first[1:]):
            used = 0
            for j in range(a, b):
                assert off[j] == used and used % 16 == 0
                used += slots[j]
            worst = max(worst, used)
            # within the budget, unless a single range alone exceeds it -- then it is the pass's only range that needs scratch
            if used > budget:
                assert sum(1 for j in range(a, b) if slots[j]) == 1
            # ... and no pass could have taken the next range too
            if b < len(slots):
                assert used + slots[b] > budget
        assert most == worst
    assert ip.passes([32, 32, 32], 64)[0] == [0, 2, 3]
    assert ip.passes([M64 - 15, 16], 100)[0] == [0, 1, 2]


STREAMS = [(1000, 70000, 0, [(80, 0), (900, 1000), (4000, 32768), (7999, 70000)]),
           (5, 0, 4, []),
           (20, 0, 0, [(0, 0)]),
           (0xfffffff0, 1 << 40, 0, [(3, 0), (8 * 0xfffffff0 - 1, 1 << 39)])]


def test_blob_round_trip():
    b = ip.blob(2, 1000, STREAMS)
    wins = [0, 1000, 32768, 32768, 0, 0, 32768]
    assert len(b) == 48 + 32 * 4 + 24 * 7 + sum(wins)
    t = ip.parse(b)
    assert t["container"] == 2 and t["spacing"] == 1000 and t["win_bytes"] == sum(wins) and t["win_at"] == len(b) - sum(wins)
    offs = [sum(wins[:k]) for k in range(7)]
    k = 0
    for got, want in zip(t["streams"], STREAMS):
        assert got[:3] == want[:3]
        assert [(a, p) for a, p, _ in got[3]] == want[3]
        assert [w for _, _, w in got[3]] == offs[k:k + len(want[3])]
        k += len(want[3])
    assert ip.parse(ip.blob(0, 1, [])) == dict(container=0, spacing=1, win_bytes=0, win_at=48, streams=[])


def test_blob_refusals():
    good = ip.blob(1, 1000, STREAMS)
    assert ip.parse(good) is not None
    for cut in (0, 1, 47, 48, 100, len(good) - 1):
        assert ip.parse(good[:cut]) is None
    assert ip.parse(good + b"\0") is None

    def put(at, value, size=8):
        return good[:at] + int(value).to_bytes(size, "little") + good[at + size:]

    def bad(streams, container=1, spacing=1000):
        return ip.parse(ip.blob(container, spacing, streams)) is None

    assert ip.parse(put(0, 0x58444947, 4)) is None and ip.parse(put(4, 2, 4)) is None and ip.parse(put(4, 0, 4)) is None
    assert ip.parse(put(8, 3, 4)) is None and ip.parse(put(16, 0)) is None
    assert ip.parse(put(12, 5, 4)) is None and ip.parse(put(12, 0xffffffff, 4)) is None       # n_streams
    assert ip.parse(put(24, 8)) is None and ip.parse(put(24, M64)) is None and ip.parse(put(24, M64 // 24 + 2)) is None  # n_points
    assert ip.parse(put(32, M64)) is None and ip.parse(put(40, len(good) + 1)) is None
    assert ip.parse(put(48 + 20, 1, 4)) is None                                                  # the reserved word of stream 0
    assert ip.parse(put(48 + 4 * 32 + 16, 1, 4)) is None                                         # point 1's window length
    assert bad([(10, 100, 0, [])])                                                               # a good stream without point 0
    assert bad([(10, 0, 4, [(0, 0)])]) and bad([(10, 7, 4, [])])                                 # a failed stream with a point, a size
    assert bad([(10, 100, 0, [(0, 1)])])                                                         # point 0 not at output byte 0
    assert bad([(10, 100, 0, [(80, 0)])]) and not bad([(10, 100, 0, [(79, 0)])])                 # in_bit inside the stream
    assert bad([(10, 5000, 0, [(0, 0), (5, 5001)])]) and not bad([(10, 5000, 0, [(0, 0), (5, 5000)])])   # out_pos within the size
    assert bad([(10, 5000, 0, [(0, 0), (5, 1000), (5, 2000)])])                                  # in_bit ascends strictly
    assert bad([(10, 5000, 0, [(0, 0), (5, 1000), (6, 1000)])])                                  # ... and out_pos
    assert bad([(10, 2999, 0, [(0, 0), (5, 1000), (6, 2000), (7, 2500)])])                       # more points than 1 + size / spacing
    assert bad([(0xfffffff1, 0, 4, [])])                                                         # a stream too long for any call
