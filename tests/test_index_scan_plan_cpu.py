"""flate_amd/csrc/index_scan_plan.h: the lists the walkers of flate_hip_index_scan hand over, to the points of a stream --
against a brute-force model that knows every mark and every match of the stream.

A stream is a timeline of marks, matches and plain block starts; it is cut into random walks at block starts (marks among
them), every walk's list is written down as kernels_index_scan.h describes it (device_lists below: the cell comparison
among the walk's own marks, the first mark of an inner walk listed whatever its cell, need measured from the newest listed
mark), and the host decision over those lists must give block 0 and exactly the kept marks behind which no match reaches
in front of them."""
import random

import pytest

import _index_scan_plan as P


def point_rule(pos, spacing):
    return [k for k in range(len(pos)) if k == 0 or pos[k] // spacing > pos[k - 1] // spacing]


def timeline(rng, n_events, spacing_hint):
    """[(kind, bit, pos, distance)]: kind 'mark' | 'match' | 'start' (a block start that is no mark), in stream order; the
    stream's size.  Matches reach exactly to a mark, one byte in front of it, or anywhere."""
    ev, bit, pos, marks = [], 80, 0, []
    for _ in range(n_events):
        bit += rng.choice((8, 16, 24, 1000))
        kind = rng.choice(("mark", "mark", "match", "match", "match", "start", "lit"))
        if kind == "lit":
            pos += rng.choice((1, 2, 50, spacing_hint, 3 * spacing_hint))
        elif kind == "match":
            if pos == 0:
                pos += 1
            far = min(pos, 32768)
            near = [pos - m for m in marks[-6:] if 0 < pos - m <= far] + [pos - m + 1 for m in marks[-6:] if 0 < pos - m + 1 <= far]
            d = rng.choice(near) if near and rng.random() < .7 else rng.randint(1, far)
            ev.append(("match", bit, pos, d))
            pos += rng.choice((3, 4, 258))
        else:
            ev.append((kind, bit, pos, 0))
            if kind == "mark":
                marks.append(pos)
                if rng.random() < .15:  # two markers in a row
                    bit += 40
                    ev.append(("mark", bit, pos, 0))
                    marks.append(pos)
    return ev, pos


def brute_points(ev, spacing):
    marks = [(b, p) for k, b, p, _ in ev if k == "mark"]
    kept = point_rule([0] + [p for _, p in marks], spacing)
    matches = [(p, d) for k, _, p, d in ev if k == "match"]
    out = [(80, 0)]
    for k in kept[1:]:
        b, c = marks[k - 1]
        if not any(p >= c and p - d < c for p, d in matches):
            out.append((b, c))
    return out


def device_lists(ev, size, spacing, cuts):
    """the walks' lists: cuts are indices into ev of the block starts (marks or plain starts) the walks begin at"""
    walks, bounds = [], [None] + list(cuts) + [None]
    for w in range(len(bounds) - 1):
        a, b = bounds[w], bounds[w + 1]
        first = a is None
        base = 0 if first else ev[a][2]
        lo = 0 if first else a + 1              # (the cut's own event is the walk in front's: it ends there)
        hi = len(ev) if b is None else b + 1
        entries = [[80 if first else ev[a][1], base, 0]]
        origin, prev, last_mark, has_mark = base, (0 if first else None), 0, False
        for kind, bit, pos, d in ev[lo:hi]:
            if kind == "match":
                if pos - d < origin:
                    entries[-1][2] = max(entries[-1][2], d - (pos - origin))
            elif kind == "mark":
                is_kept = prev is None or pos // spacing > prev // spacing
                prev, last_mark, has_mark = pos, pos, True
                if is_kept:
                    entries.append([bit, pos, 0])
                    origin = pos
        end = size if b is None else ev[b][2]
        walks.append(dict(entries=[tuple(e) for e in entries], out_len=end - base, last_mark=last_mark, has_mark=has_mark, first=first))
    return walks


def random_cuts(rng, ev, n):
    cand = [i for i, e in enumerate(ev) if e[0] in ("mark", "start")]
    return sorted(rng.sample(cand, min(n, len(cand))))


@pytest.mark.parametrize("seed", range(40))
def test_points_equal_the_brute_force_model(seed):
    rng = random.Random(seed)
    spacing = rng.choice((1, 1, 7, 100, 4096))
    seen = dict(fresh=0, stale=0, cross_kept=0, cross_dropped=0, cut_at_mark=0, edge=0)
    for _ in range(60):
        ev, size = timeline(rng, rng.choice((0, 3, 20, 80)), spacing)
        want = brute_points(ev, spacing)
        whole = P.points(device_lists(ev, size, spacing, []), size, spacing)
        assert whole == want
        for n_cuts in (1, 3, 9):
            cuts = random_cuts(rng, ev, n_cuts)
            walks = device_lists(ev, size, spacing, cuts)
            assert P.points(walks, size, spacing) == want, (spacing, ev, cuts)
            seen["cut_at_mark"] += sum(ev[c][0] == "mark" for c in cuts)
            prev = 0
            for w in walks:
                if not w["first"] and len(w["entries"]) > 1:
                    kept = w["entries"][1][1] // spacing > prev // spacing
                    seen["cross_kept" if kept else "cross_dropped"] += 1
                if w["has_mark"]:
                    prev = w["last_mark"]
                assert len(w["entries"]) <= P.max_entries(w["out_len"], spacing)
        n_marks = len(point_rule([0] + [p for k, _, p, _ in ev if k == "mark"], spacing)) - 1
        seen["fresh"] += len(want) - 1
        seen["stale"] += n_marks - (len(want) - 1)
        marks = set(p for k, _, p, _ in ev if k == "mark")
        seen["edge"] += sum(1 for k, _, p, d in ev if k == "match" and (p - d in marks or p - d + 1 in marks))
    assert seen["fresh"] and seen["stale"] and seen["cut_at_mark"] and seen["edge"], seen
    assert seen["cross_kept"] and (spacing == 1 or seen["cross_dropped"]), seen


def _good():
    """two walks of a stream of 1000 bytes: marks at 100 (fresh), 300 (a match at 350 reaches 299) and, in the second walk,
    600 and 900"""
    return [dict(entries=[(80, 0, 0), (800, 100, 0), (2400, 300, 1)], out_len=500, last_mark=300, has_mark=True, first=True),
            dict(entries=[(4000, 500, 0), (4800, 600, 0), (7200, 900, 0)], out_len=500, last_mark=900, has_mark=True, first=False)]


def test_the_directed_lists():
    assert P.points(_good(), 1000, 1) == [(80, 0), (800, 100), (4800, 600), (7200, 900)]
    # a match of the second walk reaches in front of 300 and of 100: need lies exactly at the boundary
    w = _good()
    w[1]["entries"][0] = (4000, 500, 400)
    assert P.points(w, 1000, 1) == [(80, 0), (800, 100), (4800, 600), (7200, 900)]
    w[1]["entries"][0] = (4000, 500, 401)
    assert P.points(w, 1000, 1) == [(80, 0), (4800, 600), (7200, 900)]
    # the second walk's first mark is dropped by the rule against the first walk's last mark, and only constrains
    w = _good()
    w[0]["entries"] = [(80, 0, 0)]  # (spacing 400: the first walk's marks, the last at 399, lie in block 0's cell)
    w[0]["last_mark"] = 399
    w[1]["entries"] = [(4000, 500, 0), (4800, 600, 0), (7200, 900, 0)]
    assert P.points(w, 1000, 400) == [(80, 0), (4800, 600), (7200, 900)]
    w[0]["last_mark"] = 400  # 600 lies in the cell of the last mark in front of it
    assert P.points(w, 1000, 400) == [(80, 0), (7200, 900)]
    w[1]["entries"][1] = (4800, 600, 1)  # ... and still constrains: a match behind it reaches in front of it, not of 900
    assert P.points(w, 1000, 400) == [(80, 0), (7200, 900)]
    w[1]["entries"][2] = (7200, 900, 301)  # a match behind 900 reaches in front of it
    assert P.points(w, 1000, 400) == [(80, 0)]
    # an empty stream, and a stream without marks
    assert P.points([dict(entries=[(0, 0, 0)], out_len=0, last_mark=0, has_mark=False, first=True)], 0, 1) == [(0, 0)]
    assert P.points([dict(entries=[(16, 0, 0)], out_len=77, last_mark=0, has_mark=False, first=True)], 77, 1) == [(16, 0)]
    # a mark at out_pos == size
    assert P.points([dict(entries=[(16, 0, 0), (800, 77, 0)], out_len=77, last_mark=77, has_mark=True, first=True)], 77, 1) == [(16, 0), (800, 77)]


def test_lists_that_disagree_with_the_probe_are_refused():
    assert P.points(_good(), 1000, 1) is not None
    w = _good()
    w[0]["entries"][0] = (80, 0, 1)  # a first entry with need > 0
    assert P.points(w, 1000, 1) is None
    assert P.points(_good(), 1001, 1) is None and P.points(_good(), 999, 1) is None  # the lengths do not add up to size
    w = _good()
    w[1]["out_len"] = 499
    assert P.points(w, 1000, 1) is None
    w = _good()
    w[1]["entries"][0] = (4000, 501, 0)  # a walk that does not start where the one before ended
    assert P.points(w, 1000, 1) is None
    assert P.points([], 0, 1) is None
    w = _good()
    w[0]["entries"] = []
    assert P.points(w, 1000, 1) is None
    w = _good()
    w[0]["first"] = False
    assert P.points(w, 1000, 1) is None
    w = _good()
    w[1]["first"] = True
    assert P.points(w, 1000, 1) is None
    w = _good()
    w[1]["entries"][2] = (7200, 1001, 0)  # a mark outside its walk
    assert P.points(w, 1000, 1) is None
    w = _good()
    w[1]["entries"][2] = (4800, 900, 0)  # bits that do not ascend
    assert P.points(w, 1000, 1) is None
    w = _good()
    w[0]["entries"][2] = (2400, 300, 301)  # a match that reaches in front of the stream's first byte
    assert P.points(w, 1000, 1) is None
    w = _good()
    w[0]["last_mark"] = 299  # a last mark in front of a listed one
    assert P.points(w, 1000, 1) is None
    w = _good()
    w[0]["has_mark"] = False
    assert P.points(w, 1000, 1) is None
    assert P.points(_good(), 1000, 250) is None  # 300 cannot have been kept behind 100 at this spacing


def test_room_for_a_walks_list():
    """its start, its first mark and a mark per cell -- but never more marks than markers fit into its bits (35 each)"""
    assert P.max_entries(0, 1) == 3 and P.max_entries(999, 1000) == 3 and P.max_entries(1000, 1000) == 4
    for out_len, spacing, in_bits in ((0, 1, 0), (10, 1, 24), (1 << 30, 1, 8 * 4000), (1 << 30, 1 << 20, 8 * 4000), (5000, 7, 1 << 40),
                                      (1 << 63, 1, (1 << 64) - 1)):
        got = P.walk_entries(1 + out_len // spacing, in_bits)
        assert got == 2 + min(1 + out_len // spacing, 1 + in_bits // 32)
        assert got >= 2 + min(1 + out_len // spacing, 1 + in_bits // 35)  # what a walk can list
        assert got <= P.max_entries(out_len, spacing)
