"""Streams with ONE planted event ON a sync-flush point F, for the flush handling of the tokenizers (test infrastructure; pure
numpy, no GPU import).  A flush at F runs the reference's tokenizer dry: no match crosses F, the positions F-3 .. F-1 never enter
the hash table, and a flush within 262 bytes before the window fills moves that slide's zone.  In the kernels each of these is an
inequality on F relative to a window start, a tile, a segment or a slide (k_lz_chain<true>, k_lz_parse<true>, the sort / match
tiles of kernels_lz.h, stream_tables.h).  So every case here is tests/_planted.py's background (`junk`, bytes 128..255) with one
event of bytes 0..127 placed against F = B + delta, for the boundaries B of BOUNDS and B = N (F on and 1..4 bytes before the
stream's end).

Event kinds.  `straddle`: a match of L bytes at distance D that starts k bytes before F.  `source`: 20 fresh bytes at F + j
(j = -6 .. +2) copied to F + 3000, and to F + 32768 + j' so that they are seen at distance 32768 and 32769.  `run`: R equal bytes
over F.  `ladder`: _planted.ev_ladder at a = F + d.  `far`: _planted.ev_far at F and F + 1.  `noise`: 140000 uniform bytes with
no event -- there the flush decides which blocks can still be stored (the block log's has_input).

`want` is derived from the construction, by the rules the reference's control flow gives (`_sim_copy`, `_sim_run`), never read
from the oracle; tests/test_planted_flush_cpu.py then finds every `want` in the oracle's token log:
  * a match is cut at every flush point; a piece of fewer than 4 bytes is literals;
  * a candidate at F-3 .. F-1 of any flush point F is not in the table: the copy starts as literals until its source is;
  * position p is visited after slide j (which happens when the window is full at 65536 + 32768 (j - 1)) iff p >= that fill
    minus 262 -- or p >= the last flush point inside those 262 bytes --, and then sees only candidates above 32768 j.
CANDIDATES DROPPED BY A SLIDE: the cases whose event lies in a slide's zone with its source at or below the new window start get
the `want` this last rule predicts (literals up to the window's fill, the rest of the match behind it), not a parity-only mark.
A ladder whose lazy chain lies over F (d < 0) and the `source` cases of the unfinished pattern (the copy lies behind the stream's
end) are parity only: want = ().

Flush patterns.  Every case is `[F]` with finish.  A third (rounded up) of the `straddle` and of the `source` cases at each B -- those with the
smallest CRC-32 of their name -- get a second case with one of `[F, F]`, `[F, F+1, F+2, F+3]`, `[F-4, F]`, `[F, F+4]` and the
unfinished stream (`data[:F]`, `[F]`, no finish), in rotation, so that each B meets every pattern that fits there.

THE CAP.  flush_cases(level) holds at most MAX_FLUSH = 300 cases.  `source` needs delta = -4 .. +4 by ones at nine boundaries (81
cases before any pattern), so nothing is a full matrix: the other kinds sweep delta with `sweep` at 2 .. 4 points (and
delta = 0), and the events' parameters (L, D, k; j and the copy's place; R and the run's start; steps and d; D and a - F) ROTATE
over the (boundary, delta) slots instead of being multiplied out, each value of each parameter met several times over the list.
For the same reason a chosen case gets one further pattern, not all five: five each would take 135 cases for `source` alone.  No
kind, boundary or pattern is dropped (tests/test_planted_flush_cpu.py asserts their presence).  What does not fit is skipped as
_planted._make does: `source`, `run`, `ladder` and `far` at B = N (the event would end behind the stream), `far` and D >= 32768
at B = 14400 (a - D < 0)."""
import functools
import zlib
from typing import NamedTuple

import numpy as np

import _planted as P
from _adversarial import LV

MAX_FLUSH = 300
STREAM_LEN, SMALL_LEN = 140000, 24000
BOUNDS = (14400, 32768, 49152, 65274, 65536, 73728, 81920, 98042, 98304)   # and B = "N"
STRADDLE_L, STRADDLE_D = (5, 33, 258), (1000, 32768, 32769)
SOURCE_LEN, SOURCE_J = 20, tuple(range(-6, 3))
RUN_R = (259, 700)
LADDER_STEPS = (1, 6, 28)
NOISE_F = (32767, 32768, 32769, 65273, 65274, 65275, 65400, 65535, 65536, 65537,
           98041, 98042, 98043, 98168, 98303, 98304)
PATTERNS = ("F", "FF", "F+0123", "F-4,F", "F,F+4", "unfinished")
POINTS = {"straddle": 4, "run": 2, "ladder": 2, "far": 2}
HIST, WIN, MIN_LOOKAHEAD, MIN_MATCH, MAX_MATCH = 32768, 65536, 262, 4, 258


class FlushCase(NamedTuple):
    name: str
    kind: str      # straddle | source | run | ladder | far | noise
    bound: object  # one of BOUNDS | "N"
    F: int
    a: int         # where the event starts (noise: F)
    data: bytes
    flushes: tuple
    finish: bool
    want: tuple    # ((position, ("M", distance, length) | ("L",)), ...); () = parity only
    min_lazy: int


# ---------------------------------------------------------------- what the reference does around flush points, as rules
def zones(n, flushes):
    """first position visited after slide j = 1, 2, ...: 262 bytes before the window is full for the j-th time, or the last
    flush point inside those 262 bytes (the flush ran the tokenizer up to its own position first)"""
    out = []
    full = WIN
    while full <= n:
        z = full - MIN_LOOKAHEAD
        for f in flushes:
            if z < f < full:
                z = f
        out.append(z)
        full += HIST
    return out


def _floor(p, zs):
    """candidates at or below this position are gone when p is visited"""
    return HIST * sum(1 for z in zs if p >= z)


def _in_table(q, flushes):
    return not any(f - 3 <= q <= f - 1 for f in flushes)


def _next_flush(p, flushes, n):
    return min([f for f in flushes if f > p] + [n])


def _sim_copy(a, L, D, n, flushes):
    """tokens over [a, a + L) when those bytes are a copy of [a - D, a - D + L) and of nothing else"""
    zs, out, p, end = zones(n, flushes), [], a, min(a + L, n)
    while p < end:
        room = min(end, _next_flush(p, flushes, n)) - p
        if D <= HIST and p - D > _floor(p, zs) and _in_table(p - D, flushes) and room >= MIN_MATCH:
            out.append((p, ("M", D, room)))
            p += room
        else:
            out.append((p, ("L",)))
            p += 1
    return tuple(out)


def _sim_run(r0, R, n, flushes):
    """tokens over a run of R equal bytes from r0: the nearest position of the run that is in the table"""
    zs, out, p, end = zones(n, flushes), [], r0, min(r0 + R, n)
    while p < end:
        room = min(MAX_MATCH, min(end, _next_flush(p, flushes, n)) - p)
        q = p - 1
        while q >= r0 and not (_in_table(q, flushes) and q > _floor(p, zs)):
            q -= 1
        if q >= r0 and room >= MIN_MATCH:
            out.append((p, ("M", p - q, room)))
            p += room
        else:
            out.append((p, ("L",)))
            p += 1
    return tuple(out)


# ---------------------------------------------------------------- events: plant(rng, buf) -> (a, lowest position written, rule)
def _straddle(F, L, D, k):
    def plant(rng, buf):
        a = F - k
        buf[a:a + L] = P.fresh(rng, L)
        P.copy(rng, buf, a - D, a, L)
        return ("copy", a, L, D)
    return F - k, F - k - D, F - k + L, plant


def _source(F, j, where):
    """where: 0 = copied to F + 3000; 1 / 2 = to where the source is at distance 32768 / 32769"""
    s = F + j
    a = F + 3000 if where == 0 else s + 32767 + where

    def plant(rng, buf):
        buf[s:s + SOURCE_LEN] = P.fresh(rng, SOURCE_LEN)
        P.fence(rng, buf, a - 1, int(buf[s - 1]))
        buf[a:a + SOURCE_LEN] = buf[s:s + SOURCE_LEN]
        P.fence(rng, buf, a + SOURCE_LEN, int(buf[s + SOURCE_LEN]))
        return ("copy", a, SOURCE_LEN, a - s)
    return a, s - 1, a + SOURCE_LEN + 1, plant


def _run(F, R, before):
    r0 = F - before

    def plant(rng, buf):
        P.ev_run(R)[1](rng, buf, r0)
        return ("run", r0, R)
    return r0, r0 - 1, r0 + R + 1, plant


def _ladder(F, steps, d):
    a = F + d
    length, plant0, lowest = P.ev_ladder(steps)

    def plant(rng, buf):
        want = plant0(rng, buf, a)
        return ("fixed", want if d >= 0 else ())
    return a, lowest(a), a + length, plant


def _far(F, D, off):
    a = F + off
    length, plant0, lowest = P.ev_far(D)

    def plant(rng, buf):
        plant0(rng, buf, a)
        return ("far", a, D)
    return a, lowest(a), a + length, plant


def _flushes_of(pattern, F):
    return {"F": (F,), "FF": (F, F), "F+0123": (F, F + 1, F + 2, F + 3), "F-4,F": (F - 4, F), "F,F+4": (F, F + 4),
            "unfinished": (F,)}[pattern]


def _make(kind, label, bound, n, F, event, min_lazy, pattern="F", before=()):
    """one case, or None when the event or the pattern does not fit into [0, n); `before`: earlier flush points"""
    a, lowest, top, plant = event
    fl = tuple(before) + _flushes_of(pattern, F)
    if lowest < 0 or top > n or fl[0] < 0 or fl[-1] > n or F > n:
        return None
    delta = F - (n if bound == "N" else bound)
    name = "flush/%s@%s%+d/%s" % (label, bound, delta, pattern)
    rng = P._rng(name)
    buf = P.junk(rng, n)
    rule = plant(rng, buf)
    finish = pattern != "unfinished"
    if not finish:
        buf = buf[:F]
    m = len(buf)
    if rule[0] == "copy":
        want = _sim_copy(rule[1], rule[2], rule[3], m, fl) if rule[1] < m else ()
    elif rule[0] == "run":
        want = _sim_run(rule[1], rule[2], m, fl)
    elif rule[0] == "far":
        zs = zones(m, fl)
        seen = [rule[2] <= HIST and p - rule[2] > _floor(p, zs) for p in (rule[1], rule[1] + 1)]
        want = ((rule[1], ("M", rule[2], P.FAR_LEN) if seen[0] else ("M", 500, MIN_MATCH)),)
        if seen == [False, True]:
            want = ()  # the source is the last position the slide dropped: whether a + 1 takes over depends on the level's `lazy`
    else:
        want = rule[1]
    return FlushCase(name, kind, bound, F, a, buf.tobytes(), fl, finish, want, min_lazy)


def _len_of(bound):
    return SMALL_LEN if bound == 14400 else STREAM_LEN


def _rotor(combos, stride):
    """the combos in an order in which neighbours differ in every parameter; take(fits, score) gives, of the next 32 that fit, the
    first with the highest score"""
    order = [combos[(i * stride) % len(combos)] for i in range(len(combos))]
    state = [0]

    def take(fits, score=lambda c: 0):
        m = len(order)
        cand = [order[(state[0] + i) % m] for i in range(m)]
        cand = [c for c in cand if fits(c)]
        best = max(cand[:32], key=score)  # (the first of the best)
        state[0] = (order.index(best) + 1) % m
        return best
    return take


def _k_values(L):
    return sorted({0, 1, 3, 4, 5, L - 4, L - 3, L - 1, L})


@functools.lru_cache(None)
def _all_cases():
    out = []
    phases, pairs = set(), set()  # offsets of a 24-byte segment at which a straddle has started so far; its (L, k) and (L, D)

    def add(c):
        if c is not None:
            out.append(c)
        return c

    # ---- straddle
    take = _rotor([(L, D, k) for L in STRADDLE_L for D in STRADDLE_D for k in _k_values(L)], 29)
    for b, bound in enumerate(BOUNDS):
        n = _len_of(bound)
        for delta in P.sweep(4, 29, POINTS["straddle"], b % 5):
            F = bound + delta
            L, D, k = take(lambda c: F - c[2] - c[1] >= 0,
                           lambda c: 2 * ((c[0], "k", c[2]) not in pairs) + 2 * ((c[0], "D", c[1]) not in pairs) + ((F - c[2]) % 24 not in phases))
            phases.add((F - k) % 24)
            pairs.update({(L, "k", k), (L, "D", D)})
            add(_make("straddle", "straddle_L%d_D%d_k%d" % (L, D, k), bound, n, F, _straddle(F, L, D, k), 0))
    for e in range(5):  # B = N: the match ends on the stream's last byte, the flush 0 .. 4 bytes before it
        F = STREAM_LEN - e
        for _ in range(2):
            L, D, k = take(lambda c: c[0] - c[2] == e, lambda c: ((c[0], "k", c[2]) not in pairs) + ((c[0], "D", c[1]) not in pairs))
            pairs.update({(L, "k", k), (L, "D", D)})
            add(_make("straddle", "straddle_L%d_D%d_k%d" % (L, D, k), "N", STREAM_LEN, F, _straddle(F, L, D, k), 0))

    # ---- source: delta -4 .. +4 by ones, always
    take = _rotor([(j, w) for j in SOURCE_J for w in (0, 1, 2)], 10)
    for bound in BOUNDS:
        n = _len_of(bound)
        for delta in range(-4, 5):
            F = bound + delta
            j, w = take(lambda c: _source(F, c[0], c[1])[2] <= n)
            add(_make("source", "source_j%+d_%s" % (j, ("near", "D32768", "D32769")[w]), bound, n, F, _source(F, j, w), 0))

    # ---- run
    take = _rotor([(R, half) for R in RUN_R for half in (True, False)], 1)
    for b, bound in enumerate(BOUNDS):
        n = _len_of(bound)
        for delta in P.sweep(4, 29, POINTS["run"], (b + 2) % 5):
            F = bound + delta
            R, half = take(lambda c: True)
            add(_make("run", "run_%d_%s" % (R, "half" if half else "F-2"), bound, n, F, _run(F, R, R // 2 if half else 2), 0))

    # ---- ladder: a = F + d, d = -(steps + 2) .. +1
    take = _rotor([(s, d) for s in LADDER_STEPS for d in range(-(s + 2), 2)], 17)
    lphases, lused = {s: set() for s in LADDER_STEPS}, set()
    for b, bound in enumerate(BOUNDS):
        n = _len_of(bound)
        slots = []  # at every delta a ladder whose lazy chain lies over F; at the first delta and at delta = 0 one behind F too
        for i, delta in enumerate(P.sweep(4, 29, POINTS["ladder"], (b + 1) % 5)):
            slots += [(delta, True)] + ([(delta, False)] if i == 0 or delta == 0 else [])
        for i, (delta, over) in enumerate(slots):
            F = bound + delta
            s = LADDER_STEPS[(b + i) % 3]
            c = take(lambda c: c[0] == s and over == (c[1] < 0), lambda c: (6 if c[1] in (-(s + 2), -1, 0, 1) else 2) * (c not in lused) + ((F + c[1]) % 24 not in lphases[s]))
            lphases[s].add((F + c[1]) % 24)
            lused.add(c)
            add(_make("ladder", "ladder_%d_d%+d" % c, bound, n, F, _ladder(F, c[0], c[1]), s + 4))

    # ---- far
    take = _rotor([(D, off) for D in P.FAR_D for off in (0, 1)], 1)
    for b, bound in enumerate(BOUNDS):
        n = _len_of(bound)
        for delta in P.sweep(4, 29, POINTS["far"], (b + 3) % 5):
            F = bound + delta
            D, off = take(lambda c: True)
            add(_make("far", "far_D%d_a%+d" % (D, off), bound, n, F, _far(F, D, off), 0))

    # ---- noise: one stream of uniform bytes, the flush point alone differs
    noise = P._rng("flush/noise").integers(0, 256, STREAM_LEN, dtype=np.uint8).tobytes()
    for F in NOISE_F:
        bound = min(BOUNDS, key=lambda B: (abs(F - B), B))
        out.append(FlushCase("flush/noise@%d/F" % F, "noise", bound, F, F, noise, (F,), True, (), 0))

    # ---- the further patterns of a third of the straddle and source cases at each B
    extra = []
    for b, bound in enumerate(BOUNDS + ("N",)):
        turn = b
        for kind in ("straddle", "source"):
            mine = sorted((c for c in out if c.kind == kind and c.bound == bound), key=lambda c: zlib.crc32(c.name.encode()))
            for c in mine[:(len(mine) + 2) // 3]:  # (a third, rounded up)
                for t in range(5):  # the next pattern that fits (B = N: no flush point behind the stream's end)
                    pattern = PATTERNS[1 + (turn + t) % 5]
                    again = _remake(c, pattern)
                    if again is not None:
                        extra.append(again)
                        turn += t + 1
                        break
    return tuple(out + extra)


def _remake(c, pattern):
    label = c.name.split("/")[1].split("@")[0]
    n = _len_of(c.bound) if c.bound != "N" else STREAM_LEN
    p = label.split("_")
    if c.kind == "straddle":
        ev = _straddle(c.F, int(p[1][1:]), int(p[2][1:]), int(p[3][1:]))
    else:
        ev = _source(c.F, int(p[1][1:]), ("near", "D32768", "D32769").index(p[2]))
    return _make(c.kind, label, c.bound, n, c.F, ev, c.min_lazy, pattern)


OBJECT_LEN, OBJECT_BEFORE = 330000, (60000, 150000)
OBJECT_F = (229376, 229376 - 262, 229376 - 1, 229376 + 1, 262144, 245760)


@functools.lru_cache(None)
def object_cases():
    """for the Compressor object, which drops the history a flush can no longer depend on: streams of 330000 bytes with flush
    points at 60000, 150000 and F -- F on and around the window start 229376 (the fill of the sixth slide), its zone's edge, the
    next fill and the seam between them -- and behind F an event that reaches back exactly as far as a window does"""
    out = []
    for F in OBJECT_F:
        events = [("far", "far_D%d_a%+d" % (D, off), _far(F, D, off), 0) for D in P.FAR_D for off in (0, 1)]
        events += [("straddle", "straddle_L258_D32768_k%d" % k, _straddle(F, 258, 32768, k), 0) for k in (0, 100, 257)]
        events += [("ladder", "ladder_6_d+0", _ladder(F, 6, 0), 10)]
        for kind, label, ev, min_lazy in events:
            c = _make(kind, "object/" + label, F, OBJECT_LEN, F, ev, min_lazy, before=OBJECT_BEFORE)
            assert c is not None
            out.append(c)
    return tuple(out)


def flush_cases(level):
    """the list of a level: ladders only where their last step is still evaluated lazily (steps + 4 <= lazy)"""
    lazy = LV[level][1]
    cases = [c for c in _all_cases() if c.min_lazy <= lazy]
    assert len(cases) <= MAX_FLUSH, len(cases)
    return cases


def pattern_of(case):
    return case.name.rsplit("/", 1)[1]
