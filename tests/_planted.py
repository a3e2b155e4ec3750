"""Inputs with ONE planted event at a chosen position, for the tokenizers' own geometry (test infrastructure; pure numpy, no GPU
import).  k_lz_parse parses 1024 segments of 48 bytes from guessed starts and stitches the true path through them, then does the
same for targets [49152, 65536) in segments of 24 bytes from a window moved down by 16320 positions; k_lz_walk does it with
64-byte segments; k_lz_parse<true> with 24-byte segments and a seam at window-relative 49152.  What decides whether their tokens
are right is WHERE something happens: at which offset a path enters a segment, whether a 258-byte match jumps five segments,
whether a lazy chain of improving matches straddles 49152, whether a candidate at distance exactly 32768 is seen from sub-pass
B (and one at 32769 is not), whether an event ends on the chunk's last byte.  So every case here is a background (`junk`: bytes
128..255, or `text`) with one event made of bytes 0..127 -- which junk never holds -- at a = B + delta, for the boundaries
B in {14400, 49152, 51456, N} (14400 and 51456 are multiples of 192: a segment start of the 48-, 24- and 64-byte segments alike;
49152 is the seam of the two sub-passes; B = N puts the event's end on and just before the chunk's last byte).

A case records `want`: (position, token) pairs that tests/test_planted_cpu.py must find in the oracle's token list, so that a
case which stops doing what its name says fails in the CPU tier.  Every case draws from a numpy Generator seeded from its own
name: thinning or adding cases leaves the others as they are.

The delta sweeps.  delta runs from -(event length + 4) to +49 (streams: +29) with a step that is coprime to 48 and to 64, so the
entry phases of a segment are met over the sweep.  The full matrix at step 5 .. 13 is several times the budget of a list
(1600 junk chunks, 400 text chunks, 150 streams per level), so a sweep takes the smallest step of STEPS that leaves it at most
`points` values (`sweep`): 5 or 7 for the short events, larger ones for the events of 258 bytes and more, whose long middle
stretch -- the event's inside lying over the boundary -- is the same situation at every delta.  No event kind, parameter or
boundary is dropped for it.  Every sweep also holds delta = 0, and a ladder's sweep the deltas, by fives, at which its lazy
chain lies over the boundary (`ladder_sweep`).  At B = N a sweep has only the two ends that fit: the event ends 4 bytes before
the chunk's end, and on its last byte."""
import functools
import zlib
from typing import NamedTuple

import numpy as np

from _adversarial import LV

N_FULL = 65535
N_EDGE = (49151, 49152, 49153, 49407, 49408, 49409)   # either side of the seam and of the seam + PZ_LOOK
BOUNDS = (14400, 49152, 51456)                        # and B = N
STEPS = tuple(s for s in range(5, 800) if s % 2 and s % 3)  # coprime to 48 and 64
MATCH_L = (4, 5, 33, 258)
MATCH_D = (1000, 32767, 32768, 32769)
LADDER_STEPS = (1, 3, 6, 12, 28)
FAR_D = (32768, 32769)
FAR_LEN = 40
RUN_R = (3, 4, 258, 259, 260, 700)
PERIODS = (2, 3, 7)
PERIODIC_LEN = 1500
STREAM_LEN = 140000
STREAM_BOUNDS = (73728, 81920)  # the second window's interior and its seam (window-relative 49152)
MAX_JUNK, MAX_TEXT, MAX_STREAMS = 1600, 400, 150
POINTS = {"full": 10, "edge": 3, "text": 3, "stream": 6, "periodic": 5}  # values per delta sweep (and delta = 0), by list


class Case(NamedTuple):
    name: str
    kind: str     # match | ladder | far | run | periodic | tiny
    bound: object  # 14400 | 49152 | 51456 | "N" (streams: 73728 | 81920); None for tiny
    a: int
    data: bytes
    want: tuple   # ((position, ("M", distance, length) | ("L",)), ...): what the oracle's token list must hold
    min_lazy: int  # the case applies to levels whose `lazy` is at least this


def sweep(length, hi, points, shift=0):
    """delta from -(length + 4) to hi, by the smallest step of STEPS that gives at most `points` values; and delta = 0: the event
    starts ON the boundary (the first target of sub-pass B is the one position there that sees a candidate at distance 32768
    right above the re-based null link).  `shift` (0..4) starts the sweep that much earlier: the sweeps of one event at the
    three boundaries, and of events of one length, then meet different offsets of a segment."""
    lo = -(length + 4) - shift
    for st in STEPS:
        r = range(lo, hi + 1, st)
        if len(r) <= points:
            return sorted(set(r) | {0})
    raise ValueError((length, hi, points))


def ladder_sweep(length, hi, points, shift=0):
    """a ladder's sweep, and by fives the deltas at which its lazy chain -- the `steps` literals before the 258-byte match --
    lies over the boundary: the anchor in one segment or sub-pass, its lazy calls in the next"""
    return sorted(set(sweep(length, hi, points, shift)) | set(range(-(length - 258 + 4) - shift, 5, 5)))


def _rng(name):
    return np.random.default_rng([0x504C414E, zlib.crc32(name.encode())])


def junk(rng, n):
    return rng.integers(128, 256, n, dtype=np.uint8)


def fresh(rng, n):
    """event material: bytes 0..127"""
    return rng.integers(0, 128, n, dtype=np.uint8)


@functools.lru_cache(None)
def _text(n):
    from flate_amd import synth
    t = synth.text(synth.SEED_TEXT + 41, n)
    t.setflags(write=False)
    return t


def background(rng, kind, n):
    return junk(rng, n) if kind == "junk" else _text(n).copy()


def fence(rng, buf, i, avoid):
    """make buf[i] differ from `avoid` (a byte 128..255 in its place when it does not)"""
    r = int(rng.integers(0, 128))
    if 0 <= i < len(buf) and avoid is not None and buf[i] == avoid:
        buf[i] = 128 + r if 128 + r != avoid else 128 + (r + 1) % 128


def copy(rng, buf, s, a, L):
    """buf[a : a+L] written to buf[s : s+L]; the byte before and the byte behind the copy are changed when they equal the bytes
    before and behind the original (a chance agreement would start the match one position early or make it one byte longer)"""
    buf[s:s + L] = buf[a:a + L]
    fence(rng, buf, s - 1, int(buf[a - 1]) if a >= 1 else None)
    fence(rng, buf, s + L, int(buf[a + L]) if a + L < len(buf) else None)


# ---------------------------------------------------------------- events: (length, plant(rng, buf, a) -> want, lowest position written for a)
def ev_match(L, D):
    def plant(rng, buf, a):
        buf[a:a + L] = fresh(rng, L)
        copy(rng, buf, a - D, a, L)
        return ((a, ("M", D, L) if D <= 32768 else ("L",)),)
    return L, plant, lambda a: a - D


def ladder_base(a):
    return a - 20000 if a >= 22000 else 1000


def ev_ladder(steps):
    """the construction of test_gpu_stream._edge_stream: copies of [a+k, a+2k+4) (k + 4 bytes that match at a + k), then of
    [a+steps, a+steps+258), from `base` upwards, 8 bytes apart: every position finds a longer match than the one before it"""
    def plant(rng, buf, a):
        n = steps + 258
        buf[a:a + n] = fresh(rng, n)
        pos = ladder_base(a)
        for k in range(steps):
            copy(rng, buf, pos, a + k, k + 4)
            pos += k + 4 + 8
        copy(rng, buf, pos, a + steps, 258)
        assert pos + 258 < a
        return tuple((a + k, ("L",)) for k in range(steps)) + ((a + steps, ("M", a + steps - pos, 258)),)
    return steps + 258, plant, lambda a: min(a, ladder_base(a))


def ev_far(D):
    def plant(rng, buf, a):
        buf[a:a + FAR_LEN] = fresh(rng, FAR_LEN)
        copy(rng, buf, a - D, a, FAR_LEN)
        for d in (1500, 1000, 500):  # nearer candidates that share the first 4 bytes only
            copy(rng, buf, a - d, a, 4)
        return ((a, ("M", D, FAR_LEN) if D <= 32768 else ("M", 500, 4)),)
    return FAR_LEN, plant, lambda a: a - D


def ev_run(R):
    def plant(rng, buf, a):
        v = int(fresh(rng, 1)[0])
        buf[a:a + R] = v
        fence(rng, buf, a - 1, v)
        fence(rng, buf, a + R, v)
        return ((a, ("L",)),) + (((a + 1, ("M", 1, min(258, R - 1))),) if R >= 5 else ())
    return R, plant, lambda a: a


def ev_periodic(p):
    def plant(rng, buf, a):
        unit = fresh(rng, p)
        buf[a:a + PERIODIC_LEN] = np.resize(unit, PERIODIC_LEN)
        return ()
    return PERIODIC_LEN, plant, lambda a: a


def events():
    """(kind, label, (length, plant, lowest), min_lazy)"""
    ev = [("match", "match_L%d_D%d" % (L, D), ev_match(L, D), 0) for L in MATCH_L for D in MATCH_D]
    ev += [("ladder", "ladder_%d" % s, ev_ladder(s), s + 4) for s in LADDER_STEPS]
    ev += [("far", "far_D%d" % D, ev_far(D), 0) for D in FAR_D]
    ev += [("run", "run_%d" % R, ev_run(R), 0) for R in RUN_R]
    return ev


def _make(bg, kind, label, event, min_lazy, bound, n, delta):
    """one case, or None when the event does not fit into [0, n)"""
    length, plant, lowest = event
    a = (n if bound == "N" else bound) + delta
    if lowest(a) < 0 or a + length > n:
        return None
    name = "%s/%s@%s%+d/N%d" % (bg, label, bound, delta, n)
    rng = _rng(name)
    buf = background(rng, bg, n)
    want = plant(rng, buf, a)
    return Case(name, kind, bound, a, buf.tobytes(), want, min_lazy)


def _matrix(bg, sizes, points_full, points_edge):
    out = []
    for e, (kind, label, event, min_lazy) in enumerate(events()):
        length = event[0]
        for n in sizes:
            full = n == N_FULL
            for b, bound in enumerate((BOUNDS if full else (49152,)) + ("N",)):
                shift = (2 * e + b + n) % 5  # (tests/test_planted_cpu.py: with it the starts meet every offset of a segment)
                if bound == "N":
                    deltas = [-(length + 4), -length]
                elif kind == "ladder":
                    deltas = ladder_sweep(length, 49, (points_full if full else points_edge) - 2, shift)
                else:
                    deltas = sweep(length, 49, points_full if full else points_edge, shift)
                for d in deltas:
                    c = _make(bg, kind, label, event, min_lazy, bound, n, d)
                    if c is not None:
                        out.append(c)
    return out


@functools.lru_cache(None)
def _all_chunks(bg):
    if bg == "junk":
        return tuple(_matrix("junk", (N_FULL,) + N_EDGE, POINTS["full"], POINTS["edge"]))
    return tuple(_matrix("text", (N_FULL,), POINTS["text"], 0))


def chunk_cases(level, bg="junk"):
    """the junk list (the whole matrix at N = 65535; B = 49152 and B = N at the six lengths around the seam and the seam + 256) or
    the text list (N = 65535 only) of a level: ladders only where their last step is still evaluated lazily (steps + 4 <= lazy)"""
    lazy = LV[level][1]
    return [c for c in _all_chunks(bg) if c.min_lazy <= lazy]


@functools.lru_cache(None)
def periodic_cases():
    """1500 bytes of period 2, 3, 7 over every boundary: paths from different entries never meet.  Parity only."""
    out = []
    for p in PERIODS:
        ev = ev_periodic(p)
        for bound in BOUNDS + ("N",):
            deltas = [-(PERIODIC_LEN + 4), -PERIODIC_LEN] if bound == "N" else sweep(PERIODIC_LEN, 49, POINTS["periodic"])
            for d in deltas:
                c = _make("junk", "periodic", "periodic_p%d" % p, ev, 0, bound, N_FULL, d)
                if c is not None:
                    out.append(c)
    return tuple(out)


@functools.lru_cache(None)
def tiny_cases():
    """every N from 4 to 200: junk whose last max(4, N // 3) bytes are a copy of its first ones -- the segment count goes through
    1, 2, 3, 4 and the event ends on the last byte.  Parity only."""
    out = []
    for n in range(4, 201):
        name = "junk/tiny/N%d" % n
        rng = _rng(name)
        buf = junk(rng, n)
        L = max(4, n // 3)
        buf[n - L:] = buf[:L].copy()
        out.append(Case(name, "tiny", None, n - L, buf.tobytes(), (), 0))
    return tuple(out)


def stream_events():
    ev = [("match", "match_L%d_D%d" % (L, D), ev_match(L, D), 0) for L in (5, 258) for D in (1000, 32768, 32769)]
    ev += [("ladder", "ladder_%d" % s, ev_ladder(s), s + 4) for s in (1, 6)]
    ev += [("far", "far_D%d" % D, ev_far(D), 0) for D in FAR_D]
    return ev


@functools.lru_cache(None)
def _all_streams():
    out = []
    for kind, label, event, min_lazy in stream_events():
        for bound in STREAM_BOUNDS:
            for d in (ladder_sweep(event[0], 29, POINTS["stream"] - 2) if kind == "ladder" else sweep(event[0], 29, POINTS["stream"])):
                c = _make("junk", kind, label, event, min_lazy, bound, STREAM_LEN, d)
                assert c is not None
                out.append(c._replace(name="stream/" + c.name))
    return tuple(out)


def stream_cases(level):
    """streams of 140000 junk bytes with one event in the second window: around stream position 73728 (its interior) and
    81920 (its window-relative 49152, the seam of k_lz_parse<true>'s sub-passes)"""
    lazy = LV[level][1]
    return [c for c in _all_streams() if c.min_lazy <= lazy]


# ---------------------------------------------------------------- reading a token list
def token_starts(tokens):
    """(start position of every token, its length), without a Python loop"""
    t = np.asarray(tokens, np.uint32).astype(np.int64)
    lens = np.where((t >> 23) & 1, ((t >> 15) & 0xFF) + 3, 1)
    ends = np.cumsum(lens)
    return ends - lens, lens


def token_at(tokens, starts, pos):
    """the decoded token that starts at `pos`: ("M", distance, length) | ("L",), or None when no token starts there"""
    i = int(np.searchsorted(starts, pos))
    if i >= len(starts) or starts[i] != pos:
        return None
    t = int(tokens[i])
    if (t >> 23) & 1:
        return ("M", (t & 0x7FFF) + 1, ((t >> 15) & 0xFF) + 3)
    return ("L",)


def missed(case, tokens):
    """the first (position, wanted, found) of case.want that the token list does not show, or None"""
    starts, _ = token_starts(tokens)
    for pos, w in case.want:
        got = token_at(tokens, starts, pos)
        if got != w:
            return pos, w, got
    return None
