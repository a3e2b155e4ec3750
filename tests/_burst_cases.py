"""Inputs for the tokenizer's CHAIN WALK (test infrastructure; pure numpy, no GPU import).  k_lz_parse walks a call's hash chain
in bursts of 18 steps that are written out by hand: in every step a lane may leave because its candidate passes the four-byte
filter, because the chain ends, because the next candidate lies beyond the distance limit or because the call's budget is spent,
and the test for "no lane walks any more" stands behind some of the steps only.  What can go wrong depends on the STEP a walk
ends in.  So every case here fixes the walk of ONE call:

  the call's hash bucket holds exactly k earlier positions (its chain has k members), and the j-th of them, nearest first, is the
  first whose bytes pass the call's filter -- a true copy of the call's own bytes, which the oracle's token list must show.

The other members are positions whose four bytes only share the HASH (deflate's hash is a multiplication by an odd constant, so
the words of a bucket are found by multiplying back), and, behind the j-th or in a lazy call, short copies of the call's first
four to seven bytes, which share the hash and fail the filter where the match in hand ends.

  anchor kind   nothing in hand: the call at p has the whole budget `chain`; the copy is 8 bytes long.
  lazy kind     a match of 8 bytes (= `good` at levels 5..7) in hand from p - 1: the call at p has `chain >> 2`; the copy is 12
                bytes.  The source s of the match in hand puts s + 1 into p's bucket (its bytes 1..7 ARE p's first seven); it
                fails the filter on the byte behind that match.  It is counted among the k: the farthest member, or the nearest
                when j = k.  So k = 1 does not exist in this kind, and level 4 (lazy = 4: every match is emitted at once, no call
                ever has a match in hand) has no lazy kind at all.
  j             1, the middle, and the last member the budget reaches: min(k, budget).  (k = budget + 1 puts one member
                behind the budget; a copy there would not be found by the reference either.)
  k             1 .. 20 -- a walk that ends in every step and role of a burst and in the first two of the next --, and
                budget - 1, budget, budget + 1 for both budgets of the level.

Special cases (level 6):
  cut / kept    two calls at the starts of two segments of ONE wave (positions 33888 and 34272: multiples of 48 in the block of
                3072 bytes that wave 11 parses), so that they start walking in the same step of the same burst.  The first hits
                its third member; the second has three members in reach and a true copy as the fourth, at distance 32773 (cut:
                the walk ends on the distance limit in the very step the other lane hits; the copy must NOT be found) or 32768
                (kept: it is found).
  lone          a call in a block of 3072 bytes that holds nothing else but background: one lane walks alone, 40 members fail,
                the 41st is the copy.

Every case checks itself when it is built (`_check`): the bucket's size and the first member that passes, by a model of the
chain.  A seed that fails -- a stray position of the background in the bucket -- is replaced by the next one.
tests/test_burst_steps_cpu.py asserts the planted tokens against the oracle."""
import functools
import zlib
from typing import NamedTuple

import numpy as np

import _planted as P
from _adversarial import LV

LEVELS = (4, 5, 6, 7)
MULT = 0x9E3779B1
INV = pow(MULT, -1, 1 << 32)
SLOT = 16          # bytes between two members
FIRST = 16         # the farthest member's position
ANCHOR_L, LAZY_L, HAND_L = 8, 12, 8


class Case(NamedTuple):
    name: str
    level: int
    kind: str     # anchor | lazy | cut | kept | lone
    k: int
    j: int
    p: int        # position of the call
    data: bytes
    want: tuple   # ((position, token), ...) of the oracle's token list


def hash4(b):
    return ((int.from_bytes(bytes(b[:4]), "big") * MULT) & 0xFFFFFFFF) >> 17


def hashes(buf):
    """hash of every position that has four bytes"""
    b = np.asarray(buf, np.uint64)
    w = (b[:-3] << np.uint64(24)) | (b[1:-2] << np.uint64(16)) | (b[2:-1] << np.uint64(8)) | b[3:]
    return ((w * np.uint64(MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(17)


def members(buf, p):
    """the chain of the call at p: earlier positions of its bucket, nearest first (position 0 is the chain's null)"""
    h = hashes(buf)
    q = np.nonzero(h[1:p] == h[p])[0] + 1
    return [int(x) for x in q[::-1]]


def first_pass(buf, p, chain, best):
    """number (from 1) of the first member whose four bytes at offset max(best - 3, 0) are the call's; 0: none"""
    off = max(best - 3, 0)
    own = bytes(buf[p + off:p + off + 4])
    for i, q in enumerate(chain):
        if bytes(buf[q + off:q + off + 4]) == own:
            return i + 1
    return 0


def bucket_words(rng, own, n):
    """n different four-byte words of own's bucket, none of them own"""
    h = hash4(own)
    out = []
    while len(out) < n:
        w = (INV * ((h << 17) | int(rng.integers(0, 1 << 17)))) & 0xFFFFFFFF
        b = w.to_bytes(4, "big")
        if b != bytes(own) and b not in out:
            assert hash4(b) == h
            out.append(b)
    return out


def budgets(level):
    chain = LV[level][3]
    return chain, chain >> 2


def k_values(level, kind):
    chain, quarter = budgets(level)
    ks = set(range(1, 21)) | {quarter - 1, quarter, quarter + 1, chain - 1, chain, chain + 1}
    return sorted(k for k in ks if k >= (2 if kind == "lazy" else 1))


def j_values(level, kind, k):
    jmax = min(k, budgets(level)[1 if kind == "lazy" else 0])
    return sorted({1, (1 + jmax) // 2, jmax})


def _rng(name, attempt):
    return np.random.default_rng([0x42555253, zlib.crc32(name.encode()), attempt])


def _plant_members(rng, buf, p, slots, j, L, lazy_src):
    """members at the positions `slots` (nearest first).  The j-th is the copy of buf[p : p + L].  lazy_src: the number of the
    member that is source + 1 of the match in hand (its slot holds the 8 bytes from p - 1), or 0."""
    k = len(slots)
    words = bucket_words(rng, buf[p:p + 4], k)
    for i, q in enumerate(slots, 1):
        if i == j:
            P.copy(rng, buf, q, p, L)
        elif i == lazy_src:
            P.copy(rng, buf, q - 1, p - 1, HAND_L)
        elif (i > j or lazy_src) and i % 2:
            P.copy(rng, buf, q, p, 4 + (i // 2) % 4)   # shares 4 .. 7 bytes: the hash, not the filter behind a match
        else:
            buf[q:q + 4] = np.frombuffer(words[i - 1], np.uint8)


def _check(buf, p, k, j, best):
    chain = members(buf, p)
    return len(chain) == k and first_pass(buf, p, chain, best) == j


def _build(name, level, kind, k, j, make):
    for attempt in range(200):
        got = make(_rng(name, attempt))
        if got is not None:
            buf, p, want = got
            return Case(name, level, kind, k, j, p, buf.tobytes(), want)
    raise AssertionError("no seed gives the bucket of " + name)


def _walk_case(level, kind, k, j, gap=0, name=None, also=None):
    """one call with k members, the j-th the copy; gap: background bytes between the nearest member and the call; also(buf, p):
    one more condition on the seed"""
    lazy = kind == "lazy"
    name = name or "%s/L%d_k%d_j%d" % (kind, level, k, j)

    def make(rng):
        p = FIRST + k * SLOT + 8 + lazy + gap
        L = LAZY_L if lazy else ANCHOR_L
        buf = P.junk(rng, p + L + 40)
        buf[p - lazy:p + L] = P.fresh(rng, L + lazy)
        slots = [FIRST + (k - i) * SLOT + 4 for i in range(1, k + 1)]   # nearest first
        _plant_members(rng, buf, p, slots, j, L, (1 if j == k else k) if lazy else 0)
        if lazy:
            if members(buf, p - 1) != [slots[(0 if j == k else k - 1)] - 1]:   # the call before: one member, the match in hand
                return None
            want = ((p - 1, ("L",)), (p, ("M", p - slots[j - 1], L)))
        else:
            want = ((p, ("M", p - slots[j - 1], L)),)
        ok = _check(buf, p, k, j, HAND_L if lazy else 0) and (also is None or also(buf, p))
        return (buf, p, want) if ok else None
    return _build(name, level, kind, k, j, make)


@functools.lru_cache(None)
def walk_cases(level, kind):
    if kind == "lazy" and LV[level][1] <= HAND_L:
        return ()   # (level 4: a match of `lazy` bytes or more is emitted at once)
    return tuple(_walk_case(level, kind, k, j) for k in k_values(level, kind) for j in j_values(level, kind, k))


CUT_PX, CUT_PY, CUT_N = 33888, 34272, 65535


def _cut_case(kind):
    """see the module's text: X hits its third member in the step in which Y's fourth lies beyond (cut) or on (kept) the limit"""
    D = 32773 if kind == "cut" else 32768
    name = "%s/L6_D%d" % (kind, D)

    def make(rng):
        buf = P.junk(rng, CUT_N)
        for p in (CUT_PX, CUT_PY):
            buf[p:p + ANCHOR_L] = P.fresh(rng, ANCHOR_L)
        _plant_members(rng, buf, CUT_PX, [CUT_PX - 12 * i for i in (1, 2, 3)], 3, ANCHOR_L, 0)
        _plant_members(rng, buf, CUT_PY, [CUT_PY - 12, CUT_PY - 24, CUT_PY - 36, CUT_PY - D], 4, ANCHOR_L, 0)
        ok = _check(buf, CUT_PX, 3, 3, 0) and _check(buf, CUT_PY, 4, 4, 0)
        want = ((CUT_PX, ("M", 36, ANCHOR_L)), (CUT_PY, ("M", D, ANCHOR_L) if kind == "kept" else ("L",)))
        return (buf, CUT_PY, want) if ok else None
    return _build(name, 6, kind, 4, 4, make)


LONE_K, LONE_J = 60, 41


LONE_P = 3072 + 247


def _lone_case():
    def alone(buf, p):
        """no other position of the call's block of 3072 bytes has a chain (but those inside the copy, which are the same lane's).
        Random background would put some thirty positions of the block into buckets that are taken: the last byte of such a
        position's word is drawn again (position by position, so a word's first three bytes stand when it is looked at); the
        call's own bytes and the bytes before and behind them stay, a seed that would need them changed is given up."""
        seen = set(int(x) for x in hashes(buf[:3072 + 3])[1:])
        for q in range(3072, len(buf) - 3):
            if p <= q <= p + ANCHOR_L - 4:
                continue
            for _ in range(64):
                if hash4(buf[q:q + 4]) not in seen:
                    break
                if p - 1 <= q + 3 <= p + ANCHOR_L:
                    return False
                buf[q + 3] = 128 + (int(buf[q + 3]) + 37) % 128
            else:
                return False
            seen.add(hash4(buf[q:q + 4]))
        return _check(buf, p, LONE_K, LONE_J, 0)
    c = _walk_case(6, "anchor", LONE_K, LONE_J, gap=LONE_P - (FIRST + LONE_K * SLOT + 8), name="lone/L6_k60_j41", also=alone)
    assert c.p == LONE_P and FIRST + LONE_K * SLOT < 3072
    return c._replace(kind="lone")


@functools.lru_cache(None)
def special_cases():
    return (_cut_case("cut"), _cut_case("kept"), _lone_case())


def groups():
    """(id, level, cases) of every batch the GPU test sends"""
    out = [("%s-L%d" % (kind, lv), lv, functools.partial(walk_cases, lv, kind)) for lv in LEVELS for kind in ("anchor", "lazy")
           if not (kind == "lazy" and LV[lv][1] <= HAND_L)]
    return out + [("special-L6", 6, special_cases)]
