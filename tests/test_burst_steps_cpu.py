"""The inputs of tests/_burst_cases.py hold what they say (CPU only): the call's bucket has exactly k members and the j-th is the
first that passes the filter (a model of the chain, checked again here on the finished bytes), and the oracle's token list shows
the planted tokens at the planted positions, at the case's level.  A case that stops being live fails here instead of passing
silently on the GPU (tests/test_gpu_burst_steps.py).  No case is left out; the sizes of the lists are asserted."""
import numpy as np
import pytest

import _burst_cases as B
import _oracle as O
import _planted as P
from _adversarial import LV

GROUPS = B.groups()


def test_list_sizes():
    n = {gid: len(fn()) for gid, _, fn in GROUPS}
    assert n == {"anchor-L4": 57, "anchor-L5": 66, "lazy-L5": 65, "anchor-L6": 75, "lazy-L6": 74, "anchor-L7": 75, "lazy-L7": 74,
                 "special-L6": 3}
    for lv in B.LEVELS:
        chain, quarter = B.budgets(lv)
        for kind in ("anchor", "lazy"):
            cases = B.walk_cases(lv, kind)
            if kind == "lazy" and lv == 4:
                assert cases == () and LV[4][1] == 4   # lazy = 4: no call of level 4 has a match in hand
                continue
            budget = quarter if kind == "lazy" else chain
            ks = {c.k for c in cases}
            assert set(range(2 if kind == "lazy" else 1, 21)) <= ks
            assert {quarter - 1, quarter, quarter + 1, chain - 1, chain, chain + 1} <= ks | {1}
            for k in ks:
                js = {c.j for c in cases if c.k == k}
                assert js == {1, (1 + min(k, budget)) // 2, min(k, budget)}
            assert len({c.name for c in cases}) == len(cases)
            assert max(len(c.data) for c in cases) <= 65535
    assert {k for k in range(127, 130)} <= {c.k for c in B.walk_cases(6, "anchor")}
    assert {31, 32, 33} <= {c.k for c in B.walk_cases(6, "lazy")}


@pytest.mark.parametrize("gid,level,fn", GROUPS, ids=[g[0] for g in GROUPS])
def test_every_case_is_live(gid, level, fn):
    bad = []
    for c in fn():
        buf = np.frombuffer(c.data, np.uint8)
        if c.kind in ("anchor", "lazy", "lone"):
            chain = B.members(buf, c.p)
            got = (len(chain), B.first_pass(buf, c.p, chain, B.HAND_L if c.kind == "lazy" else 0))
            if got != (c.k, c.j):
                bad.append((c.name, "bucket", got))
        tokens = O.tokenize(c.data, level)
        m = P.missed(P.Case(c.name, c.kind, None, c.p, c.data, c.want, 0), tokens)
        if m is not None:
            bad.append((c.name, "token") + m)
    assert not bad, (gid, len(bad), bad[:5])


def test_special_cases_geometry():
    cut, kept, lone = B.special_cases()
    for c in (cut, kept):
        buf = np.frombuffer(c.data, np.uint8)
        # the two calls are the first positions of two 48-byte segments of one block of 64 segments
        assert B.CUT_PX % 48 == 0 and B.CUT_PY % 48 == 0 and B.CUT_PX // 3072 == B.CUT_PY // 3072 and len(c.data) == 65535
        cx, cy = B.members(buf, B.CUT_PX), B.members(buf, B.CUT_PY)
        assert len(cx) == 3 and B.first_pass(buf, B.CUT_PX, cx, 0) == 3
        assert len(cy) == 4 and B.first_pass(buf, B.CUT_PY, cy, 0) == 4
        assert B.CUT_PY - cy[2] <= 32768 and B.CUT_PY - cy[3] == (32773 if c.kind == "cut" else 32768)
    assert lone.p == B.LONE_P and (lone.k, lone.j) == (60, 41)
    buf = np.frombuffer(lone.data, np.uint8)
    assert max(B.members(buf, lone.p)) < 3072
    h = [int(x) for x in B.hashes(buf)]
    for q in range(3072, len(h)):
        if not lone.p <= q <= lone.p + B.ANCHOR_L - 4:
            assert h[q] not in h[1:q], q
