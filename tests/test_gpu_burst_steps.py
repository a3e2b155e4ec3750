"""GPU parity of the tokenizer's chain walk on the lists of tests/_burst_cases.py: one call whose chain has exactly k members, the
j-th the first to pass the filter -- k from 1 to 20 and around both budgets of the level, as an anchor's call and as a lazy call
with a match in hand, at levels 4 to 7; a walk that ends on the distance limit in the step another lane of its wave hits; a lane
that walks alone for 40 steps.  Every list goes through compress_many as one batch at its level; every status is 0 and every
stream is the oracle's.  tests/test_burst_steps_cpu.py shows, without a GPU, that every input holds the walk its name says."""
import numpy as np
import pytest

import _burst_cases as B
import _oracle as O
import _planted as P
from gpu_util import engine

pytestmark = pytest.mark.gpu

GROUPS = B.groups()


def _first_difference(eng, case, level):
    """the case alone: the first token that differs from the oracle's and that token's position in the input"""
    outs, st = eng.compress_many([case.data], O.RAW, level)
    got = eng.debug_tokens(0)
    want = O.tokenize(case.data, level)
    m = min(len(got), len(want))
    bad = np.nonzero(got[:m] != want[:m])[0]
    first = int(bad[0]) if bad.size else m
    starts, _ = P.token_starts(want)
    return {"case": case.name, "p": case.p, "planted": case.want, "level": level, "status alone": st, "token": first,
            "position": int(starts[first]) if first < len(want) else len(case.data),
            "got": O.tok_decode(got[first]) if first < len(got) else None,
            "want": O.tok_decode(want[first]) if first < len(want) else None,
            "alone": "same bytes as the oracle" if outs[0] == O.compress(case.data, O.RAW, level) else "differs too"}


@pytest.mark.parametrize("gid,level,fn", GROUPS, ids=[g[0] for g in GROUPS])
def test_burst_steps(gid, level, fn):
    eng, cases = engine(), fn()
    outs, st = eng.compress_many([c.data for c in cases], O.RAW, level)
    assert st == [0] * len(cases), (level, [(c.name, s) for c, s in zip(cases, st) if s][:5])
    bad = [i for i, (c, got) in enumerate(zip(cases, outs)) if got != O.compress(c.data, O.RAW, level)]
    if bad:
        raise AssertionError("%d of %d differ from the oracle: %s; the first of them alone: %s" % (
            len(bad), len(cases), [cases[i].name for i in bad[:20]], _first_difference(eng, cases[bad[0]], level)))
