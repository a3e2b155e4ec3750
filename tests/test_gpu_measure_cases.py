"""GPU parity of the tokenizer on the measure matrices of tests/_measure_cases.py: one fenced match of every length around 8 and
16 bytes, at every alignment of its two sides and every (p - q) % 16, at the end of the input (with background or with zeros
behind the source: what the window's padding holds behind the copy) and in sub-pass B's re-based window.  Every list goes through
compress_many as one batch at its level; every status is 0 and every stream is the oracle's.
tests/test_measure_cases_cpu.py shows, without a GPU, that every input holds the match its name says."""
import numpy as np
import pytest

import _measure_cases as M
import _oracle as O
import _planted as P
from gpu_util import engine

pytestmark = pytest.mark.gpu


def _first_difference(eng, case, level):
    """the case alone: its name, the first token that differs from the oracle's and that token's position in the input"""
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


def _check_parity(eng, cases, level):
    outs, st = eng.compress_many([c.data for c in cases], O.RAW, level)
    assert st == [0] * len(cases), (level, [(c.name, s) for c, s in zip(cases, st) if s][:5])
    bad = [i for i, (c, got) in enumerate(zip(cases, outs)) if got != O.compress(c.data, O.RAW, level)]
    if bad:
        raise AssertionError("%d of %d differ from the oracle: %s; the first of them alone: %s" % (
            len(bad), len(cases), [cases[i].name for i in bad[:20]], _first_difference(eng, cases[bad[0]], level)))


@pytest.mark.parametrize("level", M.LEVELS)
@pytest.mark.parametrize("group", sorted(M.GROUPS))
def test_measure_cases(group, level):
    _check_parity(engine(), M.GROUPS[group](), level)
