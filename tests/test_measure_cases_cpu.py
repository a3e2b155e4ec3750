"""The inputs of tests/_measure_cases.py hold what they say (CPU only): in the oracle's token list EVERY case has
("M", distance, length) exactly at the copy's position, at each of the levels the GPU test runs them at.  A case that stops
holding its match fails here instead of passing silently on the GPU (tests/test_gpu_measure_cases.py).  No case is left out; the
sizes of the matrices are asserted, so that a later thinning shows."""
import pytest

import _measure_cases as M
import _oracle as O
import _planted as P


def _missed(cases, level):
    bad = []
    for c in cases:
        tokens = O.tokenize(c.data, level)
        starts, _ = P.token_starts(tokens)
        got = P.token_at(tokens, starts, c.p)
        if got != c.want:
            bad.append((c.name, c.p, c.want, got))
    return bad


def test_matrix_sizes():
    assert len(M.small_cases()) == M.N_SMALL == 9408
    assert len(M.end_cases()) == M.N_END == 408
    assert len(M.subb_cases()) == M.N_SUBB == 144
    for fn in M.GROUPS.values():
        assert len({c.name for c in fn()}) == len(fn())
    # the small matrix: every (p - q) % 16 with every alignment of q for the short lengths, source and copy apart
    for c in M.small_cases():
        d, L = c.want[1], c.want[2]
        assert d >= L + 1 and c.p == 64 + int(c.name.split("_ph")[1].split("_")[0]) + d
    assert {(c.want[1] % 16, c.p % 16) for c in M.small_cases() if c.want[2] <= 20} == {(r, a) for r in range(16) for a in range(16)}
    # the end of the input: the copy's last byte is the input's last
    for c in M.end_cases():
        assert len(c.data) == c.p + c.want[2] and c.want[1] == c.want[2] + 24
    zero = [c for c in M.end_cases() if c.name.endswith("_zero")]
    assert len(zero) == M.N_END // 2
    for c in zero:
        q = c.p - c.want[1]
        assert c.data[q + c.want[2]:q + c.want[2] + 20] == bytes(20)
    # sub-pass B: p = 51456 + ph in a chunk of 52 KiB
    assert {c.p for c in M.subb_cases()} == set(range(M.SUBB_P, M.SUBB_P + 16))
    assert {len(c.data) for c in M.subb_cases()} == {M.SUBB_N}


@pytest.mark.parametrize("level", M.LEVELS)
@pytest.mark.parametrize("group", sorted(M.GROUPS))
def test_every_case_holds_its_match(group, level):
    cases = M.GROUPS[group]()
    bad = _missed(cases, level)
    assert not bad, (group, level, len(bad), len(cases), bad[:5])
