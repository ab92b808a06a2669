"""The cases of tests/assign_cases.py are sound, shown without a GPU: the scipy reference (a non-finite entry = a forbidden pair) finds
the least value over ALL matchings on every kind of matrix small enough to enumerate, and every kind holds matrices whose optimum
is NOT unique -- forbidding a chosen pair and solving again gives the same value -- so that the tie rule of the solver's cross-lane
reduction decides something in tests/test_gpu_assign_edges.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_cases as AC  # noqa: E402


@pytest.mark.parametrize('kind', AC.KINDS)
def test_reference_equals_brute_force(kind):
    seen = 0
    for n in range(1, 5):
        for m in range(1, 5):
            cost, limit, exact = AC.make(kind, n, m)
            pair, v = AC.reference(cost, limit)
            best = AC.brute_force(cost, limit)
            AC.check(cost, limit, exact, pair, best)
            assert v == best if exact else abs(v - best) <= AC.REL * abs(best), (n, m, v, best)
            seen += 1
    assert seen == 16


@pytest.mark.parametrize('kind', AC.KINDS)
def test_every_kind_holds_ties(kind):
    """nonfinite_all has no pair to forbid: its only matching leaves every row unassigned, which is what is asserted for it."""
    tied = 0
    for n, m in AC.SHAPES:
        cost, limit, exact = AC.make(kind, n, m)
        pair, v = AC.reference(cost, limit)
        if kind == 'nonfinite_all':
            assert np.all(pair == -1) and v == n * limit and not np.isfinite(cost).any()
            continue
        for r in np.flatnonzero(pair >= 0)[:8]:
            alt = cost.copy()
            alt[r, pair[r]] = np.nan
            v2 = AC.reference(alt, limit)[1]
            assert v2 >= v - AC.REL * abs(v)                              # (forbidding a pair cannot improve the optimum)
            if v2 == v:
                tied += 1
                break
    print(kind, 'matrices with more than one optimum:', tied, 'of', len(AC.SHAPES))
    assert kind == 'nonfinite_all' or tied > 0


def test_the_case_list():
    cases = AC.cases()
    assert len(set(cases)) == len(cases) == len(AC.KINDS) * 9 + 2
    for shape in [(1, 1), (1, 64), (1, 65), (64, 1), (65, 129), (130, 64), (1, 512), (512, 1), (512, 511)]:
        assert sorted(k for k, n, m in cases if (n, m) == shape) == sorted(AC.KINDS)
    assert sorted(k for k, n, m in cases if (n, m) == (512, 512)) == sorted(AC.FULL_KINDS) and len(AC.FULL_KINDS) == 2
    for kind, n, m in cases:
        if (n, m) in AC.SHAPES:
            cost, limit, exact = AC.make(kind, n, m)
            assert cost.shape == (n, m) and cost.dtype == np.float64 and np.isfinite(limit) and not np.isneginf(cost).any()
            if exact:
                f = cost[np.isfinite(cost)]
                assert np.all(f == np.round(f)) and np.all(np.abs(f) <= 2 ** 20) and limit == round(limit)
            bad = ~np.isfinite(cost)
            assert bad.any() == kind.startswith('nonfinite')
            if kind == 'nonfinite_scatter' and n * m >= 64:
                assert 0.1 < bad.mean() < 0.3 and np.isnan(cost).any() and np.isposinf(cost).any()
            if kind == 'nonfinite_row':
                assert bad.all(1).sum() == 1 and bad.sum() == m
            if kind == 'nonfinite_col':
                assert bad.all(0).sum() == 1 and bad.sum() == n
            if kind in ('mot_scores', 'clear_bonus'):
                assert limit == 0 and np.all(cost <= 0) and (min(n, m) < 8 or (cost == 0).mean() > 0.5)
            if kind == 'clear_bonus' and n * m >= 64:
                assert (cost <= -1000).any() and not ((cost < 0) & (cost > -0.5)).any()
