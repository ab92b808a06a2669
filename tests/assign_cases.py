"""Seeded cost matrices for the tests of the assignment solver alone (csrc/assign.h through romp_track_assign); a helper, not a
conftest, and nothing here runs a solver on import.

The kinds are the inputs the solver's five callers can hand it and that uniform(0, 600) never produces: small integer alphabets
(ties everywhere), constant matrices, the -score matrices of csrc/mot.hip (limit 0, mostly exact zeros, CLEAR's 1000 bonus), and
non-finite entries, which mean "this pair is forbidden".  Optima tie, so a result is judged by its VALUE, the sum over the rows of
(the cost of its pair, or `limit`), and by its structure -- never by which of the equal optima it is.

`exact` says that every entry and the limit are whole numbers of magnitude <= 2^20: every partial sum of at most 1024 of them is a
whole number below 2^53, exact in float64 in any order, so the value of the device's answer must EQUAL the reference's.  Otherwise
the bound is the 1e-12 relative of test_gpu_track.test_assign_alone.
"""
import itertools

import numpy as np
from scipy.optimize import linear_sum_assignment

KINDS = ('alphabet', 'all_limit', 'zeros', 'mot_scores', 'clear_bonus', 'nonfinite_scatter', 'nonfinite_row', 'nonfinite_col',
         'nonfinite_all')
SHAPES = [(1, 1), (1, 64), (1, 65), (64, 1), (65, 129), (130, 64)]      # a lane's second column, rows past one wave, both at once
CAP_SHAPES = [(1, 512), (512, 1), (512, 511)]                           # the caps of the ABI, each side alone and together
FULL = (512, 512)                                                       # the largest solve: two kinds only (about n^2 / 2 steps of one wave)
FULL_KINDS = ('alphabet', 'nonfinite_scatter')
REL = 1e-12


def make(kind, n, m):
    """-> (cost (n, m) float64, limit, exact)"""
    rs = np.random.RandomState((KINDS.index(kind) * 1000003 + n * 1009 + m) % (2 ** 31))
    limit = float(rs.randint(-2, 5))
    alphabet = rs.randint(-3, 6, (n, m)).astype(np.float64)
    if kind == 'alphabet':
        return alphabet, limit, True
    if kind == 'all_limit':
        return np.full((n, m), limit), limit, True
    if kind == 'zeros':
        return np.zeros((n, m)), 0., True
    if kind in ('mot_scores', 'clear_bonus'):
        # an IoU-like score: a few positive entries in a row, exact zeros elsewhere; row r overlaps the columns near r m / n
        score = np.zeros((n, m))
        near = (np.arange(n) * m) // n
        for d in (-1, 0, 1, 2):
            c = near + d
            ok = (c >= 0) & (c < m) & (rs.rand(n) < 0.7)
            score[np.arange(n)[ok], c[ok]] = rs.rand(int(ok.sum()))
        score[rs.rand(n, m) < 0.02] = 0.5                                # the same score in many places: ties among positive pairs
        if kind == 'clear_bonus':                                       # csrc/mot.hip: (1000 for the pair of the frame before) + v, 0 under the threshold
            bonus = np.zeros((n, m))
            keep = rs.rand(n) < 0.5
            keep[0] = True
            bonus[np.arange(n)[keep], near[keep]] = 1000.
            score[np.arange(n)[keep], near[keep]] = 0.5 + 0.5 * rs.rand(int(keep.sum()))
            score = np.where(score < 0.5, 0., bonus + score)
        return -score, 0., False
    bad = np.zeros((n, m), bool)
    if kind == 'nonfinite_scatter':
        bad = rs.rand(n, m) < 0.2
    elif kind == 'nonfinite_row':
        bad[rs.randint(n)] = True
    elif kind == 'nonfinite_col':
        bad[:, rs.randint(m)] = True
    elif kind == 'nonfinite_all':
        bad[:] = True
    else:
        raise ValueError(kind)
    cost = alphabet.copy()
    cost[bad] = np.where(rs.rand(int(bad.sum())) < 0.5, np.nan, np.inf)  # (no -inf: nothing defines it and no caller can produce it)
    return cost, limit, True


def cases():
    """-> [(kind, n, m)]"""
    out = [(k, n, m) for n, m in SHAPES + CAP_SHAPES for k in KINDS]
    return out + [(k,) + FULL for k in FULL_KINDS]


def value(cost, limit, pair):
    """The sum over the rows of (the cost of its pair, or limit)."""
    pair = np.asarray(pair)
    hit = pair >= 0
    return float(cost[np.arange(len(pair))[hit], pair[hit]].sum() + (~hit).sum() * limit)


def reference(cost, limit):
    """scipy on tracker.assign's padded matrix, a non-finite entry being a forbidden pair -> (pair_of_row, value)."""
    n, m = cost.shape
    padded = np.zeros((n + m, n + m))
    padded[:n, :m] = np.where(np.isfinite(cost), cost, np.inf)
    padded[:n, m:] = padded[n:, :m] = limit / 2.
    rows, cols = linear_sum_assignment(padded)
    pair = np.full(n, -1)
    for r, c in zip(rows, cols):
        if r < n and c < m:
            pair[r] = c
    return pair, value(cost, limit, pair)


def brute_force(cost, limit):
    """The least value over ALL matchings (n, m <= 4): every row takes a distinct column or none; a non-finite pair is never taken."""
    n, m = cost.shape
    best = np.inf
    for choice in itertools.product(range(-1, m), repeat=n):
        cols = [c for c in choice if c >= 0]
        if len(set(cols)) != len(cols) or any(c >= 0 and not np.isfinite(cost[r, c]) for r, c in enumerate(choice)):
            continue
        best = min(best, value(cost, limit, np.asarray(choice)))
    return best


def check(cost, limit, exact, got, want_value):
    """What every answer of the solver must satisfy; `got` is pair_of_row."""
    n, m = cost.shape
    got = np.asarray(got)
    assert got.shape == (n,) and np.all(got >= -1) and np.all(got < m), got
    cols = got[got >= 0]
    assert len(np.unique(cols)) == len(cols), 'a column is used twice'
    assert np.all(np.isfinite(cost[np.arange(n)[got >= 0], cols])), 'a pair of non-finite cost was chosen'
    v = value(cost, limit, got)
    if exact:
        assert v == want_value, (v, want_value)
    else:
        assert abs(v - want_value) <= REL * abs(want_value), (v, want_value)
