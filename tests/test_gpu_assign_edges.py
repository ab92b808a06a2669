"""The assignment solver alone (csrc/assign.h through romp_track_assign) where its five callers take it and test_assign_alone does
not: ties everywhere, the -score matrices of csrc/mot.hip with limit 0, non-finite costs (a forbidden pair), and the caps of the ABI
(n, m = 512: index m of the solver's column arrays, rows past the second 64, the largest solve there is).

Reference: scipy on tracker.assign's padded matrix with every non-finite entry forbidden (tests/assign_cases.py; test_assign_cases.py
shows it equal to brute force and the cases to hold ties).  Optima tie, so the VALUE is compared -- equal for whole-number matrices,
1e-12 relative otherwise -- plus the structure: entries in [-1, m), no column twice, no pair of non-finite cost.  Only what
assign.h states, "the lowest column on a tie", is pinned beyond that.  Every launch writes between sentinel words that must survive,
and is made twice: equal bytes.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_cases as AC  # noqa: E402

pytestmark = pytest.mark.gpu
SENT_I, PAD = -77777, 5
_REF = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def _solve(dev, cost, limit, timed=False):
    """romp_track_assign into the middle of a buffer of sentinels, twice -> pair_of_row (and the device time of the second launch, ms)."""
    from romp_amd import lib as L
    h = L.load()
    n, m = cost.shape
    c = torch.from_numpy(np.ascontiguousarray(cost)).to(dev)
    outs = []
    ms = None
    for rep in range(2):
        buf = torch.full((PAD + n + PAD,), SENT_I, dtype=torch.int32, device=dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        L.check(h.romp_track_assign(L.ptr(c), n, m, float(limit), L.ptr(buf[PAD:]), L.stream_ptr(dev)))
        t1.record()
        host = buf.cpu().numpy()
        ms = t0.elapsed_time(t1)
        assert np.all(host[:PAD] == SENT_I) and np.all(host[PAD + n:] == SENT_I), 'a word outside pair_of_row was written'
        outs.append(host[PAD:PAD + n])
    assert outs[0].tobytes() == outs[1].tobytes(), 'two launches on the same input differ'
    return (outs[0], ms) if timed else outs[0]


def _reference(kind, n, m):
    if (kind, n, m) not in _REF:
        cost, limit, exact = AC.make(kind, n, m)
        _REF[kind, n, m] = (cost, limit, exact) + AC.reference(cost, limit)
    return _REF[kind, n, m]


@pytest.mark.parametrize('kind,n,m', AC.cases(), ids=lambda v: str(v))
def test_value_and_structure(dev, kind, n, m):
    cost, limit, exact, want_pair, want = _reference(kind, n, m)
    got, ms = _solve(dev, cost, limit, timed=True)
    if n * m >= 512 * 511:
        print('%s %d x %d: one solve %.1f ms on the device, value %.17g' % (kind, n, m, ms, want))
    AC.check(cost, limit, exact, got, want)
    if kind == 'nonfinite_all':
        assert np.all(got == -1)
    if kind == 'nonfinite_row':
        assert got[int(np.flatnonzero(~np.isfinite(cost).any(1))[0])] == -1
    if kind == 'nonfinite_col':
        assert int(np.flatnonzero(~np.isfinite(cost).any(0))[0]) not in got.tolist()


@pytest.mark.parametrize('m', [1, 2, 64, 65, 129, 512])
def test_the_lowest_column_wins_a_tie(dev, m):
    """assign.h: "minimum over the wave, the lowest column on a tie"; "stay unassigned" is column m, after every real one."""
    row = np.full((1, m), 3.)
    assert _solve(dev, row, 5.).tolist() == [0]                         # equal costs under the limit: column 0
    assert _solve(dev, row, 3.).tolist() == [0]                         # ... equal to the limit: still paired, a real column comes first
    assert _solve(dev, row, 2.).tolist() == [-1]                        # ... above it: nobody
    for j in sorted({0, m // 2, m - 1, min(m - 1, 64)}):                # the minimum equals the limit in one column only, wherever it is
        one = np.full((1, m), 7.)
        one[0, j] = -2.
        assert _solve(dev, one, -2.).tolist() == [j]
        two = one.copy()
        two[0, m - 1] = -2.                                             # ... and again in the last column: the lower of the two
        assert _solve(dev, two, -2.).tolist() == [j]
    if m >= 2:                                                          # a NaN or +inf in front of the minimum is passed over
        for bad in (np.nan, np.inf):
            r = np.full((1, m), 3.)
            r[0, 0] = bad
            assert _solve(dev, r, 3.).tolist() == [1]
