"""Centre maps with NaN, +inf and -inf: what the reference's parse returns for them, pinned on the CPU.

The device parses (romp_parse, romp_bev_parse) are tested against the oracles O.parse_centermap / BO.parse_3dcentermap.  The oracles
sort, the reference calls torch.topk, and the two treat a NaN differently: topk ranks it ABOVE everything, so a NaN of the suppressed
map takes one of the K slots and is then masked by `> thresh`; the oracles rank it last (2-D) or never admit it (3-D).  As long as the
NaNs and the real peaks of an image fit into K slots together, both return the same rows.  This file states that condition for every
case (`_check_slots`: a condition on the planted input, not a measurement) and asserts that each oracle equals a direct torch
evaluation of the reference's steps -- max_pool(5,1,2), eq, multiply, topk(K) [per depth, then over the depths, in 3-D], `> thresh`
-- so the GPU tests that import these cases (tests/test_gpu_romp_parse.py, tests/test_gpu_bev_kernels.py) compare with the reference.

What the steps do with the special values: the pool hands a NaN on, so every pixel within two of a NaN has max != value and is
suppressed (value * 0); the NaN pixel itself scores NaN; +inf is a maximum like any other (its finite neighbours score 0); -inf that is
not a window maximum scores -inf * 0 = NaN, and it never exceeds a neighbour, so the pixels around it are unaffected."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from oracle import bev_oracle as BO
from oracle import romp_oracle as O

NAN, PINF, NINF = float('nan'), float('inf'), float('-inf')
THRESH, MAX_PERSON = 0.25, 64

# name -> (B, [(image, (y, x), (z, y, x), value, returned)], images that are NaN all over)
PLANTS = {
    'nan_in_window': (1, [(0, (20, 20), (10, 20, 20), NAN, False), (0, (21, 22), (12, 21, 22), 5.0, False),
                          (0, (40, 40), (30, 40, 40), 0.9, True)], ()),
    'nan_3_away': (1, [(0, (20, 20), (10, 20, 20), NAN, False), (0, (20, 23), (13, 20, 20), 5.0, True),
                       (0, (23, 20), (10, 20, 23), 0.7, True)], ()),
    'nan_corner_edge': (1, [(0, (0, 0), (0, 0, 0), NAN, False), (0, (2, 0), (2, 2, 0), 0.9, False), (0, (0, 3), (0, 0, 3), 0.8, True),
                            (0, (0, 30), (0, 0, 30), NAN, False), (0, (1, 28), (1, 1, 28), 0.95, False), (0, (0, 33), (0, 0, 33), 0.6, True),
                            (0, (63, 63), (63, 127, 127), NAN, False), (0, (61, 62), (61, 126, 125), 0.85, False)], ()),
    'nan_other_image': (2, [(0, (20, 20), (10, 20, 20), NAN, False), (0, (21, 22), (12, 21, 22), 5.0, False),
                            (1, (21, 22), (12, 21, 22), 5.0, True)], ()),
    'all_nan_image': (3, [(0, (10, 10), (5, 10, 10), 0.9, True), (0, (30, 30), (20, 30, 30), 0.8, True),
                          (2, (5, 50), (3, 5, 50), 0.7, True)], (1,)),
    'pos_inf': (1, [(0, (10, 10), (5, 10, 10), PINF, True), (0, (11, 12), (6, 11, 12), 0.95, False),
                    (0, (30, 30), (20, 30, 30), 0.9, True)], ()),
    'two_pos_inf': (1, [(0, (30, 5), (20, 30, 5), PINF, True), (0, (10, 10), (5, 10, 10), PINF, True),
                        (0, (50, 50), (40, 50, 50), 0.9, True)], ()),
    'neg_inf': (1, [(0, (20, 20), (10, 20, 20), NINF, False), (0, (21, 22), (12, 21, 22), 0.9, True),
                    (0, (18, 20), (8, 20, 20), 0.8, True)], ()),
}
NAMES = list(PLANTS)
NAN_NAMES = [n for n in NAMES if n.startswith('nan_') or n == 'all_nan_image']


def _check_slots(B, plants, nan_images):
    """Per image: (values that pass the threshold) + (pixels whose suppressed score is NaN: the NaNs and the isolated -infs) must
    leave one of the K slots free, so that topk's NaN-first order and the oracles' order return the same rows.  An image that is NaN
    all over has no peak to displace: every slot holds a NaN, every slot is masked, in either order."""
    for b in range(B):
        mine = [p for p in plants if p[0] == b]
        if b in nan_images:
            assert not mine
            continue
        peaks = sum(1 for p in mine if p[3] > THRESH)
        nan_scores = sum(1 for p in mine if np.isnan(p[3]) or p[3] == NINF)
        assert peaks + nan_scores <= MAX_PERSON - 1, (b, peaks, nan_scores)


def case_2d(name):
    """-> (centre maps (B,1,64,64) float32, the (image, flat index) pairs that must come back)."""
    B, plants, nan_images = PLANTS[name]
    _check_slots(B, plants, nan_images)
    cm = torch.rand(B, 1, 64, 64, generator=torch.Generator().manual_seed(len(name))).numpy() * np.float32(0.1)
    for b, (y, x), _, v, _ in plants:
        cm[b, 0, y, x] = v
    for b in nan_images:
        cm[b] = NAN
    return cm, sorted((b, y * 64 + x) for b, (y, x), _, _, kept in plants if kept)


def case_3d(name):
    """-> (centre volumes (B,64,128,128) float32 tensor, the (image, z, y, x) tuples that must come back)."""
    B, plants, nan_images = PLANTS[name]
    _check_slots(B, plants, nan_images)
    cm = torch.rand(B, 64, 128, 128, generator=torch.Generator().manual_seed(len(name))) * 0.1 - 0.05
    for b, _, (z, y, x), v, _ in plants:
        cm[b, z, y, x] = v
    for b in nan_images:
        cm[b] = NAN
    return cm, sorted((b, z, y, x) for b, _, (z, y, x), _, kept in plants if kept)


def _canonical(bids, flat, scores):
    """topk leaves the order of equal scores open: rows sorted by image, score descending, flat index."""
    order = np.lexsort((flat, -scores, bids))
    return bids[order], flat[order], scores[order]


def torch_parse_2d(cm, thresh, K):
    t = torch.from_numpy(np.asarray(cm, np.float32))
    nmsd = t * torch.eq(TF.max_pool2d(t, 5, 1, 2), t).float()
    b, c, h, w = nmsd.shape
    sc, ind = torch.topk(nmsd.reshape(b, c, -1), K)
    sc, index = torch.topk(sc.reshape(b, -1), K)
    ind = (ind % (h * w)).reshape(b, -1).gather(1, index)
    mask = sc > thresh
    return _canonical(torch.where(mask)[0].numpy(), ind[mask].numpy(), sc[mask].numpy())


def torch_parse_3d(cm, thresh, K):
    t = torch.as_tensor(cm).float()
    nmsd = t * torch.eq(TF.max_pool3d(t.unsqueeze(1), 5, 1, 2).squeeze(1), t).float()
    b, d, h, w = nmsd.shape
    sc, ind = torch.topk(nmsd.reshape(b, d, -1), K)                 # the K best of every depth
    sc, index = torch.topk(sc.reshape(b, -1), K)                    # the K best of those
    ind = (ind % (h * w)).reshape(b, -1).gather(1, index)
    z = index // K
    mask = sc > thresh
    bids, flat, scores = _canonical(torch.where(mask)[0].numpy(), (z * (h * w) + ind)[mask].numpy(), sc[mask].numpy())
    return bids, np.stack([flat // (h * w), (flat // w) % h, flat % w], 1), scores


def test_topk_ranks_nan_first_and_the_pool_hands_it_on():
    """The two facts the slot condition rests on, for the torch in use."""
    v = torch.tensor([0.5, NAN, PINF, 0.1])
    assert torch.isnan(torch.topk(v, 2).values[0]) and torch.topk(v, 2).values[1] == PINF
    m = torch.zeros(1, 1, 9, 9)
    m[0, 0, 4, 4] = NAN
    assert torch.isnan(TF.max_pool2d(m, 5, 1, 2)[0, 0, 2:7, 2:7]).all() and not torch.isnan(TF.max_pool2d(m, 5, 1, 2)[0, 0, 1]).any()
    m3 = torch.zeros(1, 1, 9, 9, 9)
    m3[0, 0, 4, 4, 4] = NAN
    assert torch.isnan(TF.max_pool3d(m3, 5, 1, 2)[0, 0, 2:7, 2:7, 2:7]).all() and int(torch.isnan(TF.max_pool3d(m3, 5, 1, 2)).sum()) == 125


@pytest.mark.parametrize('name', NAMES)
def test_oracle_2d_equals_the_reference_steps(name):
    cm, kept = case_2d(name)
    assert np.isnan(cm).any() or np.isinf(cm).any()
    want = torch_parse_2d(cm, THRESH, MAX_PERSON)
    got = O.parse_centermap(cm, THRESH, MAX_PERSON)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert sorted(zip(got[0].tolist(), got[1].tolist())) == kept
    assert not np.isnan(got[2]).any() and not np.isneginf(got[2]).any()
    if 'pos_inf' in name:                                           # +inf first, two of them by flat index
        n = 2 if name == 'two_pos_inf' else 1
        assert np.isposinf(got[2][:n]).all() and np.isfinite(got[2][n:]).all() and (np.diff(got[1][:n]) > 0).all()


@pytest.mark.parametrize('name', NAMES)
def test_oracle_3d_equals_the_reference_steps(name):
    cm, kept = case_3d(name)
    want = torch_parse_3d(cm, THRESH, MAX_PERSON)
    got = BO.parse_3dcentermap(cm, THRESH, MAX_PERSON)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert sorted((int(b),) + tuple(r) for b, r in zip(got[0], got[1].tolist())) == kept
    if 'pos_inf' in name:
        n = 2 if name == 'two_pos_inf' else 1
        assert np.isposinf(got[2][:n]).all() and np.isfinite(got[2][n:]).all()
