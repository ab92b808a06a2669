"""Benchmark scoring (romp_eval_match2d / romp_eval_points / romp_eval_accumulate, romp_amd/evaluation.py): the CPU part.
Fixture: tests/golden/eval_metrics.npz, written by the reference's own match_2d_greedy, batch_compute_similarity_transform_torch,
compute_mpjpe and compute_error_verts (scripts/make_golden_eval.py).  Here: a numpy float64 restatement of the three kernels
(`match2d_np`, `points_np`, `accumulate_np`, and `summary_np` straight from the rows), checked against that fixture -- matches,
false positives and misses exactly, errors and sRt within the deviation the fixture measured between the reference's float32
and float64 -- plus the properties that make the fixture worth having.  tests/test_gpu_eval_metrics.py holds the kernels to
this restatement."""
import functools
import json
import os
import re

import numpy as np
import pytest

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROCRUSTES = ('j14', 'reflect', 'planar', 'collinear', 'p3', 'far', 'masked', 'verts')
RANK1 = ('collinear',)                    # R (and with it t) is not unique there; aligned points, errors and scale are
N_MATCH, TIE_CASE, CAP_CASE = 7, 1, 6
STRIDE = 53


@functools.lru_cache(None)
def golden():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'eval_metrics.npz')) as z:
        return {k: z[k] for k in z.files}


def quat_rot(w, x, y, z):
    n = w * w + x * x + y * y + z * z
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], np.float64) / n


@functools.lru_cache(None)
def verts_inputs(n=4, p=6890):
    """The closed formula of scripts/make_golden_eval.py verts_inputs (integer and correctly rounded float64 arithmetic)."""
    i = np.arange(p, dtype=np.int64)[None, :, None]
    k = np.arange(n, dtype=np.int64)[:, None, None]
    c = np.arange(3, dtype=np.int64)[None, None, :]
    pred = (((i * (37 + 6 * c) + 101 * k + 17 * c) % 1009).astype(np.float64) / 1009.0 - 0.5) * np.array([0.3, 0.9, 0.2])
    noise = (((i * (53 + 4 * c) + 29 * k + 7 * c) % 997).astype(np.float64) / 997.0 - 0.5) * 0.02
    pred = pred.astype(F)
    x, y, z = (pred[..., a].astype(np.float64) for a in range(3))
    target = np.empty((n, p, 3), np.float64)
    for m in range(n):
        R = quat_rot(1 + m, 2, 2, 4)
        s, t = 0.8 + 0.125 * m, (0.25 * m, -0.5, 2.0 + m)
        for r in range(3):
            target[m, :, r] = s * ((R[r, 0] * x[m] + R[r, 1] * y[m]) + R[r, 2] * z[m]) + t[r]
    return pred, (target + noise).astype(F)


def procrustes_case(name):
    """-> pred, target (N,P,3) float32, point mask (P,) or None, the index of the stored aligned points."""
    g = golden()
    if name == 'verts':
        return verts_inputs() + (None, slice(None, None, STRIDE))
    mask = g.get(name + '_mask')
    return g[name + '_pred'], g[name + '_target'], mask, (slice(None) if mask is None else mask)


def match_case(k):
    g = golden()
    return g[f'm{k}_pred'], g[f'm{k}_gt'], g[f'm{k}_valid']


def match_batch(cases=range(N_MATCH)):
    """The matching cases as the images of one call -> pred (Np,J,2), pred ids, gt, valid, gt ids, B."""
    ps, gs, vs, pi, gi = [], [], [], [], []
    for b, k in enumerate(cases):
        p, g, v = match_case(k)
        ps.append(p); gs.append(g); vs.append(v)
        pi += [b] * len(p); gi += [b] * len(g)
    return (np.concatenate(ps), np.asarray(pi, np.int64), np.concatenate(gs), np.concatenate(vs), np.asarray(gi, np.int64), len(list(cases)))


def offsets(ids, B):
    return np.searchsorted(ids, np.arange(B + 1)).astype(np.int32)


# ------------------------------------------------------------------------------------------------ restatement
def pair_errors_np(pred, gt, valid, norm='frobenius'):
    """(P,G) float32: the norm of pred[p] - gt[g] over g's valid joints."""
    P, G = len(pred), len(gt)
    e = np.zeros((P, G), F)
    for p in range(P):
        for g in range(G):
            d = (pred[p] - gt[g])[valid[g].astype(bool)].astype(F)
            sxx, syy, sxy = F((d[:, 0] * d[:, 0]).sum()), F((d[:, 1] * d[:, 1]).sum()), F((d[:, 0] * d[:, 1]).sum())
            if norm == 'spectral':
                h, q = F(0.5) * (sxx + syy), F(0.5) * (sxx - syy)
                e[p, g] = np.sqrt(h + np.sqrt(q * q + sxy * sxy))
            else:
                e[p, g] = np.sqrt(sxx + syy)
    return e


def box_iou_np(a, b):
    """get_bbx_overlap over all joints, float32, +1 widths."""
    one = F(1)
    a1, a2, b1, b2 = a.min(0), a.max(0), b.min(0), b.max(0)
    w = max(F(0), min(a2[0], b2[0]) - max(a1[0], b1[0]) + one)
    h = max(F(0), min(a2[1], b2[1]) - max(a1[1], b1[1]) + one)
    inter = F(w * h)
    return inter / ((a2[0] - a1[0] + one) * (a2[1] - a1[1] + one) + (b2[0] - b1[0] + one) * (b2[1] - b1[1] + one) - inter)


def match2d_np(pred, poff, gt, valid, goff, iou_thresh=0.05, max_pred=64, max_gt=64, norm='frobenius'):
    """romp_eval_match2d -> gt_of_pred (Np,), pred_of_gt (Ng,), over_cap (B,)."""
    pred, gt = np.asarray(pred, F), np.asarray(gt, F)
    B = len(poff) - 1
    gt_of_pred, pred_of_gt, over = np.full(len(pred), -1, np.int32), np.full(len(gt), -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        p0, g0 = poff[b], goff[b]
        P, G = poff[b + 1] - p0, goff[b + 1] - g0
        if P > max_pred or G > max_gt:
            over[b] = 1
            continue
        if P == 0 or G == 0:
            continue
        err = pair_errors_np(pred[p0:p0 + P], gt[g0:g0 + G], valid[g0:g0 + G], norm).reshape(-1)
        n_match = n_fp = 0
        p_free, g_free = np.ones(P, bool), np.ones(G, bool)
        while n_match < G and n_match + n_fp < P and np.isfinite(err).any():
            i = int(np.argmin(err))
            p, g = divmod(i, G)
            err[i] = np.inf
            iou = box_iou_np(pred[p0 + p], gt[g0 + g])
            if p_free[p] and g_free[g] and iou >= F(iou_thresh):
                p_free[p] = g_free[g] = False
                gt_of_pred[p0 + p], pred_of_gt[g0 + g] = g0 + g, p0 + p
                n_match += 1
            elif iou < F(iou_thresh):
                n_fp += 1
    return gt_of_pred, pred_of_gt, over


def procrustes_np(a, b):
    """evaluation_matrix.py:252-303 for one person, (P,3) float64 -> aligned, sRt (13,), singular values of K."""
    mu1, mu2 = a.mean(0), b.mean(0)
    X1, X2 = (a - mu1).T, (b - mu2).T
    var1 = (X1 ** 2).sum()
    K = X1 @ X2.T
    U, s, Vh = np.linalg.svd(K)
    V = Vh.T
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(U @ V.T))
    R = V @ Z @ U.T
    with np.errstate(all='ignore'):
        scale = np.trace(R @ K) / var1
        t = mu2 - scale * (R @ mu1)
    return scale, R, t, s, np.linalg.det(U @ V.T)


def points_np(pred, target, pred_of_gt=None, align_inds=None, vis=None, point_mask=None):
    """romp_eval_points in float64 -> dict mpjpe, mpjpe_all, pa_mpjpe (Ng,), sRt (Ng,13), aligned (Ng,P,3), sigma (Ng,3)."""
    pred, target = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    Ng, P = target.shape[:2]
    out = {'mpjpe': np.full(Ng, np.nan), 'mpjpe_all': np.full(Ng, np.nan), 'pa_mpjpe': np.full(Ng, np.nan),
           'sRt': np.full((Ng, 13), np.nan), 'aligned': np.full((Ng, P, 3), np.nan), 'sigma': np.full((Ng, 3), np.nan)}
    sel = np.ones(P, bool) if point_mask is None else np.asarray(point_mask).astype(bool)
    for g in range(Ng):
        p = g if pred_of_gt is None else int(pred_of_gt[g])
        if p < 0 or p >= len(pred):
            continue
        a, b = pred[p], target[g]
        if align_inds is not None and len(align_inds):
            a0, b0 = a - a[list(align_inds)].mean(0), b - b[list(align_inds)].mean(0)
        else:
            a0, b0 = a, b
        v = np.ones(P) if vis is None else np.asarray(vis[g], np.float64)
        err = np.linalg.norm(a0 - b0, axis=-1)
        with np.errstate(all='ignore'):
            out['mpjpe'][g] = (err * v).sum() / v.sum()
            out['mpjpe_all'][g] = (err * v).sum() / P
            scale, R, t, s, _ = procrustes_np(a[sel], b[sel])
            al = scale * (a @ R.T) + t
        out['aligned'][g], out['sigma'][g] = al, s
        out['sRt'][g] = np.concatenate([[scale], R.reshape(-1), t])
        out['pa_mpjpe'][g] = np.linalg.norm(al[sel] - b[sel], axis=-1).mean()
    return out


def accumulate_np(acc, metrics, pred_of_gt, gt_of_pred, over=None):
    """romp_eval_accumulate: metrics (M,Ng) as the device stores them (float32)."""
    metrics = np.asarray(metrics, F)
    M = len(metrics)
    for k in range(M):
        fin = np.isfinite(metrics[k])
        acc[2 * k] += metrics[k][fin].astype(np.float64).sum()
        acc[2 * k + 1] += fin.sum()
    acc[2 * M:2 * M + 5] += [(np.asarray(pred_of_gt) < 0).sum(), (np.asarray(gt_of_pred) < 0).sum(), len(pred_of_gt), len(gt_of_pred),
                             0 if over is None else np.asarray(over).astype(bool).sum()]
    return acc


def summary_np(rows, pred_of_gt, gt_of_pred, missing_punish_mm=150.):
    """What MeshEvaluator.summary() reports, straight from the per-row figures (metres) of the whole dataset."""
    pred_of_gt, gt_of_pred = np.asarray(pred_of_gt), np.asarray(gt_of_pred)
    mm = lambda x: float(np.asarray(x, np.float64)[np.isfinite(x)].mean() * 1000.) if np.isfinite(x).any() else float('nan')
    misses, fps, matched = int((pred_of_gt < 0).sum()), int((gt_of_pred < 0).sum()), int((pred_of_gt >= 0).sum())
    cmu = np.asarray(rows['cmu_mpjpe'], np.float64)
    cmu = np.concatenate([cmu[np.isfinite(cmu)] * 1000., np.full(misses, missing_punish_mm)])       # eval_cmu_panoptic.py:306-307
    prec, rec = matched / max(matched + fps, 1), matched / max(len(pred_of_gt), 1)
    return {'MPJPE': mm(rows['mpjpe']), 'PA_MPJPE': mm(rows['pa_mpjpe']), 'PVE': mm(rows['pve']), 'PA_PVE': mm(rows['pa_pve']),
            'CMU_MPJPE': float(cmu.mean()), 'precision': prec, 'recall': rec, 'F1': 2 * prec * rec / (prec + rec),
            'matched': matched, 'misses': misses, 'false_positives': fps, 'n_gt': len(pred_of_gt), 'n_pred': len(gt_of_pred)}


# ------------------------------------------------------------------------------------------------ matching
@pytest.mark.parametrize('norm', ['frobenius', 'spectral'])
@pytest.mark.parametrize('k', range(N_MATCH))
def test_matching_restatement_equals_the_reference(k, norm):
    g = golden()
    pred, gt, valid = match_case(k)
    gop, pog, over = match2d_np(pred, [0, len(pred)], gt, valid, [0, len(gt)], norm=norm)
    assert not over.any()
    matches = sorted((int(p), int(q)) for p, q in enumerate(gop) if q >= 0)
    assert matches == sorted(map(tuple, g[f'm{k}_matches'].tolist()))
    assert all(pog[q] == p for p, q in matches)
    assert np.flatnonzero(gop < 0).tolist() == g[f'm{k}_fp'].tolist()
    assert np.flatnonzero(pog < 0).tolist() == g[f'm{k}_miss'].tolist()


def test_matching_fixture_holds_the_cases_it_was_made_for():
    g = golden()
    assert int(g['n_match_cases']) == N_MATCH
    assert g['m0_matches'].tolist() == [[0, 2], [1, 0]] and g['m0_fp'].tolist() == [2, 3] and g['m0_miss'].tolist() == [1]
    assert (~g['m0_valid']).sum(1).tolist() == [0, 0, 4]
    assert np.array_equal(g['m1_pred'][0], g['m1_pred'][1]) and g['m1_matches'].tolist() == [[0, 0], [2, 1]]
    assert [g[f'm{k}_pred'].shape[0] for k in range(N_MATCH)] == [4, 3, 1, 4, 0, 2, 64]
    assert [g[f'm{k}_gt'].shape[0] for k in range(N_MATCH)] == [3, 2, 3, 1, 2, 0, 5]
    assert len(g['m6_matches']) == 4 and len(g['m6_fp']) == 60 and g['m6_miss'].tolist() == [4]
    # the invalid joints matter: with every joint valid, case 0's restated errors of the true pair (0, 2) more than double
    pred, gt, valid = match_case(0)
    assert pair_errors_np(pred, gt, np.ones_like(valid))[0, 2] > 2 * pair_errors_np(pred, gt, valid)[0, 2]


@pytest.mark.parametrize('norm', ['frobenius', 'spectral'])
def test_pair_errors_are_separated_so_that_float32_order_is_no_coin_toss(norm):
    for k in range(N_MATCH):
        pred, gt, valid = match_case(k)
        if not len(pred) or not len(gt):
            continue
        e = np.sort(pair_errors_np(pred, gt, valid, norm).astype(np.float64).reshape(-1))
        d = np.diff(e)
        ties = d == 0
        assert ties.sum() == (2 if k == TIE_CASE else 0), (k, ties.sum())          # the duplicate prediction: one tie per gt
        assert (d[~ties] / e[1:][~ties]).min(initial=np.inf) >= 1e-3, (k, (d[~ties] / e[1:][~ties]).min())


def test_cap_and_batched_matching_restated():
    pred, pi, gt, valid, gi, B = match_batch()
    poff, goff = offsets(pi, B), offsets(gi, B)
    gop, pog, over = match2d_np(pred, poff, gt, valid, goff)
    assert not over.any()
    for b in range(B):                                                         # global row numbers, image by image
        m = golden()[f'm{b}_matches']
        assert sorted((p - poff[b], q - goff[b]) for p, q in enumerate(gop) if q >= 0 and poff[b] <= p < poff[b + 1]) == \
            sorted(map(tuple, m.tolist()))
    gop2, pog2, over2 = match2d_np(pred, poff, gt, valid, goff, max_pred=63)   # the cap image is over: never truncated
    assert over2.tolist() == [0] * CAP_CASE + [1] and (gop2[poff[CAP_CASE]:] == -1).all() and (pog2[goff[CAP_CASE]:] == -1).all()
    assert np.array_equal(gop2[:poff[CAP_CASE]], gop[:poff[CAP_CASE]])


# ------------------------------------------------------------------------------------------------ Procrustes, MPJPE
@pytest.mark.parametrize('name', PROCRUSTES)
def test_points_restatement_within_the_reference_deviation(name):
    g = golden()
    pred, target, mask, keep = procrustes_case(name)
    r = points_np(pred, target, point_mask=mask)
    slack = 1 + 1e-6
    np.testing.assert_allclose(r['pa_mpjpe'], g[name + '_f64_err'], rtol=1e-10)
    assert (np.abs(r['pa_mpjpe'] - g[name + '_ref_err']) / r['pa_mpjpe']).max() <= float(g[name + '_dev_err']) * slack
    assert np.abs(r['aligned'][:, keep] - g[name + '_ref_aligned']).max() <= float(g[name + '_dev_aligned']) * slack
    assert np.abs(r['aligned'][:, keep] - g[name + '_f64_aligned']).max() <= 1e-10
    ref = g[name + '_ref_sRt'].astype(np.float64)
    assert (np.abs(r['sRt'][:, 0] - ref[:, 0]) / r['sRt'][:, 0]).max() <= float(g[name + '_dev_scale']) * slack
    if name not in RANK1:
        assert np.abs(r['sRt'][:, 1:10] - ref[:, 1:10]).max() <= float(g[name + '_dev_R']) * slack
        assert np.abs(r['sRt'][:, 10:] - ref[:, 10:]).max() <= float(g[name + '_dev_t']) * slack
        R = r['sRt'][:, 1:10].reshape(-1, 3, 3)
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.allclose(np.linalg.det(R), 1.0)


def test_procrustes_fixture_holds_the_cases_it_was_made_for():
    g = golden()
    assert list(g['cases']) == list(PROCRUSTES)
    shapes = {n: procrustes_case(n)[0].shape for n in PROCRUSTES}
    assert all(s[0] in (4, 5) for s in shapes.values())                       # never the 2 or 3 the reference misreads
    assert {n: s[1] for n, s in shapes.items()} == {'j14': 14, 'reflect': 14, 'planar': 17, 'collinear': 10, 'p3': 3, 'far': 24,
                                                    'masked': 17, 'verts': 6890}
    det = lambda n: [procrustes_np(a.astype(np.float64), b.astype(np.float64))[4] for a, b in zip(*procrustes_case(n)[:2])]
    sig = lambda n: np.array([procrustes_np(a.astype(np.float64), b.astype(np.float64))[3] for a, b in zip(*procrustes_case(n)[:2])])
    assert all(d < 0 for d in det('reflect')) and all(d > 0 for d in det('j14'))
    assert (sig('planar')[:, 2] / sig('planar')[:, 0]).max() < 1e-6 and (sig('planar')[:, 1] / sig('planar')[:, 0]).min() > 1e-3
    assert (sig('collinear')[:, 1] / sig('collinear')[:, 0]).max() < 1e-12          # exactly on a line: rank 1
    assert (sig('p3')[:, 2] / sig('p3')[:, 0]).max() < 1e-6                         # three points span a plane
    assert (sig('j14')[:, 2] / sig('j14')[:, 0]).min() > 1e-3
    assert float(g['far_dev_err']) > float(g['j14_dev_err']) and float(g['far_dev_aligned']) > float(g['j14_dev_aligned'])
    assert int(g['masked_mask'].sum()) == 14 and (g['masked_target'][:, ~g['masked_mask']] == -2).all()
    assert 6890 % 64 and 6890 % 256


def test_mpjpe_restatement_against_compute_mpjpe():
    """The reference sums in float32: a norm (4 roundings), the mean of P <= 6890 of them (pairwise, <= 14 levels) and, for
    the root-aligned variants, a subtraction of coordinates below 1.5 m from errors above 0.1 m: 4e-6 relative covers them."""
    g = golden()
    pred, target, vis = g['j14_pred'], g['j14_target'], g['j14_vis']
    np.testing.assert_allclose(points_np(pred, target)['mpjpe'], g['j14_ref_mpjpe'], rtol=4e-6)
    np.testing.assert_allclose(points_np(pred, target, align_inds=[13])['mpjpe'], g['j14_ref_mpjpe_root13'], rtol=4e-6)
    r = points_np(pred, target, align_inds=[13], vis=vis)
    np.testing.assert_allclose(r['mpjpe'], g['j14_ref_mpjpe_root13_vis'], rtol=4e-6)
    np.testing.assert_allclose(r['mpjpe_all'], r['mpjpe'] * vis.sum(1) / 14, rtol=1e-12)
    assert not vis.all() and vis.any(1).all()
    vp, vt = verts_inputs()
    np.testing.assert_allclose(points_np(vp, vt)['mpjpe'], g['verts_ref_pve'], rtol=4e-6)


def test_three_people_the_reference_misreads():
    """batch_compute_similarity_transform_torch on (3,14,3) takes the people for coordinates: its answer for the first three
    people of j14 alone is off by order 1, while the same people inside the batch of 5 agree to 1e-6.  Here inputs are
    always (N,P,3) and the answer does not depend on N."""
    g = golden()
    ours = points_np(g['j14_pred'][:3], g['j14_target'][:3])['pa_mpjpe']
    np.testing.assert_allclose(ours, g['j14_f64_err'][:3], rtol=1e-10)
    np.testing.assert_allclose(g['j14_ref_err'][:3], ours, rtol=2e-6)
    assert (np.abs(g['quirk3_ref_err'] - ours) / ours).max() > 1.0


def test_missing_and_degenerate_rows_restated():
    g = golden()
    pred, target = g['j14_pred'].copy(), g['j14_target']
    pred[2] = pred[2, 0]                                                       # var1 = 0
    r = points_np(pred, target, pred_of_gt=[0, -1, 2, 3, 7])
    assert np.isnan(r['pa_mpjpe'][[1, 4]]).all() and np.isnan(r['mpjpe'][[1, 4]]).all() and not np.isfinite(r['pa_mpjpe'][2])
    np.testing.assert_allclose(r['pa_mpjpe'][[0, 3]], g['j14_f64_err'][[0, 3]], rtol=1e-10)
    assert np.isfinite(r['mpjpe'][2])


def test_accumulator_and_summary_restated():
    from romp_amd import evaluation as E
    rng = np.random.default_rng(0)
    rows = {k: rng.random(9).astype(F) * 0.1 for k in E.METRICS}
    pog = np.array([0, 1, -1, 2, 3, -1, 4, 5, 6])
    gop = np.array([0, 1, 3, 4, 6, 7, 8, -1, -1, -1])
    for k in E.METRICS:
        rows[k][pog < 0] = np.nan
    rows['pve'][:] = np.nan                                                    # no vertices in this dataset
    rows['pa_pve'][:] = np.nan
    acc = np.zeros(2 * len(E.METRICS) + E.ACC_TAIL)
    for sl in (slice(0, 4), slice(4, 9)):                                      # two calls
        accumulate_np(acc, np.stack([rows[k][sl] for k in E.METRICS]), pog[sl], gop[:5] if sl.start == 0 else gop[5:])
    got, want = E.summarize(acc, 150.), summary_np(rows, pog, gop, 150.)
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, err_msg=k)
    assert np.isnan(got['PVE']) and got['misses'] == 2 and got['false_positives'] == 3 and got['matched'] == 7
    acc[-1] = 1
    with pytest.raises(Exception, match='max_pred'):
        E.summarize(acc)


# ------------------------------------------------------------------------------------------------ ABI, CLI
def test_eval_symbols_header_binding_and_library_agree():
    from romp_amd import build, lib
    assert lib.EVAL_EXPORTS == ['romp_eval_match2d', 'romp_eval_points', 'romp_eval_accumulate']
    assert not set(lib.EVAL_EXPORTS) & (set(lib.EXPORTS) | set(lib.VIEW_EXPORTS) | set(lib.MAP_EXPORTS) | set(lib.TEXTURE_EXPORTS))
    assert len(lib.EXPORTS) == 52 and 'eval.hip' in build.SOURCES
    header = open(os.path.join(ROOT, 'include', 'romp_hip_eval.h')).read()
    declared = re.findall(r'^int\s+(romp_\w+)\(', header, re.M)
    assert declared == lib.EVAL_EXPORTS
    h = lib.load()
    assert all(hasattr(h, n) and getattr(h, n).argtypes is not None for n in lib.EVAL_EXPORTS) and h.romp_abi_version() == 7
    for name in declared:                                                      # the binding passes as many arguments as the header declares
        args = re.search(name + r'\((.*?)\);', header, re.S).group(1)
        assert len(getattr(h, name).argtypes) == len(args.split(',')), name
    from romp_amd import evaluation as E
    assert E.ACC_TAIL == int(re.search(r'#define ROMP_EVAL_ACC_TAIL (\d+)', header).group(1))
    assert E.NORMS == {'frobenius': int(re.search(r'#define ROMP_EVAL_NORM_FROBENIUS (\d+)', header).group(1)),
                       'spectral': int(re.search(r'#define ROMP_EVAL_NORM_SPECTRAL\s+(\d+)', header).group(1))}
    assert E.JOINT_SETS['h36m17_to_j14'] == [54 + j for j in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14)]


def stored_files(tmp_path):
    """The matching images with the j14 people as 3-D joints -> a prediction and a ground-truth file of the CLI."""
    from romp_amd import evaluation as E
    pred, pi, gt, valid, gi, B = match_batch()
    g = golden()
    rng = np.random.default_rng(5)
    p3 = g['j14_pred'][rng.integers(0, 5, len(pred))] + rng.standard_normal((len(pred), 1, 3)).astype(F) * F(0.01)
    g3 = g['j14_target'][rng.integers(0, 5, len(gt))]
    vis = rng.random(g3.shape[:2]) > 0.2
    vis[:, 0] = True
    pp, gp = str(tmp_path / 'pred.npz'), str(tmp_path / 'gt.npz')
    E.save_results(pp, kp2d=pred, kp3d=p3, batch_ids=pi)
    E.save_results(gp, kp2d=gt, kp3d=g3, batch_ids=gi, valid=valid, vis=vis, B=B)
    return pp, gp, dict(kp2d=pred, kp3d=p3, batch_ids=pi), dict(kp2d=gt, kp3d=g3, batch_ids=gi, valid=valid, vis=vis, B=B)


def test_cli_round_trips_a_stored_file(tmp_path, capsys):
    from romp_amd import evaluation as E
    pp, gp, pred, gt = stored_files(tmp_path)
    for path, want in ((pp, pred), (gp, gt)):
        got = E.load_results(path)
        assert set(got) == set(want) and all(np.array_equal(got[k], np.asarray(want[k])) and got[k].dtype == np.asarray(want[k]).dtype for k in want)
    res = E.main(['--pred', pp, '--gt', gp, '--check'])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    assert res['pred']['kp2d'] == [78, 14, 2] and res['gt']['kp3d'] == [16, 14, 3] and res['gt']['valid'] == [16, 14]
    E.save_results(pp, kp2d=pred['kp2d'], kp3d=pred['kp3d'][:, :13], batch_ids=pred['batch_ids'])
    with pytest.raises(ValueError):
        E.main(['--pred', pp, '--gt', gp, '--check'])
    E.save_results(pp, kp2d=pred['kp2d'], kp3d=pred['kp3d'], batch_ids=pred['batch_ids'][::-1])
    with pytest.raises(ValueError, match='ascend'):
        E.load_results(pp)
    with pytest.raises(ValueError, match='joints'):
        E.main(['--pred', gp, '--gt', gp, '--joints', '0,1,2', '--check'])
