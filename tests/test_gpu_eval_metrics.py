"""Benchmark scoring on the GPU: romp_eval_match2d / romp_eval_points / romp_eval_accumulate through the C ABI and through
romp_amd/evaluation.py, against the numpy float64 restatement of tests/test_eval_metrics.py and the reference's answers in
tests/golden/eval_metrics.npz.  Bars: matching EXACT; per-row errors relative max(the deviation the fixture measured between
the reference's float32 and float64 for that case, 2^-22 -- four float32 roundings of the output); aligned points and t
absolute max(that case's stored deviation, 2^-22 * max|coordinate|); two launches byte-identical."""
import json

import numpy as np
import pytest
import torch

from test_eval_metrics import (CAP_CASE, N_MATCH, PROCRUSTES, RANK1, golden, match2d_np, match_batch, offsets, points_np, procrustes_case,
                               stored_files, summary_np)

pytestmark = pytest.mark.gpu
F = np.float32
EPS = 2.0 ** -22
SENT_I, SENT_F, PAD = -77777, -12345.5, 5
ROMP_EINVAL = -1


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def t_(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def abi_match(dev, pred, poff, gt, valid, goff, max_pred=64, max_gt=5, thresh=0.05, norm=0, expect=0):
    """romp_eval_match2d into buffers PAD rows longer than needed, filled with a sentinel -> numpy outputs (or the status
    code when `expect` is one); asserts that the rows past the end still hold the sentinel."""
    from romp_amd import lib as L
    B, J = len(poff) - 1, pred.shape[1]
    gop = torch.full((len(pred) + PAD,), SENT_I, dtype=torch.int32, device=dev)
    pog = torch.full((len(gt) + PAD,), SENT_I, dtype=torch.int32, device=dev)
    over = torch.full((B + PAD,), SENT_I, dtype=torch.int32, device=dev)
    args = [t_(pred.astype(F), dev), t_(np.asarray(poff, np.int32), dev), t_(gt.astype(F), dev), t_(valid.astype(np.uint8), dev),
            t_(np.asarray(goff, np.int32), dev)]
    rc = L.load().romp_eval_match2d(*[L.ptr(a) for a in args], B, J, max_pred, max_gt, thresh, norm, L.ptr(gop), L.ptr(pog), L.ptr(over),
                                    L.stream_ptr(dev))
    torch.cuda.current_stream(dev).synchronize()
    if expect:
        assert rc == expect and L.load().romp_last_error()
        assert (gop == SENT_I).all() and (pog == SENT_I).all()                  # nothing was written
        return rc
    assert rc == 0, L.load().romp_last_error()
    gop, pog, over = gop.cpu().numpy(), pog.cpu().numpy(), over.cpu().numpy()
    assert (gop[len(pred):] == SENT_I).all() and (pog[len(gt):] == SENT_I).all() and (over[B:] == SENT_I).all()
    return gop[:len(pred)], pog[:len(gt)], over[:B]


def abi_points(dev, pred, target, pred_of_gt=None, align_inds=None, vis=None, mask=None, which=('mpjpe', 'mpjpe_all', 'pa_mpjpe', 'sRt', 'aligned'),
               expect=0, raw=False):
    from romp_amd import lib as L
    Np, (Ng, P) = len(pred), target.shape[:2]
    rows = {'mpjpe': 1, 'mpjpe_all': 1, 'pa_mpjpe': 1, 'sRt': 13, 'aligned': 3 * P}
    bufs = {k: torch.full(((Ng + PAD) * rows[k],), SENT_F, dtype=torch.float32, device=dev) for k in which}
    ai = None if align_inds is None else t_(np.asarray(align_inds, np.int32), dev)
    args = [t_(pred.astype(F), dev), t_(target.astype(F), dev), None if pred_of_gt is None else t_(np.asarray(pred_of_gt, np.int32), dev), ai,
            None if vis is None else t_(np.asarray(vis).astype(np.uint8), dev), None if mask is None else t_(np.asarray(mask).astype(np.uint8), dev)]
    rc = L.load().romp_eval_points(L.ptr(args[0]), Np, L.ptr(args[1]), Ng, P, L.ptr(args[2]), L.ptr(args[3]), 0 if ai is None else ai.numel(),
                                   L.ptr(args[4]), L.ptr(args[5]), *[L.ptr(bufs.get(k)) for k in ('mpjpe', 'mpjpe_all', 'pa_mpjpe', 'sRt', 'aligned')],
                                   L.stream_ptr(dev))
    torch.cuda.current_stream(dev).synchronize()
    if expect:
        assert rc == expect and L.load().romp_last_error()
        assert all((b == SENT_F).all() for b in bufs.values())
        return rc
    assert rc == 0, L.load().romp_last_error()
    out = {}
    for k, b in bufs.items():
        b = b.cpu().numpy()
        assert (b[Ng * rows[k]:] == F(SENT_F)).all(), k
        out[k] = b[:Ng * rows[k]].copy() if raw else b[:Ng * rows[k]].reshape({'sRt': (Ng, 13), 'aligned': (Ng, P, 3)}.get(k, (Ng,)))
    return out


# ------------------------------------------------------------------------------------------------ matching
@pytest.mark.parametrize('norm', ['frobenius', 'spectral'])
def test_match_every_fixture_image_in_one_launch(dev, norm):
    from romp_amd import evaluation as E
    g = golden()
    pred, pi, gt, valid, gi, B = match_batch()
    poff, goff = offsets(pi, B), offsets(gi, B)
    gop, pog, over = abi_match(dev, pred, poff, gt, valid, goff, norm=E.NORMS[norm])
    assert not over.any()
    for b in range(B):                                                          # the reference's answer, image by image
        p0, p1, g0, g1 = poff[b], poff[b + 1], goff[b], goff[b + 1]
        m = sorted((p, int(gop[p0 + p]) - g0) for p in range(p1 - p0) if gop[p0 + p] >= 0)
        assert m == sorted(map(tuple, g[f'm{b}_matches'].tolist())), b
        assert np.flatnonzero(gop[p0:p1] < 0).tolist() == g[f'm{b}_fp'].tolist(), b
        assert np.flatnonzero(pog[g0:g1] < 0).tolist() == g[f'm{b}_miss'].tolist(), b
        assert all(pog[g0 + q] == p0 + p for p, q in m)
    want = match2d_np(pred, poff, gt, valid, goff, norm=norm)
    assert np.array_equal(gop, want[0]) and np.array_equal(pog, want[1])
    again = abi_match(dev, pred, poff, gt, valid, goff, norm=E.NORMS[norm])    # deterministic
    assert all(a.tobytes() == b.tobytes() for a, b in zip((gop, pog, over), again))
    a, b = E.match_2d_greedy(t_(pred, dev), t_(pi, dev), t_(gt, dev), t_(valid, dev), t_(gi, dev), B, norm=norm)       # the Python layer; max_gt read back
    assert np.array_equal(a.cpu().numpy(), gop) and np.array_equal(b.cpu().numpy(), pog) and a.dtype == torch.int32
    a, b = E.match_2d_greedy(t_(pred, dev), t_(pi, dev), t_(gt, dev), None, t_(gi, dev), B, max_gt=5, norm=norm)       # gt_valid None: every joint
    want = match2d_np(pred, poff, gt, np.ones_like(valid), goff, norm=norm)
    assert np.array_equal(a.cpu().numpy(), want[0]) and np.array_equal(b.cpu().numpy(), want[1])


def test_match_images_alone_and_threshold(dev):
    for k in range(N_MATCH):
        pred, pi, gt, valid, gi, B = match_batch([k])
        got = abi_match(dev, pred, [0, len(pred)], gt, valid, [0, len(gt)])
        want = match2d_np(pred, [0, len(pred)], gt, valid, [0, len(gt)])
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), k
    pred, pi, gt, valid, gi, B = match_batch([3])                               # 4 x 1: a threshold no box reaches
    got = abi_match(dev, pred, [0, 4], gt, valid, [0, 1], thresh=1.5)
    assert (got[0] == -1).all() and (got[1] == -1).all()
    assert all(np.array_equal(a, b) for a, b in zip(got, match2d_np(pred, [0, 4], gt, valid, [0, 1], iou_thresh=1.5)))


def test_match_over_the_cap_is_flagged_never_truncated_and_lds_is_checked(dev):
    from romp_amd import evaluation as E
    pred, pi, gt, valid, gi, B = match_batch()
    poff, goff = offsets(pi, B), offsets(gi, B)
    full = abi_match(dev, pred, poff, gt, valid, goff)
    gop, pog, over = abi_match(dev, pred, poff, gt, valid, goff, max_pred=63)
    assert over.tolist() == [0] * CAP_CASE + [1]
    assert (gop[poff[CAP_CASE]:] == -1).all() and (pog[goff[CAP_CASE]:] == -1).all()
    assert np.array_equal(gop[:poff[CAP_CASE]], full[0][:poff[CAP_CASE]]) and np.array_equal(pog[:goff[CAP_CASE]], full[1][:goff[CAP_CASE]])
    gop, pog, over = abi_match(dev, pred, poff, gt, valid, goff, max_gt=4)
    assert over.tolist() == [0] * CAP_CASE + [1]
    assert abi_match(dev, pred, poff, gt, valid, goff, max_pred=128, max_gt=128, expect=ROMP_EINVAL) == ROMP_EINVAL   # 64 KiB of errors alone
    assert abi_match(dev, pred, poff, gt, valid, goff, max_pred=0, expect=ROMP_EINVAL) == ROMP_EINVAL
    with pytest.raises(Exception, match='LDS'):
        E.match_2d_greedy(t_(pred, dev), t_(pi, dev), t_(gt, dev), t_(valid, dev), t_(gi, dev), B, max_pred=1000, max_gt=1000)
    abi_match(dev, pred, poff, gt, valid, goff, max_pred=120, max_gt=120)       # 58 KiB: fits


# ------------------------------------------------------------------------------------------------ points
@pytest.mark.parametrize('name', PROCRUSTES)
def test_points_every_fixture_case(dev, name):
    from romp_amd import evaluation as E
    g = golden()
    pred, target, mask, keep = procrustes_case(name)
    want = points_np(pred, target, point_mask=mask)
    got = abi_points(dev, pred, target, mask=mask)
    tol_err = max(float(g[name + '_dev_err']), EPS)
    rel = np.abs(got['pa_mpjpe'] - want['pa_mpjpe']) / want['pa_mpjpe']
    coord = max(np.abs(target).max(), np.abs(want['aligned']).max())
    tol_pts = max(float(g[name + '_dev_aligned']), EPS * coord)
    d_pts = np.abs(got['aligned'] - want['aligned']).max()
    print(f'{name}: pa error rel {rel.max():.2e} (tol {tol_err:.2e}), aligned abs {d_pts:.2e} (tol {tol_pts:.2e})')
    assert rel.max() <= tol_err
    assert d_pts <= tol_pts
    assert np.abs(got['aligned'][:, keep] - g[name + '_ref_aligned']).max() <= float(g[name + '_dev_aligned']) + tol_pts     # and the reference itself
    rel = np.abs(got['mpjpe'] - want['mpjpe']) / want['mpjpe']
    assert rel.max() <= EPS and np.array_equal(got['mpjpe'], got['mpjpe_all'])
    if name not in RANK1:                                                       # R, and with it t, is unique
        tol_t = max(float(g[name + '_dev_t']), EPS * coord)
        assert np.abs(got['sRt'][:, 10:] - want['sRt'][:, 10:]).max() <= tol_t
        assert np.abs(got['sRt'][:, 1:10] - want['sRt'][:, 1:10]).max() <= max(float(g[name + '_dev_R']), EPS)
        assert (np.abs(got['sRt'][:, 0] - want['sRt'][:, 0]) / want['sRt'][:, 0]).max() <= max(float(g[name + '_dev_scale']), EPS)
    again = abi_points(dev, pred, target, mask=mask, raw=True)                  # two launches: the same bytes
    first = abi_points(dev, pred, target, mask=mask, raw=True)
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)
    # the Python layer
    p_d, t_d, m_d = t_(pred, dev), t_(target, dev), t_(mask, dev)
    e, (s, R, t) = E.pa_mpjpe(p_d, t_d, m_d, return_transform=True)
    al, (s2, R2, t2) = E.similarity_align(p_d, t_d, m_d)
    assert np.array_equal(e.cpu().numpy(), got['pa_mpjpe']) and np.array_equal(al.cpu().numpy(), got['aligned'])
    assert np.array_equal(torch.cat([s[:, None], R.reshape(-1, 9), t], 1).cpu().numpy(), got['sRt']) and torch.equal(R, R2)
    assert np.array_equal(E.pa_mpjpe(p_d, t_d, m_d).cpu().numpy(), got['pa_mpjpe'])
    assert np.array_equal(E.mpjpe(p_d, t_d).cpu().numpy(), got['mpjpe'])
    if name == 'verts':
        assert np.array_equal(E.pve(p_d, t_d).cpu().numpy(), got['mpjpe']) and np.array_equal(E.pa_pve(p_d, t_d).cpu().numpy(), got['pa_mpjpe'])
        np.testing.assert_allclose(got['mpjpe'], g['verts_ref_pve'], rtol=4e-6)


def test_points_alignment_visibility_and_two_points(dev):
    from romp_amd import evaluation as E
    g = golden()
    pred, target, vis = g['j14_pred'], g['j14_target'], g['j14_vis']
    for kw in ({'align_inds': [13]}, {'align_inds': [2, 3], 'vis': vis}, {'vis': vis}):
        want = points_np(pred, target, **kw)
        got = abi_points(dev, pred, target, **kw)
        for k in ('mpjpe', 'mpjpe_all', 'pa_mpjpe'):
            assert (np.abs(got[k] - want[k]) / want[k]).max() <= EPS, (kw, k)
    np.testing.assert_allclose(abi_points(dev, pred, target, align_inds=[13], vis=vis)['mpjpe'], g['j14_ref_mpjpe_root13_vis'], rtol=4e-6)
    got = E.mpjpe(t_(pred, dev), t_(target, dev), align_inds=[13], vis=t_(vis, dev)).cpu().numpy()
    assert np.array_equal(got, abi_points(dev, pred, target, align_inds=[13], vis=vis)['mpjpe'])
    p2, t2 = pred[:, [0, 5]], target[:, [0, 5]]                                 # P = 2: rank 1, and two points always align exactly
    want, got = points_np(p2, t2), abi_points(dev, p2, t2)
    assert np.abs(got['aligned'] - want['aligned']).max() <= EPS * np.abs(t2).max()
    assert np.abs(got['aligned'] - t2).max() <= EPS * np.abs(t2).max() and got['pa_mpjpe'].max() <= EPS * np.abs(t2).max()
    assert (np.abs(got['sRt'][:, 0] - want['sRt'][:, 0]) / want['sRt'][:, 0]).max() <= EPS
    assert abi_points(dev, pred[:, :1], target[:, :1], expect=ROMP_EINVAL) == ROMP_EINVAL        # P = 1
    with pytest.raises(Exception, match='at least 2'):
        E.pa_mpjpe(t_(pred[:, :1], dev), t_(target[:, :1], dev))
    with pytest.raises(AssertionError):
        E.pa_mpjpe(t_(pred.transpose(0, 2, 1), dev), t_(target, dev))           # (N,3,P) is not guessed at


def test_points_misses_are_nan_and_a_degenerate_row_stays_alone(dev):
    g = golden()
    pred, target = g['j14_pred'].copy(), g['j14_target']
    clean = abi_points(dev, pred, target, pred_of_gt=[0, 1, 2, 3, 4])
    pred[2] = pred[2, 0]                                                        # var1 = 0
    pog = [0, -1, 2, 3, 7]                                                      # a miss, and a row past the predictions
    got = abi_points(dev, pred, target, pred_of_gt=pog)
    for k in got:
        assert np.isnan(got[k][[1, 4]]).all(), k
    assert not np.isfinite(got['pa_mpjpe'][2]) and not np.isfinite(got['sRt'][2, 0]) and np.isfinite(got['mpjpe'][2])
    for k in got:                                                               # the neighbours: the very bytes of the clean run
        assert got[k][[0, 3]].tobytes() == clean[k][[0, 3]].tobytes(), k
    swapped = abi_points(dev, g['j14_pred'], target, pred_of_gt=[4, 3, 2, 1, 0])
    want = points_np(g['j14_pred'], target, pred_of_gt=[4, 3, 2, 1, 0])
    assert (np.abs(swapped['pa_mpjpe'] - want['pa_mpjpe']) / want['pa_mpjpe']).max() <= EPS
    only = abi_points(dev, pred, target, pred_of_gt=pog, which=('pa_mpjpe',))   # every output is optional
    assert only['pa_mpjpe'].tobytes() == got['pa_mpjpe'].tobytes()


# ------------------------------------------------------------------------------------------------ the evaluator
def dataset():
    """The matching images with the j14 people as 3-D joints (tests/test_eval_metrics.py stored_files, kept in memory)."""
    g = golden()
    pred, pi, gt, valid, gi, B = match_batch()
    rng = np.random.default_rng(5)
    p3 = g['j14_pred'][rng.integers(0, 5, len(pred))] + rng.standard_normal((len(pred), 1, 3)).astype(F) * F(0.01)
    g3 = g['j14_target'][rng.integers(0, 5, len(gt))]
    vis = rng.random(g3.shape[:2]) > 0.2
    vis[:, 0] = True
    return dict(kp2d=pred, kp3d=p3, batch_ids=pi), dict(kp2d=gt, kp3d=g3, batch_ids=gi, valid=valid, vis=vis, B=B)


def restated_summary(pred, gt, punish=150.):
    B = gt['B']
    poff, goff = offsets(pred['batch_ids'], B), offsets(gt['batch_ids'], B)
    gop, pog, _ = match2d_np(pred['kp2d'], poff, gt['kp2d'], gt['valid'], goff)
    r = points_np(pred['kp3d'], gt['kp3d'], pog, align_inds=[13], vis=gt['vis'])
    nan = np.full(len(pog), np.nan)
    rows = {'mpjpe': r['mpjpe'], 'pa_mpjpe': r['pa_mpjpe'], 'cmu_mpjpe': r['mpjpe_all'], 'pve': nan, 'pa_pve': nan}
    return summary_np(rows, pog, gop, punish), rows, gop, pog


def run_evaluator(dev, pred, gt, splits, punish=150.):
    from romp_amd import evaluation as E
    ev = E.MeshEvaluator(dev, joints=None, align_inds=[13], missing_punish_mm=punish, max_gt=5, kp2d_key='kp2d')
    for b0, b1 in splits:
        ps = np.flatnonzero((pred['batch_ids'] >= b0) & (pred['batch_ids'] < b1))
        gs = np.flatnonzero((gt['batch_ids'] >= b0) & (gt['batch_ids'] < b1))
        out = {'kp2d': t_(pred['kp2d'][ps], dev), 'joints': t_(pred['kp3d'][ps], dev)} if len(ps) else None
        ev.update(out, t_(pred['batch_ids'][ps] - b0, dev),
                  {'kp2d': t_(gt['kp2d'][gs], dev), 'kp3d': t_(gt['kp3d'][gs], dev), 'batch_ids': t_(gt['batch_ids'][gs] - b0, dev),
                   'valid': t_(gt['valid'][gs], dev), 'vis': t_(gt['vis'][gs], dev), 'B': b1 - b0})
    return ev


def test_mesh_evaluator_two_updates_equal_one_and_the_restatement(dev):
    pred, gt = dataset()
    want, rows, gop, pog = restated_summary(pred, gt, 140.)
    one = run_evaluator(dev, pred, gt, [(0, 7)], 140.)
    two = run_evaluator(dev, pred, gt, [(0, 4), (4, 7)], 140.)                  # the second call starts with the empty sides
    three = run_evaluator(dev, pred, gt, [(0, 4), (4, 5), (5, 7)], 140.)        # (4, 5): an update without predictions
    s1, s2, s3 = one.summary(), two.summary(), three.summary()
    assert want['matched'] == 10 and want['misses'] == 6 and want['false_positives'] == 68          # 2+2+1+1+0+0+4 of 16 gts / 78 preds
    assert set(s1) == set(want)
    for k, v in want.items():
        if isinstance(v, int):
            assert s1[k] == s2[k] == s3[k] == v, k
        elif np.isnan(v):
            assert np.isnan(s1[k]) and np.isnan(s2[k]), k
        else:
            assert abs(s1[k] - v) <= EPS * abs(v), (k, s1[k], v)               # float32 rows, float64 sums
            assert abs(s2[k] - s1[k]) <= 1e-12 * abs(v) and abs(s3[k] - s1[k]) <= 1e-12 * abs(v), k
    assert one.acc.dtype == torch.float64 and torch.equal(one.acc, run_evaluator(dev, pred, gt, [(0, 7)], 140.).acc)
    one.reset()
    assert not one.acc.any()
    over = run_evaluator(dev, pred, gt, [(0, 7)])
    over.max_pred = 63
    over.update({'kp2d': t_(pred['kp2d'], dev), 'joints': t_(pred['kp3d'], dev)}, t_(pred['batch_ids'], dev),
                {k: (v if k == 'B' else t_(v, dev)) for k, v in gt.items()})
    with pytest.raises(Exception, match='max_pred'):
        over.summary()


def test_cli_scores_stored_files_through_the_evaluator(dev, tmp_path, capsys):
    from romp_amd import evaluation as E
    pp, gp, pred, gt = stored_files(tmp_path)
    res = E.main(['--pred', pp, '--gt', gp, '--align_inds', '13', '--missing_punish_mm', '140', '--device', 'cuda:0'])
    no_nan = lambda d: {k: v for k, v in d.items() if v == v}
    assert no_nan(json.loads(capsys.readouterr().out.strip().splitlines()[-1])) == no_nan(res)
    want = run_evaluator(dev, *dataset(), [(0, 7)], 140.).summary()
    assert no_nan(res) == no_nan(want) and set(res) == set(want)
    assert np.isnan(res['PVE']) and res['matched'] == 10


# ------------------------------------------------------------------------------------------------ end to end
def test_forward_batch_scored_against_itself_and_against_a_moved_copy(dev):
    import romp_amd
    from oracle import romp_oracle as O
    from romp_amd import evaluation as E
    from romp_amd.post_parser import body_mesh_projection2image
    settings = romp_amd.romp_settings([])
    settings.GPU, settings.center_thresh, settings.max_batch = 0, 1.3, 2
    model = romp_amd.ROMP(settings, state_dict=O.make_romp_state_dict(0, center_bias=2.0), smpl_model=O.make_synthetic_smpl(0))
    out, bids = model.forward_batch(O.make_images(2, seed=3).to(dev))
    assert out is not None and out['verts'].shape[1:] == (6890, 3) and out['joints'].shape[1:] == (71, 3)
    N = out['joints'].shape[0]
    out['pj2d_px'] = (body_mesh_projection2image(out['joints'], out['cam'], host_pnp=False)['pj2d'] + 1) * 256
    sel = E.JOINT_SETS['h36m17_to_j14']
    ev = E.MeshEvaluator(dev, 'h36m17_to_j14', align_inds=[13], kp2d_key='pj2d_px')
    counts = torch.bincount(bids.long(), minlength=2).tolist()
    gts = {'kp2d': out['pj2d_px'][:, sel], 'kp3d': out['joints'][:, sel], 'verts': out['verts'], 'batch_ids': bids, 'B': 2}
    rows = ev.update(out, bids, gts)
    s = ev.summary()
    print(f'{N} persons ({counts} per image): {s}')
    assert torch.equal(rows['pred_of_gt'].cpu(), torch.arange(N, dtype=torch.int32))
    assert s['matched'] == s['n_gt'] == s['n_pred'] == N and s['misses'] == 0 and s['false_positives'] == 0
    assert s['precision'] == s['recall'] == s['F1'] == 1.0
    for k in ('MPJPE', 'PA_MPJPE', 'PVE', 'PA_PVE', 'CMU_MPJPE'):
        assert s[k] == 0.0, (k, s[k])                                           # exactly
    for k in E.METRICS:
        assert not rows[k].any(), k

    # the same people rotated, scaled and shifted, each by its own similarity: Procrustes undoes it, MPJPE does not
    rng = np.random.default_rng(0)
    q = rng.standard_normal((N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                  np.stack([2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)], -1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1)], 1)
    reach = float(out['verts'].norm(dim=-1).max())                               # keep every moved coordinate below 4 m (the bound below)
    sc, sh = rng.uniform(0.8, 1.2, (N, 1, 1)) * min(1.0, 3.0 / reach), rng.uniform(-0.3, 0.3, (N, 1, 3))
    move = lambda t: torch.from_numpy((sc * (t.double().cpu().numpy() @ R.transpose(0, 2, 1)) + sh).astype(F)).to(dev)
    moved = dict(gts, kp3d=move(out['joints'][:, sel]), verts=move(out['verts']))
    # the moved copy is rounded to float32 once: below 4 m that is at most 2^-23 m per coordinate, sqrt(3) * 2^-23 < 2^-22 per point
    assert float(moved['verts'].abs().max()) < 4.0
    ev.reset()
    rows = ev.update(out, bids, moved)
    s = ev.summary()
    print(f'moved copy: {s}')
    assert s['matched'] == N
    assert s['PA_MPJPE'] < EPS * 1000. and s['PA_PVE'] < EPS * 1000.            # 2^-22 * 1 m, in mm
    assert float(rows['pa_mpjpe'].max()) < EPS and float(rows['pa_pve'].max()) < EPS
    assert s['MPJPE'] > 50. and s['PVE'] > 50.
