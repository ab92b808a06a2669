"""Tracking scores on the device (csrc/mot.hip, romp_amd/tracking_metrics.py) against the host mirror score_clip_host and the
values recorded from the reference's TrackEval (golden/mot_metrics.npz, tests/make_golden_mot.py).

Similarity: 1e-12 against a float64 numpy IoU (absolute for the IoU, which is at most 1; relative for the row and column sums).
Summary against the host mirror: counts equal, floats within 1e-12 relative -- both sides are float64 and differ only in the order
of their sums.  Summary against the recorded reference: mot_cases.reference_bound(), as in test_mot.py.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mot_cases as MC  # noqa: E402

from romp_amd import tracking_metrics as M  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES, ARGS, REF, SETTINGS = MC.load()
BOXES = [n for n in NAMES if 'pred_boxes' in ARGS[n]]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def host():
    return {n: M.score_clip_host(skip_frames_without_gt=False, **SETTINGS, **ARGS[n]) for n in NAMES}


def _evaluator(dev, names):
    ev = M.TrackingEvaluator(dev, skip_frames_without_gt=False, **SETTINGS)
    for n in names:
        ev.add_clip(n, **ARGS[n])
    return ev


def _check(got, names, host):
    bound, worst_host, worst_ref = MC.reference_bound(), 0., 0.
    assert sorted(got['clips']) == sorted(names)
    for n in names:
        diff = M._compare(got['clips'][n], host[n], 1e-12)
        assert diff is None, (n, diff)
        worst_ref = max(worst_ref, MC.against_reference(got['clips'][n], REF[n], bound))
        worst_host = max(worst_host, MC.against_reference(got['clips'][n], host[n], 1e-12))
    ref, comb = M.combine_clips({n: host[n] for n in names})
    assert M._compare(got['combined'], comb, 1e-12) is None
    for k in ref:
        assert abs(got['reference'][k] - ref[k]) <= 1e-12 * abs(ref[k])
    return worst_host, worst_ref


@pytest.mark.parametrize('name', NAMES)
def test_similarity(dev, name):
    a = ARGS[name]
    clip = M.prepare_clip(skip_frames_without_gt=False, **a)
    data = M.clip_data(clip, SETTINGS['max_iou'], SETTINGS['enlarge_xy'])
    go, po = np.concatenate([[0], np.cumsum(clip['gt_rows'])]), np.concatenate([[0], np.cumsum(clip['pred_rows'])])
    block = M.pack_layout([0, clip['T']], go, po, [clip['n_gt_ids']], [clip['n_pred_ids']])
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    r = M.score_clips(dev, block, up(clip['gt_boxes']), up(clip['gt_ids']), up(clip['pred_ids']), up(clip['pred_boxes']), up(clip['pred_kp2d']),
                      metrics=False, **SETTINGS)
    sim, rowsum, colsum = r['sim'].cpu().numpy(), r['rowsum'].cpu().numpy(), r['colsum'].cpu().numpy()
    at, worst = 0, 0.
    for t, want in enumerate(data['similarity_scores']):
        got = sim[at:at + want.size].reshape(want.shape)
        at += want.size
        worst = max(worst, float(np.abs(got - want).max(initial=0.)))
        assert np.all(np.abs(got - want) <= 1e-12), t
        assert np.all((got == 0) == (want == 0)), t           # the max_iou floor and the empty intersections fall the same way
        assert np.all(np.abs(rowsum[go[t]:go[t + 1]] - want.sum(1)) <= 1e-12 * np.maximum(want.sum(1), 1e-300))
        assert np.all(np.abs(colsum[po[t]:po[t + 1]] - want.sum(0)) <= 1e-12 * np.maximum(want.sum(0), 1e-300))
    assert at == sim.size
    print('%s: similarity max abs gap %.3g' % (name, worst))


def test_box_iou_and_boxes_from_kp2d(dev):
    a, e = ARGS['seed7_kp2d'], ARGS['edges']
    kp = torch.from_numpy(a['pred_kp2d']).to(dev)
    boxes = M.boxes_from_kp2d(kp, SETTINGS['enlarge_xy']).cpu().numpy()
    want = M.boxes_from_kp2d_host(a['pred_kp2d'], SETTINGS['enlarge_xy'])
    assert boxes.dtype == np.float64 and np.all(np.abs(boxes - want) <= 1e-12 * np.abs(want))
    gt = torch.from_numpy(a['gt_boxes'][:5]).to(dev)
    got = M.box_iou(gt, pred_kp2d=kp[:3], **{k: SETTINGS[k] for k in ('max_iou', 'enlarge_xy')}).cpu().numpy()
    assert got.shape == (5, 3) and np.all(np.abs(got - M.iou_host(a['gt_boxes'][:5], want[:3])) <= 1e-12)
    edge = M.box_iou(torch.from_numpy(e['gt_boxes'][:2]).to(dev), torch.from_numpy(e['pred_boxes'][:2]).to(dev)).cpu().numpy()
    assert edge[0, 0] == 0.5 and edge[1, 1] == 0. and edge[0, 1] == 0.
    unfloored = M.box_iou(torch.from_numpy(e['gt_boxes'][:2]).to(dev), torch.from_numpy(e['pred_boxes'][:2]).to(dev), max_iou=1.).cpu().numpy()
    assert 0.0098 < unfloored[1, 1] < 0.01
    degenerate = M.box_iou(torch.zeros(1, 4, device=dev), torch.zeros(1, 4, device=dev)).cpu().numpy()
    assert degenerate[0, 0] == 0.                                # a union of 0


def test_all_box_clips_in_one_call(dev, host):
    ev = _evaluator(dev, BOXES)
    got = ev.summary()
    worst_host, worst_ref = _check(got, BOXES, host)
    print('summary() of %d clips: %d launches, %d bytes downloaded; largest relative gap %.3g to the host mirror, %.3g to TrackEval (bound %.3g)'
          % (len(BOXES), ev.last_launches, ev.last_download_bytes, worst_host, worst_ref, MC.reference_bound()))
    assert ev.last_launches == 9 and ev.last_download_bytes == 8 * len(BOXES) * (19 * 7 + 12 + 3 + 1)


@pytest.mark.parametrize('name', NAMES)
def test_one_clip_per_call(dev, host, name):
    _check(_evaluator(dev, [name]).summary(), [name], host)


def test_three_clips_of_1_7_and_40_frames(dev, host):
    names = ['single_frame', 'seed7', 'seed40']
    assert [len(np.unique(np.concatenate([ARGS[n]['gt_frames'], ARGS[n]['pred_frames']]))) for n in names] == [1, 7, 40]
    _check(_evaluator(dev, names).summary(), names, host)
    names = ['seed7_kp2d', 'no_pred']                           # kp2d predictions next to a clip without any
    _check(_evaluator(dev, names).summary(), names, host)


def test_skipping_frames_without_ground_truth(dev):
    ev = M.TrackingEvaluator(dev, **SETTINGS)
    ev.add_clip('empty_frames', **ARGS['empty_frames'])
    want = M.score_clip_host(**SETTINGS, **ARGS['empty_frames'])
    assert M._compare(ev.summary()['clips']['empty_frames'], want, 1e-12) is None and want['CLEAR']['CLR_Frames'] == 4


def test_equal_inputs_give_equal_bits(dev):
    a, b = _evaluator(dev, BOXES), _evaluator(dev, BOXES)
    a.summary()
    torch.empty(1 << 20, device=dev).normal_()                  # other work in between: the allocator hands out other addresses
    b.summary()
    assert a.last_raw.tobytes() == b.last_raw.tobytes() and np.all(np.isfinite(a.last_raw))


def test_add_tracked_equals_add_clip_on_the_downloaded_ids(dev):
    from romp_amd.tracking import DeviceTracker
    T, P, J = 12, 3, 6
    rs = np.random.RandomState(3)
    pos = np.array([[100., 200.], [300., 220.], [520., 180.]])
    pts, kps, gt_box, gt_id, gt_fr, frame_rows = [], [], [], [], [], []
    for t in range(T):
        pos = pos + rs.randn(P, 2) * 3
        seen = [p for p in range(P) if not (p == 1 and 4 <= t < 7)]         # the second person goes undetected for three frames
        for p in seen:
            pts.append([pos[p, 0], pos[p, 1], 50. + 10 * p, 40.])
            u = rs.rand(J, 2)
            u[0], u[1] = 0., 1.                                              # (two joints on opposite corners: the enlarged box is close to the true one)
            kps.append(pos[p] + (u - 0.5) * [54., 127.])
        frame_rows.append(len(seen))
        if t != 9:                                                           # a frame without ground truth
            for p in range(P):
                gt_box.append([pos[p, 0] - 30, pos[p, 1] - 75, 60., 150.]); gt_id.append(10 * p + 4); gt_fr.append(t)
    points, kp2d = torch.tensor(np.asarray(pts), dtype=torch.float32, device=dev), torch.tensor(np.asarray(kps), dtype=torch.float32, device=dev)
    scores = torch.full((len(pts),), 0.5, device=dev)
    trk = DeviceTracker(dev, capacity=16)
    count, ids, rows, _ = trk.update_frames(points, scores, frame_rows)
    for skip in (True, False):
        ev = M.TrackingEvaluator(dev, skip_frames_without_gt=skip, **SETTINGS)
        ev.add_tracked('clip', count, ids, rows, kp2d, gt_box, gt_id, gt_fr)
        got = ev.summary()['clips']['clip']
        n, ids_h, rows_h = count.cpu().numpy(), ids.cpu().numpy(), rows.cpu().numpy()
        p_ids = np.concatenate([ids_h[t, :n[t]] for t in range(T)])
        p_rows = np.concatenate([rows_h[t, :n[t]] for t in range(T)])
        p_frames = np.concatenate([np.full(n[t], t) for t in range(T)])
        ev2 = M.TrackingEvaluator(dev, skip_frames_without_gt=skip, **SETTINGS)
        ev2.add_clip('clip', p_ids, p_frames, gt_box, gt_id, gt_fr, pred_kp2d=kp2d.cpu().numpy()[p_rows])
        want = ev2.summary()['clips']['clip']
        assert M._compare(got, want, 1e-12) is None
        assert M._compare(got, M.score_clip_host(p_ids, p_frames, gt_box, gt_id, gt_fr, pred_kp2d=kp2d.cpu().numpy()[p_rows],
                                                 skip_frames_without_gt=skip, **SETTINGS), 1e-12) is None
        assert got['CLEAR']['CLR_TP'] >= 25 and got['CLEAR']['CLR_Frames'] == (11 if skip else 12) and len(set(p_ids.tolist())) >= 3
    with pytest.raises(ValueError, match='capacity'):
        M.TrackingEvaluator(dev).add_tracked('big', torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, 257, dtype=torch.int32, device=dev),
                                             torch.zeros(1, 257, dtype=torch.int32, device=dev), kp2d, gt_box, gt_id, gt_fr)


def test_caps_and_null_pointers_are_refused(dev):
    from romp_amd import lib
    h = lib.load()
    for bad in (([0, 1], [0, 257], [0, 1], [1], [1]), ([0, 1], [0, 1], [0, 257], [1], [1]), ([0, 1], [0, 1], [0, 1], [513], [1]),
                ([0, 1], [0, 1], [0, 1], [1], [513])):
        with pytest.raises(lib.RompHipError):
            M.pack_layout(*bad)
    block = M.pack_layout([0, 1], [0, 2], [0, 2], [2], [2])
    bp = block.ctypes.data_as(C.POINTER(C.c_int64))
    buf = torch.zeros(4096, dtype=torch.float64, device=dev)
    p, st = lib.ptr(buf), lib.stream_ptr(dev)
    before = buf.clone()
    assert h.romp_mot_tables(bp, p, p, None, p, st) == -1 and h.romp_mot_tables(None, p, p, p, p, st) == -1
    assert h.romp_mot_similarity(bp, p, None, p, p, None, 0, 1., 1., p, 0.99, p, p, p, st) == -1
    assert h.romp_mot_similarity(bp, p, p, p, p, p, 5, 1., 1., p, 0.99, p, p, p, st) == -1
    alphas = (C.c_double * 19)(*M.ALPHAS.tolist())
    assert h.romp_mot_hota(bp, p, p, p, p, p, p, alphas, p, None, st) == -1 and h.romp_mot_hota(bp, None, p, p, p, p, p, alphas, p, p, st) == -1
    assert h.romp_mot_clear(bp, p, p, p, None, 0.5, p, p, st) == -1 and h.romp_mot_clear(bp, p, p, p, p, 1.5, p, p, st) == -1
    assert h.romp_mot_identity(bp, p, p, None, p, 0.5, p, p, st) == -1 and h.romp_mot_identity(bp, p, p, p, p, 0.5, None, p, st) == -1
    assert h.romp_mot_boxes(p, 0, 5, 1.1, 1.18, p, st) == -1
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                              # nothing was launched on the buffer every pointer named
    with pytest.raises(ValueError, match='one of them'):
        M.score_clips(dev, block, buf[:8].float().view(2, 4), torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))


def test_the_moved_solver_still_serves_romp_track_assign(dev):
    from scipy.optimize import linear_sum_assignment
    from romp_amd import lib
    h = lib.load()
    cost = np.random.RandomState(7).rand(5, 7)
    d_cost, d_pair = torch.from_numpy(cost).to(dev), torch.empty(5, dtype=torch.int32, device=dev)
    lib.check(h.romp_track_assign(lib.ptr(d_cost), 5, 7, 10., lib.ptr(d_pair), lib.stream_ptr(dev)))
    r, c = linear_sum_assignment(cost)
    assert r.tolist() == [0, 1, 2, 3, 4] and d_pair.cpu().numpy().tolist() == c.tolist()
