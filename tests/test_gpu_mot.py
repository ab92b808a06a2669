"""Tracking scores on the device (csrc/mot.hip, romp_amd/tracking_metrics.py) against the host mirror score_clip_host and the
values recorded from the reference's TrackEval (golden/mot_metrics.npz, tests/make_golden_mot.py).

Similarity: 1e-12 against a float64 numpy IoU (absolute for the IoU, which is at most 1; relative for the row and column sums).
Summary against the host mirror: counts equal, floats within 1e-12 relative -- both sides are float64 and differ only in the order
of their sums.  Summary against the recorded reference: mot_cases.reference_bound(), as in test_mot.py (mot_cases.bound_of: the
cap-sized clip 'caps' under its own bound, every other clip under the bound of the others).

Through the ABI directly (pack_layout + score_clips): rows that take part in nothing (id -1, id >= the clip's id count, an id count
that is never reached), a clip of zero frames between two others, and boxes with a NaN or +-inf coordinate, which are similar to
nothing -- as iou_host has it (test_mot.py).
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
    worst_host, worst_ref = 0., 0.
    assert sorted(got['clips']) == sorted(names)
    for n in names:
        diff = M._compare(got['clips'][n], host[n], 1e-12)
        assert diff is None, (n, diff)
        to_ref, to_host = MC.against_reference(got['clips'][n], REF[n], MC.bound_of(n)), MC.against_reference(got['clips'][n], host[n], 1e-12)
        if n == 'caps':
            print('caps: largest relative gap %.3g to the host mirror, %.3g to TrackEval (bound %.3g)' % (to_host, to_ref, MC.bound_of(n)))
        worst_ref, worst_host = max(worst_ref, to_ref), max(worst_host, to_host)
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
    assert 'caps' in BOXES and len(BOXES) == 12
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


# ------------------------------------------------------------------------------------------------ through the ABI directly
def _layout(clips, n_pred_ids=None):
    """Prepared clips -> (block, the five device-side arrays as numpy)."""
    clip_frames = np.concatenate([[0], np.cumsum([c['T'] for c in clips])])
    go = np.concatenate([[0], np.cumsum(np.concatenate([c['gt_rows'] for c in clips]))]).astype(np.int64)
    po = np.concatenate([[0], np.cumsum(np.concatenate([c['pred_rows'] for c in clips]))]).astype(np.int64)
    block = M.pack_layout(clip_frames, go, po, [c['n_gt_ids'] for c in clips], n_pred_ids or [c['n_pred_ids'] for c in clips])
    cat = lambda k, dt, tail: np.ascontiguousarray(np.concatenate([np.asarray(c[k], dt).reshape((-1,) + tail) for c in clips]), dt)  # noqa: E731
    return block, go, po, cat('gt_boxes', np.float32, (4,)), cat('gt_ids', np.int32, ()), cat('pred_ids', np.int32, ()), cat('pred_boxes', np.float32, (4,))


def _score(dev, block, gb, gi, pi, pb, metrics=True):
    up = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    r = M.score_clips(dev, block, up(gb), up(gi), up(pi), up(pb), None, metrics=metrics, **SETTINGS)
    return {k: r[k].cpu().numpy() for k in ('sim', 'rowsum', 'colsum') + (('hota', 'clear', 'identity') if metrics else ())}


def _fields(r, s, n_gt_ids):
    return {'HOTA': M._hota_fields(*(r['hota'][s][:, i] for i in range(M.HOTA_OUT))),
            'CLEAR': M._clear_fields(*r['clear'][s].tolist(), num_gt_ids=n_gt_ids), 'Identity': M._identity_fields(*r['identity'][s].tolist())}


def _prepared(name):
    return M.prepare_clip(skip_frames_without_gt=False, **ARGS[name])


def test_rows_that_take_part_in_nothing(dev, host):
    """Rows with id -1 and with id >= the id count in the middle of frames, on both sides, and an id count of the predictions that
    no id reaches: the summary is that of the clip without those rows, and their similarities are 0."""
    clip = _prepared('seed40')
    rs = np.random.RandomState(9)
    go, po = np.concatenate([[0], np.cumsum(clip['gt_rows'])]), np.concatenate([[0], np.cumsum(clip['pred_rows'])])
    G, K = clip['n_gt_ids'], clip['n_pred_ids'] + 5
    new = {k: [] for k in ('gt_boxes', 'gt_ids', 'pred_boxes', 'pred_ids')}
    rows, junk = {'gt': [], 'pred': []}, {'gt': [], 'pred': []}
    for t in range(clip['T']):
        for side, off, n_ids in (('gt', go, G), ('pred', po, K)):
            boxes, ids = clip[side + '_boxes'][off[t]:off[t + 1]], clip[side + '_ids'][off[t]:off[t + 1]]
            k = len(ids)
            extra = [(-1, k // 2), (n_ids, k // 2), (n_ids + 7, 0), (2 ** 31 - 1, k)][:2 + t % 3]     # (value, where): the middle, the ends
            mark = np.zeros(k, bool)
            for val, at in extra:
                src = boxes[rs.randint(k)] if k else np.array([10., 10., 50., 80.], np.float32)        # on top of a real box: it would count
                boxes, ids, mark = np.insert(boxes, at, src + rs.randn(4).astype(np.float32), 0), np.insert(ids, at, val), np.insert(mark, at, True)
            new[side + '_boxes'].append(boxes); new[side + '_ids'].append(ids)
            rows[side].append(len(ids)); junk[side].append(mark)
    dirty = dict(clip, gt_rows=np.asarray(rows['gt']), pred_rows=np.asarray(rows['pred']), n_pred_ids=K,
                 **{k: np.concatenate(v) for k, v in new.items()})
    assert max(rows['gt']) <= 256 and sum(m.sum() for m in junk['gt']) >= 2 * clip['T'] and int(dirty['pred_ids'].max()) == 2 ** 31 - 1
    assert not np.any((clip['pred_ids'] >= clip['n_pred_ids']))                                       # ids n_pred_ids .. K-1 own no row at all
    block, go2, po2, gb, gi, pi, pb = _layout([dirty])
    r = _score(dev, block, gb, gi, pi, pb)
    want = host['seed40']
    assert M._compare(_fields(r, 0, G), want, 1e-12) is None
    at = 0
    for t in range(clip['T']):
        n, m = rows['gt'][t], rows['pred'][t]
        sim = r['sim'][at:at + n * m].reshape(n, m)
        at += n * m
        assert np.all(sim[junk['gt'][t]] == 0) and np.all(sim[:, junk['pred'][t]] == 0), t
        clean = M.iou_host(dirty['gt_boxes'][go2[t]:go2[t + 1]][~junk['gt'][t]], dirty['pred_boxes'][po2[t]:po2[t + 1]][~junk['pred'][t]], SETTINGS['max_iou'])
        assert np.all(np.abs(sim[~junk['gt'][t]][:, ~junk['pred'][t]] - clean) <= 1e-12), t
        assert np.all(r['rowsum'][go2[t]:go2[t + 1]][junk['gt'][t]] == 0) and np.all(r['colsum'][po2[t]:po2[t + 1]][junk['pred'][t]] == 0)
    assert at == r['sim'].size


def test_a_clip_of_zero_frames_between_two_others(dev):
    a, b = _prepared('seed7'), _prepared('clear_book')
    empty = dict(a, T=0, gt_rows=np.zeros(0, np.int64), pred_rows=np.zeros(0, np.int64), n_gt_ids=0, n_pred_ids=0, gt_ids=np.zeros(0, np.int32),
                 pred_ids=np.zeros(0, np.int32), gt_boxes=np.zeros((0, 4), np.float32), pred_boxes=np.zeros((0, 4), np.float32))
    three, two = _layout([a, empty, b]), _layout([a, b])
    r3, r2 = _score(dev, three[0], *three[3:]), _score(dev, two[0], *two[3:])
    for k in ('hota', 'clear', 'identity'):
        assert r3[k].shape[0] == 3 and np.all(r3[k][1] == 0), k                                        # all zero, not merely small
        assert r3[k][0].tobytes() == r2[k][0].tobytes() and r3[k][2].tobytes() == r2[k][1].tobytes(), k
    for k in ('sim', 'rowsum', 'colsum'):
        assert r3[k].tobytes() == r2[k].tobytes(), k
    assert r2['clear'][:, 0].min() > 0 and np.isfinite(r3['hota']).all()                              # (CLR_TP of the neighbours)


BAD_BOXES = [(np.nan, 0), (np.inf, 1), (-np.inf, 2), (np.nan, 3), (np.inf, 0), (-np.inf, 1), (np.nan, 2), (np.inf, 3), (-np.inf, 0), (np.nan, 1),
             (np.inf, 2), (-np.inf, 3)]                                                                # every value in every coordinate


def test_a_non_finite_box_is_similar_to_nothing(dev):
    """A NaN or +-inf coordinate: similarity exactly 0 in that row or column, every other element byte-equal to the run without it."""
    clip = _prepared('seed40')
    block, go, po, gb, gi, pi, pb = _layout([clip])
    clean = _score(dev, block, gb, gi, pi, pb, metrics=False)
    gb2, pb2 = gb.copy(), pb.copy()
    bad_g, bad_p = np.zeros(len(gb), bool), np.zeros(len(pb), bool)
    frames = [t for t in range(clip['T']) if clip['gt_rows'][t] >= 2 and clip['pred_rows'][t] >= 2]
    for i, (v, k) in enumerate(BAD_BOXES):                                                             # one row of either side in a frame of its own
        t = frames[i]
        g, p = go[t] + i % clip['gt_rows'][t], po[t] + (i + 1) % clip['pred_rows'][t]
        gb2[g, k], pb2[p, k] = v, v
        bad_g[g], bad_p[p] = True, True
    got = _score(dev, block, gb2, gi, pi, pb2, metrics=False)
    at, hit = 0, 0
    for t in range(clip['T']):
        n, m = int(clip['gt_rows'][t]), int(clip['pred_rows'][t])
        a, b = got['sim'][at:at + n * m].reshape(n, m), clean['sim'][at:at + n * m].reshape(n, m)
        at += n * m
        rg, cp = bad_g[go[t]:go[t + 1]], bad_p[po[t]:po[t + 1]]
        hit += int((b[rg] > 0).sum() + (b[:, cp] > 0).sum())
        assert np.all(a[rg] == 0) and np.all(a[:, cp] == 0), (t, a[rg], a[:, cp])
        assert a[~rg][:, ~cp].tobytes() == b[~rg][:, ~cp].tobytes(), t
        with np.errstate(invalid='ignore'):
            want = M.iou_host(gb2[go[t]:go[t + 1]], pb2[po[t]:po[t + 1]], SETTINGS['max_iou'])
        assert np.all(np.abs(a - want) <= 1e-12) and np.all((a == 0) == (want == 0)), t           # (the host mirror says the same)
    assert hit >= len(BAD_BOXES) and np.isfinite(got['sim']).all() and np.isfinite(got['rowsum']).all() and np.isfinite(got['colsum']).all()


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
