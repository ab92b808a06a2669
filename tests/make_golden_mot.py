"""Writes tests/golden/mot_metrics.npz: hand-built and seeded clips with what the reference's TrackEval returns for them.

    PYTHONDONTWRITEBYTECODE=1 python tests/make_golden_mot.py /path/to/simple_romp/trace2/evaluation/TrackEval

Runs on the CPU (numpy + scipy).  Each clip is prepared by romp_amd.tracking_metrics (frame list, dense ids, float64 IoU of the
float32 boxes with the max_iou floor) with skip_frames_without_gt=False, so that frames without ground truth reach the metrics, and
fed to HOTA().eval_sequence, CLEAR(THRESHOLD).eval_sequence and Identity(THRESHOLD).eval_sequence.  Stored: the raw inputs
('<clip>/pred_boxes' ...) and every returned field: '<clip>/HOTA_arrays' (a float32 row of 19 per field named in 'HOTA_arrays'),
'<clip>/HOTA_scalars', '<clip>/CLEAR', '<clip>/Identity' (a float64 per field named in the array of that name).

Before anything is written the script asserts what keeps a comparison of assignments honest: in every frame of every clip, for
HOTA's and for CLEAR's score matrix, the optimum is unique among pairs of positive score -- forbidding any matched pair of positive
score and solving again gives a strictly lower optimum.  No frame is exempt; a seeded clip that fails is a reason to change its seed.
"""
import os
import sys

import numpy as np
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from romp_amd import tracking_metrics as M  # noqa: E402

THRESHOLD, MAX_IOU, ENLARGE = 0.5, 0.99, (1.1, 1.18)
HOTA_SCALARS = ('HOTA(0)', 'LocA(0)', 'HOTALocA(0)')
HOTA_ARRAYS = tuple(k for k in M.HOTA_INT + M.HOTA_FLOAT if k not in HOTA_SCALARS)      # float32 (19,) each, as TrackEval keeps them


def rows(per_frame):
    """[(frame, [(id, box)])] -> ids, frames, boxes"""
    ids, frames, boxes = [], [], []
    for fr, people in per_frame:
        for i, b in people:
            ids.append(i); frames.append(fr); boxes.append(b)
    return np.asarray(ids, np.int64), np.asarray(frames, np.int64), np.asarray(boxes, np.float32).reshape(-1, 4)


def clip(gt, pred, frames=None, kp2d=False, seed=0):
    gi, gf, gb = rows(gt)
    pi, pf, pb = rows(pred)
    c = {'gt_ids': gi, 'gt_frames': gf, 'gt_boxes': gb, 'pred_ids': pi, 'pred_frames': pf}
    if frames is not None:
        c['frames'] = np.asarray(frames, np.int64)
    if kp2d:                                              # five joints inside the box, two of them on opposite corners of its core
        rs = np.random.RandomState(seed)
        core = np.stack([pb[:, 0] + pb[:, 2] / 2 - pb[:, 2] / 2 / ENLARGE[0], pb[:, 1] + pb[:, 3] / 2 - pb[:, 3] / 2 / ENLARGE[1],
                         pb[:, 0] + pb[:, 2] / 2 + pb[:, 2] / 2 / ENLARGE[0], pb[:, 1] + pb[:, 3] / 2 + pb[:, 3] / 2 / ENLARGE[1]], 1)
        u = rs.rand(len(pb), 5, 2)
        u[:, 0], u[:, 1] = 0., 1.
        c['pred_kp2d'] = (core[:, None, :2] + u * (core[:, None, 2:] - core[:, None, :2])).astype(np.float32)
    else:
        c['pred_boxes'] = pb
    return c


def walk(seed, frames, n_gt, n_trk, miss, swap):
    """n_gt persons walking at random; the tracker sees them with jitter, misses some, swaps ids now and then, and carries
    n_trk - n_gt (or none) tracks of its own that follow nobody."""
    rs = np.random.RandomState(seed)
    pos, size = rs.rand(n_gt, 2) * 400, 40 + rs.rand(n_gt, 2) * 60
    ghost = rs.rand(max(n_trk - n_gt, 0), 2) * 400
    track = list(100 + 10 * np.arange(n_gt))
    nxt = 500
    gt, pred = [], []
    for t in range(frames):
        pos = pos + rs.randn(n_gt, 2) * 5
        here = [g for g in range(n_gt) if t == 0 or rs.rand() > 0.1]
        gt.append((t, [(3 + 7 * g, np.r_[pos[g], size[g]]) for g in here]))
        people = []
        for g in here:
            if rs.rand() < swap:
                track[g] = nxt
                nxt += 1
            if rs.rand() >= miss and (n_trk >= n_gt or g < n_trk):
                people.append((track[g], np.r_[pos[g], size[g]] + rs.randn(4) * 4))
        ghost = ghost + rs.randn(*ghost.shape) * 5
        people += [(900 + k, np.r_[ghost[k], 50, 70]) for k in range(len(ghost)) if rs.rand() > 0.3]
        pred.append((t, people))
    return gt, pred


def person(x, y=0.):
    return np.array([x, y, 40., 80.])


def near(box, dx=4.):
    return box + np.array([dx, 0., 0., 0.])


def build_clips():
    clips = {}
    A, B, Cc = person(0), person(200), person(400)
    # frames without ground truth (1), without predictions (2), with neither (3); ids seen in one frame only (900 / 55); raw ids with gaps
    clips['empty_frames'] = clip(
        gt=[(0, [(3, A), (17, B)]), (2, [(3, A), (17, B)]), (4, [(3, A), (900, Cc)]), (5, [(17, B)])],
        pred=[(0, [(7, near(A)), (8, near(B))]), (1, [(7, near(A)), (55, near(Cc))]), (4, [(7, near(A)), (8, near(Cc, 9.))]), (5, [(8, near(B))])],
        frames=range(6))
    clips['no_pred'] = clip(gt=[(0, [(3, A)]), (1, [(3, A), (17, B)])], pred=[], frames=range(2))
    clips['no_gt'] = clip(gt=[], pred=[(0, [(7, A)]), (1, [(7, A), (8, B)])], frames=range(2))
    clips['single_frame'] = clip(gt=[(0, [(3, A), (17, B), (900, Cc)])], pred=[(0, [(8, near(B)), (7, near(A, 11.))])])
    # 70 x 3 and 3 x 70: past the 64 lanes of a wave, on either side
    rs = np.random.RandomState(5)
    many = [np.r_[rs.rand(2) * 300, 30 + rs.rand(2) * 50] for _ in range(70)]
    few = [many[i] + rs.randn(4) * 3 for i in (4, 33, 68)]
    clips['wide'] = clip(gt=[(0, [(i, b) for i, b in enumerate(many)]), (1, [(i, few[k]) for k, i in enumerate((4, 33, 68))])],
                         pred=[(0, [(i, few[k]) for k, i in enumerate((4, 33, 68))]), (1, [(i, many[i] + rs.randn(4)) for i in range(70)])])
    # 65 ground-truth ids, 13 per frame
    ppl = [np.r_[(i % 13) * 100., 0., 40., 80.] for i in range(65)]
    clips['ids65'] = clip(gt=[(t, [(2 * i + 1, ppl[i]) for i in range(13 * t, 13 * t + 13)]) for t in range(5)],
                          pred=[(t, [(i % 20, ppl[i] + rs.randn(4) * 3) for i in range(13 * t, 13 * t + 13) if i % 4]) for t in range(5)])
    # IoU exactly 0.5 (counts for CLEAR, Identity and HOTA at alpha 0.5); IoU 0.0099 < 1 - max_iou (zeroed); both in every frame
    clips['edges'] = clip(gt=[(t, [(1, np.array([0., 0., 2., 2.])), (2, np.array([10., 10., 10., 10.]))]) for t in range(3)],
                          pred=[(t, [(1, np.array([0., 0., 2., 1.])), (2, np.array([10., 10., 1., 0.99]))]) for t in range(3)])
    # every similarity 0: all pairs tie at score 0
    clips['disjoint'] = clip(gt=[(t, [(1, A), (2, B)]) for t in range(3)], pred=[(t, [(1, person(1000)), (2, person(2000)), (3, person(3000))]) for t in range(3)])
    # CLEAR bookkeeping.  3: matched by 7 in frames 0-1, absent 2-4, matched by 9 in 5-6: one IDSW, no bonus, a new run.
    # 17: present 0-4, tracked 0, 1, 3, 4: ratio 4/5 (not MT), one fragmentation (frame 2 holds a far-away track 12, so that it is
    # scored: a frame without predictions is passed over and breaks no run).  900: present 5-9, tracked in 5 only: ratio 1/5 (PT).
    gt = [(t, [(3, A)] * (t < 2 or 5 <= t < 7) + [(17, B)] * (t < 5) + [(900, Cc)] * (t >= 5)) for t in range(10)]
    pred = [(t, [(7, near(A))] * (t < 2) + [(9, near(A))] * (5 <= t < 7) + [(8, near(B))] * (t < 5 and t != 2) + [(11, near(Cc))] * (t == 5) +
             [(12, person(3000))] * (t == 2)) for t in range(10)]
    clips['clear_book'] = clip(gt, pred, frames=range(10))
    # seeded: more ground truth than predictions (as boxes, and as kp2d that box to nearly the same), and the reverse
    clips['seed7'] = clip(*walk(11, 7, 5, 3, 0.1, 0.1))
    clips['seed7_kp2d'] = clip(*walk(11, 7, 5, 3, 0.1, 0.1), kp2d=True, seed=11)
    clips['seed40'] = clip(*walk(12, 40, 4, 6, 0.15, 0.05))
    # the caps: four frames of 256 x 256 rows (persons on a grid, disjoint, the predictions a few pixels off, both sides shuffled) and
    # 512 ids a side -- the even frames hold one half of them, the odd frames the other; from frame 2 on every 37th prediction
    # carries an id of the other half.  Identity's assignment is 512 x 512.
    rs = np.random.RandomState(3)
    P = 256
    base = np.stack([(np.arange(P) % 16) * 100., (np.arange(P) // 16) * 200., np.full(P, 60.), np.full(P, 150.)], 1)
    gt, pred = [], []
    for t in range(4):
        off = 0 if t % 2 == 0 else P
        gt.append((t, [(off + i, base[i]) for i in rs.permutation(P)]))
        pred.append((t, [((off + i) if not (t >= 2 and i % 37 == 0) else 2 * P - 1 - (off + i), base[i] + rs.randn(4) * 3) for i in rs.permutation(P)]))
    clips['caps'] = clip(gt, pred)
    return clips


def unique_optimum(score):
    r, c = linear_sum_assignment(-score)
    best = score[r, c].sum()
    for i, j in zip(r, c):
        if score[i, j] > 0:
            s = score.copy()
            s[i, j] = -1e9
            r2, c2 = linear_sum_assignment(-s)
            if not s[r2, c2].sum() < best:
                return False
    return True


def main(trackeval_dir):
    sys.dont_write_bytecode = True
    sys.path.insert(0, trackeval_dir)
    from trackeval.metrics import CLEAR, HOTA, Identity
    out = {'names': np.asarray(sorted(build_clips()), dtype=np.str_), 'threshold': np.float64(THRESHOLD), 'max_iou': np.float64(MAX_IOU),
           'enlarge_xy': np.asarray(ENLARGE, np.float64), 'HOTA_arrays': np.asarray(HOTA_ARRAYS, dtype=np.str_),
           'HOTA_scalars': np.asarray(HOTA_SCALARS, dtype=np.str_), 'CLEAR': np.asarray(M.CLEAR_INT + M.CLEAR_FLOAT, dtype=np.str_),
           'Identity': np.asarray(M.ID_INT + M.ID_FLOAT, dtype=np.str_)}
    for name, c in build_clips().items():
        prepared = M.prepare_clip(skip_frames_without_gt=False, **c)
        data = M.clip_data(prepared, MAX_IOU, ENLARGE)
        trace = []
        M.score_data_host(data, THRESHOLD, trace)
        for metric, t, score in trace:
            assert unique_optimum(score), 'clip %s, frame %d: the %s optimum is not unique among pairs of positive score' % (name, t, metric)
        res = {'HOTA': HOTA().eval_sequence(data), 'CLEAR': CLEAR({'THRESHOLD': THRESHOLD, 'PRINT_CONFIG': False}).eval_sequence(data),
               'Identity': Identity({'THRESHOLD': THRESHOLD, 'PRINT_CONFIG': False}).eval_sequence(data)}
        for k, v in c.items():
            out['%s/%s' % (name, k)] = v
        # every returned field, a few arrays per clip (the names of the rows are stored once, below)
        assert set(res['HOTA']) == set(M.HOTA_INT + M.HOTA_FLOAT) and set(res['CLEAR']) == set(M.CLEAR_INT + M.CLEAR_FLOAT) and \
            set(res['Identity']) == set(M.ID_INT + M.ID_FLOAT)
        out[name + '/HOTA_arrays'] = np.stack([np.asarray(res['HOTA'][k], np.float32) for k in HOTA_ARRAYS])
        out[name + '/HOTA_scalars'] = np.asarray([res['HOTA'][k] for k in HOTA_SCALARS], np.float64)
        out[name + '/CLEAR'] = np.asarray([res['CLEAR'][k] for k in M.CLEAR_INT + M.CLEAR_FLOAT], np.float64)
        out[name + '/Identity'] = np.asarray([res['Identity'][k] for k in M.ID_INT + M.ID_FLOAT], np.float64)
        print('%-13s %3d frames, %3d + %3d rows, %2d solved frames: HOTA %.4f MOTA %.4f IDSW %d Frag %d MT/PT/ML %d/%d/%d IDF1 %.4f'
              % (name, data['num_timesteps'], data['num_gt_dets'], data['num_tracker_dets'], len(trace) // 2, np.mean(res['HOTA']['HOTA']),
                 res['CLEAR']['MOTA'], res['CLEAR']['IDSW'], res['CLEAR']['Frag'], res['CLEAR']['MT'], res['CLEAR']['PT'], res['CLEAR']['ML'],
                 res['Identity']['IDF1']))
    path = os.path.join(ROOT, 'tests', 'golden', 'mot_metrics.npz')
    if os.path.exists(path):                              # a clip that is added changes nothing that is there: every stored array but the list of names
        with np.load(path) as old:
            for k in old.files:
                if k == 'names':
                    assert set(old[k].tolist()) <= set(out[k].tolist()), 'a clip of the fixture is gone'
                else:
                    assert k in out and old[k].dtype == out[k].dtype and old[k].shape == out[k].shape and \
                        old[k].tobytes() == out[k].tobytes(), 'the stored array %s would change' % k
            print('every array of the %d stored clips is reproduced bit for bit' % len(old['names']))
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
