"""Benchmark scoring on the device (include/romp_hip_eval.h, csrc/eval.hip): the reference's 2-D greedy matching
(simple_romp/evaluation/RH_evaluation/matching.py match_2d_greedy), MPJPE / PA-MPJPE / PVE / PA-PVE
(romp/lib/evaluation/evaluation_matrix.py, loss_funcs/keypoints_loss.py calc_mpjpe / calc_pampjpe) and the CMU-Panoptic
figure (simple_romp/evaluation/eval_cmu_panoptic.py:300-311), on what `forward_batch` / `forward_chunks` return, without a
host round trip: `MeshEvaluator.update` enqueues match -> points -> accumulate, `summary()` downloads one small buffer.

Conventions.  Point sets are ALWAYS (N, P, 3), persons first.  (The reference's batched Procrustes guesses the layout from
`shape[0] not in (2, 3)`, so it silently misreads a batch of exactly 2 or 3 people; nothing is guessed here.)  Rows of
predictions and of ground truth are grouped by image in ascending image order, as `forward_batch`'s `batch_ids` are.
Distances are in the unit of the inputs (metres for the SMPL outputs); `summary()` reports millimetres.

Matching error.  `norm='frobenius'` (default) is the root of the summed squares over the ground truth's valid joints.
The reference's literal `np.linalg.norm(d, 2)` on the (joints, 2) difference is the matrix 2-norm, its largest singular
value; `norm='spectral'` computes that.  The two order pairs alike unless two candidates are within a factor sqrt(2).

`python -m romp_amd.evaluation --pred P.npz --gt G.npz` scores stored results through the same calls.
"""
import argparse
import json
import sys

import numpy as np
import torch

from . import lib as L

H36M17_TO_J14 = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14]           # eval_cmu_panoptic.py:285
JOINT_SETS = {'h36m17_to_j14': [54 + j for j in H36M17_TO_J14]}           # the 17 h36m joints are rows 54: of the 71 (smpl.py:28)
NORMS = {'frobenius': 0, 'spectral': 1}
METRICS = ('mpjpe', 'pa_mpjpe', 'cmu_mpjpe', 'pve', 'pa_pve')
ACC_TAIL = 5                                                               # ROMP_EVAL_ACC_TAIL
MAX_PERSON = 64                                                            # the centre-map parser's cap on one image's detections


def _f32(t, device=None):
    t = torch.as_tensor(t, device=device)
    return t.to(torch.float32).contiguous()


def _u8(t, device):
    return None if t is None else torch.as_tensor(t, device=device).to(torch.uint8).contiguous()


def batch_offsets(batch_ids, B):
    """(N,) image index of each row, ascending -> (B+1,) int32 row offsets, on the device, no sync."""
    ids = batch_ids.to(torch.int64).contiguous()
    return torch.searchsorted(ids, torch.arange(B + 1, dtype=torch.int64, device=ids.device)).to(torch.int32)


def match_2d_greedy(pred_kp2d, pred_batch_ids, gt_kp2d, gt_valid, gt_batch_ids, B, iou_thresh=0.05, max_pred=MAX_PERSON,
                    max_gt=None, norm='frobenius', return_over_cap=False):
    """match_2d_greedy(valid=None) for the B images of a call in one launch.  pred_kp2d (Np,J,2), gt_kp2d (Ng,J,2), gt_valid
    (Ng,J) bool / uint8 (None: all valid), *_batch_ids (N,) ascending image indices: device tensors.
    -> gt_of_pred (Np,) int32 (-1: a false positive), pred_of_gt (Ng,) int32 (-1: a miss), global row numbers.
    max_pred / max_gt cap one image's counts (the pair table lives in LDS); max_gt=None reads the largest ground-truth count
    back from the device (one sync: pass it to stay asynchronous).  An image over the caps is all -1 and flagged in
    `over_cap` (B,) (return_over_cap=True), never truncated."""
    pred_kp2d, gt_kp2d = _f32(pred_kp2d), _f32(gt_kp2d, pred_kp2d.device)
    dev = pred_kp2d.device
    Np, Ng = pred_kp2d.shape[0], gt_kp2d.shape[0]
    J = gt_kp2d.shape[1] if Ng else pred_kp2d.shape[1]
    assert pred_kp2d.shape[1:] == (J, 2) or Np == 0, pred_kp2d.shape
    assert gt_kp2d.shape[1:] == (J, 2) or Ng == 0, gt_kp2d.shape
    valid = torch.ones(Ng, J, dtype=torch.uint8, device=dev) if gt_valid is None else _u8(gt_valid, dev)
    assert tuple(valid.shape) == (Ng, J), valid.shape
    poff = batch_offsets(torch.as_tensor(pred_batch_ids, device=dev), B)
    goff = batch_offsets(torch.as_tensor(gt_batch_ids, device=dev), B)
    if max_gt is None:
        max_gt = max(int((goff[1:] - goff[:-1]).max()), 1)
    gt_of_pred = torch.full((Np,), -1, dtype=torch.int32, device=dev)          # (rows of an image index >= B stay -1)
    pred_of_gt = torch.full((Ng,), -1, dtype=torch.int32, device=dev)
    over = torch.zeros(B, dtype=torch.int32, device=dev)
    L.check(L.load().romp_eval_match2d(L.ptr(pred_kp2d), L.ptr(poff), L.ptr(gt_kp2d), L.ptr(valid), L.ptr(goff), B, J,
                                       int(max_pred), int(max_gt), float(iou_thresh), NORMS[norm], L.ptr(gt_of_pred),
                                       L.ptr(pred_of_gt), L.ptr(over), L.stream_ptr(dev)))
    return (gt_of_pred, pred_of_gt, over) if return_over_cap else (gt_of_pred, pred_of_gt)


def eval_points(pred, target, pred_of_gt=None, align_inds=None, vis=None, point_mask=None,
                want=('mpjpe', 'mpjpe_all', 'pa_mpjpe', 'sRt', 'aligned'), out=None):
    """romp_eval_points: pred (Np,P,3), target (Ng,P,3) device tensors; row g of the target is scored against row
    pred_of_gt[g] of pred (None: row g).  -> dict of the outputs named in `want` ((Ng,), sRt (Ng,13), aligned (Ng,P,3));
    `out` supplies preallocated (Ng,) float32 rows for some of them."""
    pred, target = _f32(pred), _f32(target)
    dev = target.device
    assert pred.dim() == 3 and target.dim() == 3 and pred.shape[2] == 3 and target.shape[1:] == pred.shape[1:], \
        'point sets are (N, P, 3): %s vs %s' % (tuple(pred.shape), tuple(target.shape))
    Np, Ng, P = pred.shape[0], target.shape[0], target.shape[1]
    if pred_of_gt is None:
        assert Np == Ng, 'unmatched inputs need one prediction per target row'
    else:
        pred_of_gt = pred_of_gt.to(torch.int32).contiguous()
        assert tuple(pred_of_gt.shape) == (Ng,)
    ai = None if align_inds is None else torch.as_tensor(align_inds, device=dev).to(torch.int32).reshape(-1).contiguous()
    vis, point_mask = _u8(vis, dev), _u8(point_mask, dev)
    assert vis is None or tuple(vis.shape) == (Ng, P), vis.shape
    assert point_mask is None or tuple(point_mask.shape) == (P,), point_mask.shape
    shapes = {'mpjpe': (Ng,), 'mpjpe_all': (Ng,), 'pa_mpjpe': (Ng,), 'sRt': (Ng, 13), 'aligned': (Ng, P, 3)}
    res = dict(out or {})
    for k in want:
        if k not in res:
            res[k] = torch.empty(shapes[k], dtype=torch.float32, device=dev)
    L.check(L.load().romp_eval_points(L.ptr(pred), Np, L.ptr(target), Ng, P, L.ptr(pred_of_gt), L.ptr(ai),
                                      0 if ai is None else ai.numel(), L.ptr(vis), L.ptr(point_mask),
                                      *[L.ptr(res.get(k)) for k in ('mpjpe', 'mpjpe_all', 'pa_mpjpe', 'sRt', 'aligned')],
                                      L.stream_ptr(dev)))
    return res


def mpjpe(pred, target, align_inds=None, vis=None):
    """compute_mpjpe(sample_wise=True) after align_by_parts(align_inds): (N,P,3) x 2 -> (N,); vis (N,P): sum(err*vis)/sum(vis)."""
    return eval_points(pred, target, align_inds=align_inds, vis=vis, want=('mpjpe',))['mpjpe']


def pa_mpjpe(pred, target, point_mask=None, return_transform=False):
    """calc_pampjpe: the similarity transform fitted on the points of the batch-common point_mask (P,), then the mean distance
    over them.  -> (N,), with return_transform also (scale (N,), R (N,3,3), t (N,3)) of  aligned = scale * R x + t."""
    r = eval_points(pred, target, point_mask=point_mask, want=('pa_mpjpe', 'sRt') if return_transform else ('pa_mpjpe',))
    if not return_transform:
        return r['pa_mpjpe']
    s = r['sRt']
    return r['pa_mpjpe'], (s[:, 0], s[:, 1:10].reshape(-1, 3, 3), s[:, 10:13])


def similarity_align(pred, target, point_mask=None):
    """batch_compute_similarity_transform_torch on (N,P,3): -> (aligned (N,P,3), (scale, R, t)).  The transform is fitted on
    the masked points and applied to all P."""
    r = eval_points(pred, target, point_mask=point_mask, want=('sRt', 'aligned'))
    s = r['sRt']
    return r['aligned'], (s[:, 0], s[:, 1:10].reshape(-1, 3, 3), s[:, 10:13])


def pve(pred_verts, target_verts):
    """compute_error_verts: mean distance over the vertices, (N,6890,3) x 2 -> (N,)."""
    return mpjpe(pred_verts, target_verts)


def pa_pve(pred_verts, target_verts):
    return pa_mpjpe(pred_verts, target_verts)


def _accel(joints, gt, links, vis, joint_inds):
    import ctypes as C
    joints = _f32(joints)
    dev = joints.device
    assert joints.dim() == 3 and joints.shape[2] == 3, 'joints are (N, J, 3): %s' % (tuple(joints.shape),)
    N, J = joints.shape[:2]
    gt = None if gt is None else _f32(gt, dev)
    assert gt is None or gt.shape == joints.shape, 'gt %s against joints %s' % (tuple(gt.shape), tuple(joints.shape))
    vis = _u8(vis, dev)
    assert vis is None or tuple(vis.shape) == (N,), vis.shape
    prev, nxt = (torch.as_tensor(t, device=dev).to(torch.int32).contiguous() for t in links)
    assert tuple(prev.shape) == (N,) and tuple(nxt.shape) == (N,), 'links: one entry per row'
    idx = None if joint_inds is None else [int(i) for i in (joint_inds.tolist() if hasattr(joint_inds, 'tolist') else joint_inds)]
    K = J if idx is None else len(idx)
    value = torch.empty(N, dtype=torch.float32, device=dev)
    valid = torch.empty(N, dtype=torch.uint8, device=dev)
    if dev.type != 'cuda':
        raise L.RompHipError('the acceleration metric runs on the HIP device only (no CPU fallback); move the tensors to "cuda:N"')
    with torch.cuda.device(dev):
        L.check(L.load().romp_clip_accel(L.ptr(joints), N, J, L.ptr(gt), L.ptr(vis), K, None if idx is None else (C.c_int32 * K)(*idx),
                                         L.ptr(prev), L.ptr(nxt), L.ptr(value), L.ptr(valid), L.stream_ptr(dev)))
    return value, valid


def accel(joints, links, joint_inds=None):
    """compute_accel (evaluation_matrix.py:424-435) along the links of a clip (``romp_amd.clip.clip_links``): joints (N,J,3),
    links = (prev, next) -> (values (N,), valid (N,) uint8) on the device.  values[n] = the mean over the (picked) joints of
    |J[prev n] - 2 J[n] + J[next n]| at a row with both links; 0 and valid 0 elsewhere.  In the units of the joints."""
    return _accel(joints, None, links, None, joint_inds)


def accel_error(pred, gt, links, vis=None, joint_inds=None):
    """compute_error_accel (evaluation_matrix.py:437-465): the mean over the joints of the distance between the predicted and
    the true acceleration.  vis (N,): a row counts when it and both its neighbours are visible, the rows the reference's
    np.roll mask keeps.  -> (values (N,), valid (N,) uint8) on the device."""
    return _accel(pred, gt, links, vis, joint_inds)


def mean_accel(joints, links, gt=None, vis=None, joint_inds=None):
    """The mean of ``accel`` (or, with gt, of ``accel_error``) over the valid rows: a 0-d device tensor, NaN without a valid row."""
    value, valid = _accel(joints, gt, links, vis, joint_inds)
    return value.sum() / valid.sum()                             # invalid rows hold 0


class MeshEvaluator:
    """A running score over a dataset, kept on the device.

    joints: 'h36m17_to_j14' (rows 54 + [0..12, 14] of forward_batch's 71 joints), an index list, or None (the predictions
    are already in the ground truth's joint order).  align_inds: joints (in the SELECTED order) whose mean is subtracted from
    each side before MPJPE; [13] is eval_cmu_panoptic.py's root.  max_pred / max_gt: caps on one image's people."""

    def __init__(self, device, joints='h36m17_to_j14', align_inds=None, missing_punish_mm=150., iou_thresh=0.05,
                 max_pred=MAX_PERSON, max_gt=MAX_PERSON, norm='frobenius', kp2d_key='pj2d_org'):
        self.device = torch.device(device)
        L.load()
        idx = JOINT_SETS[joints] if isinstance(joints, str) else joints
        self.joint_index = None if idx is None else torch.as_tensor(list(idx), dtype=torch.int64, device=self.device)
        self.align_inds = None if align_inds is None else torch.as_tensor(list(align_inds), dtype=torch.int32, device=self.device)
        self.missing_punish_mm, self.iou_thresh, self.norm, self.kp2d_key = float(missing_punish_mm), float(iou_thresh), norm, kp2d_key
        self.max_pred, self.max_gt = int(max_pred), int(max_gt)
        self.acc = torch.zeros(2 * len(METRICS) + ACC_TAIL, dtype=torch.float64, device=self.device)

    def reset(self):
        self.acc.zero_()

    def _select(self, t):
        return t if self.joint_index is None else t.index_select(1, self.joint_index)

    def update(self, outputs, batch_ids, gts):
        """outputs: what forward_batch returns ('joints' (N,71,3), 'verts' (N,6890,3)) plus the caller's 2-D projections under
        `kp2d_key` ((N,71,2), in the ground truth's pixel frame); None when nobody was detected.  batch_ids (N,).
        gts: 'kp2d' (Ng,J,2), 'kp3d' (Ng,J,3), 'batch_ids' (Ng,), 'B' images of the call; optional 'valid' (Ng,J) (matching),
        'vis' (Ng,J) (MPJPE weights), 'point_mask' (J,) (Procrustes), 'verts' (Ng,6890,3) (PVE / PA-PVE).
        Enqueues match -> points -> accumulate on the current stream; returns the per-row tensors of this call."""
        dev = self.device
        g2d, g3d = _f32(gts['kp2d'], dev), _f32(gts['kp3d'], dev)
        Ng, J = g3d.shape[:2]
        B = int(gts['B'])
        if outputs is None:
            p2d, p3d = torch.zeros(0, J, 2, device=dev), torch.zeros(0, J, 3, device=dev)
            batch_ids = torch.zeros(0, dtype=torch.int64, device=dev)
        else:
            p2d, p3d = self._select(_f32(outputs[self.kp2d_key], dev)), self._select(_f32(outputs['joints'], dev))
        gt_of_pred, pred_of_gt, over = match_2d_greedy(p2d, batch_ids, g2d, gts.get('valid'), gts['batch_ids'], B, self.iou_thresh,
                                                       self.max_pred, self.max_gt, self.norm, return_over_cap=True)
        metrics = torch.full((len(METRICS), Ng), float('nan'), dtype=torch.float32, device=dev)
        rows = dict(zip(METRICS, metrics))
        eval_points(p3d, g3d, pred_of_gt, self.align_inds, gts.get('vis'), gts.get('point_mask'), want=(),
                    out={'mpjpe': rows['mpjpe'], 'mpjpe_all': rows['cmu_mpjpe'], 'pa_mpjpe': rows['pa_mpjpe']})
        if gts.get('verts') is not None:
            pv = _f32(outputs['verts'], dev) if outputs is not None else torch.zeros(0, gts['verts'].shape[1], 3, device=dev)
            eval_points(pv, _f32(gts['verts'], dev), pred_of_gt, want=(), out={'mpjpe': rows['pve'], 'pa_mpjpe': rows['pa_pve']})
        L.check(L.load().romp_eval_accumulate(L.ptr(metrics), len(METRICS), Ng, L.ptr(pred_of_gt), L.ptr(gt_of_pred),
                                              gt_of_pred.numel(), L.ptr(over), B, L.ptr(self.acc), L.stream_ptr(dev)))
        return dict(rows, gt_of_pred=gt_of_pred, pred_of_gt=pred_of_gt)

    def summary(self):
        """One download.  Millimetres over the matched pairs; CMU_MPJPE: eval_cmu_panoptic.py's mean of the matched persons'
        sum(err*vis)/J and `missing_punish_mm` per miss; precision / recall / F1 from the miss and false-positive counts."""
        return summarize(self.acc.cpu().numpy(), self.missing_punish_mm)


def summarize(acc, missing_punish_mm=150.):
    """The fields of MeshEvaluator.summary() from an accumulator (2*len(METRICS) + 5 float64)."""
    acc = np.asarray(acc, np.float64)
    tail = acc[2 * len(METRICS):]
    misses, false_pos, n_gt, n_pred, over = (float(x) for x in tail)
    if over:
        raise L.RompHipError('%d image(s) held more people than the evaluator\'s max_pred / max_gt: raise the caps' % over)
    mean = lambda k: float(acc[2 * k] / acc[2 * k + 1] * 1000.) if acc[2 * k + 1] else float('nan')
    res = {'MPJPE': mean(0), 'PA_MPJPE': mean(1), 'PVE': mean(3), 'PA_PVE': mean(4)}
    cmu_n = acc[5] + misses
    res['CMU_MPJPE'] = float((acc[4] * 1000. + misses * missing_punish_mm) / cmu_n) if cmu_n else float('nan')
    matched = n_gt - misses
    res['precision'] = matched / (matched + false_pos) if matched + false_pos else float('nan')
    res['recall'] = matched / n_gt if n_gt else float('nan')
    pr = res['precision'] + res['recall']
    res['F1'] = 2 * res['precision'] * res['recall'] / pr if pr and pr == pr else float('nan')
    res.update(matched=int(matched), misses=int(misses), false_positives=int(false_pos), n_gt=int(n_gt), n_pred=int(n_pred))
    return res


# ---------------------------------------------------------------------------------------------------- stored results
PRED_KEYS, GT_KEYS = ('kp2d', 'kp3d', 'batch_ids'), ('kp2d', 'kp3d', 'batch_ids')


def save_results(path, **arrays):
    """A prediction or ground-truth file of the CLI: kp2d (N,J,2), kp3d (N,J,3), batch_ids (N,), optionally verts (N,V,3) and,
    for ground truth, valid (N,J), vis (N,J), point_mask (J,), B."""
    np.savez(path, **{k: np.asarray(v) for k, v in arrays.items() if v is not None})


def load_results(path, required=PRED_KEYS):
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    for k in required:
        if k not in d:
            raise ValueError('%s: no array %r' % (path, k))
    n = len(d['batch_ids'])
    if d['kp2d'].shape[:1] != (n,) or d['kp2d'].shape[2:] != (2,) or d['kp3d'].shape != d['kp2d'].shape[:2] + (3,):
        raise ValueError('%s: kp2d %s / kp3d %s / batch_ids %s do not belong together' % (path, d['kp2d'].shape, d['kp3d'].shape, d['batch_ids'].shape))
    if n and np.any(np.diff(d['batch_ids']) < 0):
        raise ValueError('%s: batch_ids must ascend' % path)
    return d


def score_files(pred, gt, device='cuda:0', joints=None, align_inds=None, missing_punish_mm=150., iou_thresh=0.05, norm='frobenius',
                images_per_call=32):
    """Score loaded files (load_results) `images_per_call` images at a time through MeshEvaluator -> summary dict."""
    B = int(gt['B']) if 'B' in gt else int(max(gt['batch_ids'].max(initial=-1), pred['batch_ids'].max(initial=-1))) + 1
    cap = lambda ids: max(int(np.bincount(ids.astype(np.int64)).max(initial=1)), 1)
    ev = MeshEvaluator(device, joints, align_inds, missing_punish_mm, iou_thresh, cap(pred['batch_ids']), cap(gt['batch_ids']), norm,
                       kp2d_key='kp2d')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ev.device)
    for b0 in range(0, B, images_per_call):
        b1 = min(b0 + images_per_call, B)
        ps, gs = [np.flatnonzero((d['batch_ids'] >= b0) & (d['batch_ids'] < b1)) for d in (pred, gt)]
        out = None
        if len(ps):
            out = {'kp2d': t(pred['kp2d'][ps]), 'joints': t(pred['kp3d'][ps])}
            if 'verts' in pred:
                out['verts'] = t(pred['verts'][ps])
        g = {'kp2d': t(gt['kp2d'][gs]), 'kp3d': t(gt['kp3d'][gs]), 'batch_ids': t(gt['batch_ids'][gs] - b0), 'B': b1 - b0}
        for k in ('valid', 'vis', 'verts'):
            if k in gt and (k != 'verts' or 'verts' in pred):
                g[k] = t(gt[k][gs])
        if 'point_mask' in gt:
            g['point_mask'] = t(gt['point_mask'])
        ev.update(out, t(pred['batch_ids'][ps] - b0), g)
    return ev.summary()


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m romp_amd.evaluation', description='Score stored predictions against stored ground truth on the device.')
    ap.add_argument('--pred', required=True, help='npz: kp2d (N,J,2), kp3d (N,J,3), batch_ids (N,), optional verts')
    ap.add_argument('--gt', required=True, help='npz: kp2d, kp3d, batch_ids, optional valid, vis, point_mask, verts, B')
    ap.add_argument('--joints', default=None, help="'h36m17_to_j14' or a comma list of rows of the predictions; default: as stored")
    ap.add_argument('--align_inds', default=None, help='comma list of joints whose mean is subtracted before MPJPE (CMU-Panoptic: 13)')
    ap.add_argument('--missing_punish_mm', type=float, default=150.)
    ap.add_argument('--iou_thresh', type=float, default=0.05)
    ap.add_argument('--norm', choices=sorted(NORMS), default='frobenius')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--check', action='store_true', help='load and validate the two files, print their shapes, score nothing')
    a = ap.parse_args(argv)
    ints = lambda s: None if s is None else [int(x) for x in s.split(',') if x != '']
    joints = a.joints if a.joints in JOINT_SETS else ints(a.joints)
    pred, gt = load_results(a.pred, PRED_KEYS), load_results(a.gt, GT_KEYS)
    n_sel = pred['kp3d'].shape[1] if joints is None else len(JOINT_SETS.get(joints, joints) if isinstance(joints, str) else joints)
    if n_sel != gt['kp3d'].shape[1]:
        raise ValueError('predictions give %d joints, ground truth %d' % (n_sel, gt['kp3d'].shape[1]))
    if a.check:
        res = {'pred': {k: list(v.shape) for k, v in sorted(pred.items())}, 'gt': {k: list(v.shape) for k, v in sorted(gt.items())}}
    else:
        res = score_files(pred, gt, a.device, joints, ints(a.align_inds), a.missing_punish_mm, a.iou_thresh, a.norm)
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main(sys.argv[1:])
