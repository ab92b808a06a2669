"""The Relative Human benchmark scored on the device (include/romp_hip_rh.h, csrc/rh.hip): what
simple_romp/evaluation/eval_Relative_Human.py and RH_evaluation/evaluation.py compute -- the share of person pairs placed in
the right depth order (PCDR, overall and per age group), mPCKh over the matched people, detection precision / recall / F1 --
on what `forward_batch` returns, without a host round trip: `RelativeHumanEvaluator.update` enqueues
match (romp_eval_match2d, as the reference's match_2d_greedy :209) -> score -> accumulate, `summary()` downloads 24 doubles.

What is restated (RH_evaluation/evaluation.py):
  joints     predictions pj2d_org[:, CROWDPOSE14_FROM_SMPL54] (eval_Relative_Human.py:42-59,70); ground truth of 14 joints as
             stored, of 19 joints through BK19_TO_CROWDPOSE14 (7-character basename) or OCHUMAN19_TO_CROWDPOSE14; an invalid or
             unmapped joint becomes (-2, -2) with flag 0 (:171-190)
  PCKh       _calc_matched_PCKh_ :71-88: a joint counts when both ground-truth COORDINATES are > -1 (not the flag); scale = the
             diagonal of those joints' box; error / scale < 0.143 in float32; fewer than 2 such joints: the row is -1, and the
             reference's mean includes it (`mPCKh`; `mPCKh_scored` leaves those rows out)
  pairs      _calc_relative_depth_error_weak_ :37-69, get_results :101-123: the matched rows with depth_id != -1, every unordered
             pair, dist = depth_j - depth_i (float32), did = id_j - id_i; did == 0: |dist| < thr, did < 0: dist < -thr, did > 0:
             dist > thr, thr as a float32; PCRD = correct / (pairs + miss_fine * missed persons); per age the pairs with either
             member of that age and the missed persons of that age, reported only when the age has pairs

Pair order.  Swapping i and j flips both dist and did, so correctness, the `eq` count and the per-age counts do not depend on
the order in which a pair is taken.  The reference's split of the unequal pairs into "close" (did < 0) and "far" (did > 0),
which it only prints, does: it follows the order of its greedy matches.  Here pairs are taken in ascending ground-truth row
order, `eq` is reported on its own and close + far together as `ordered`.

Precision / recall / F1 are the true ones from the matched counts, as MeshEvaluator reports them.  `reference_prf1` is the
reference's compute_prf1 (:90-99) literally -- it takes tp = n_pred - misses rather than n_gt - misses and rounds to two
decimals -- so that published numbers can be compared.

Not reproduced: the reference does not filter its `gt_inds` by `valid_person` (:203-214), so its indices shift when a person
has no valid keypoint at all.  `load_rh_annots` drops such a person and keeps the indices right.

`python -m romp_amd.relative_human --results R.npz --annots A.npz [--dr_thresh 0.2] [--device cuda:0] [--check]` scores stored
files, the reference's pickled ones or the flat pickle-free format of `save_results`, and prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

from . import lib as L
from .evaluation import MAX_PERSON, _f32, batch_offsets, match_2d_greedy

# joint orders, by name (eval_Relative_Human.py:42-57, RH_evaluation/evaluation.py:16-28)
CROWDPOSE_14 = ('L_Shoulder', 'R_Shoulder', 'L_Elbow', 'R_Elbow', 'L_Wrist', 'R_Wrist', 'L_Hip', 'R_Hip', 'L_Knee', 'R_Knee',
                'L_Ankle', 'R_Ankle', 'Head_top', 'Neck_LSP')
SMPL_54 = ('Pelvis_SMPL', 'L_Hip_SMPL', 'R_Hip_SMPL', 'Spine_SMPL', 'L_Knee', 'R_Knee', 'Thorax_SMPL', 'L_Ankle', 'R_Ankle',
           'Thorax_up_SMPL', 'L_Toe_SMPL', 'R_Toe_SMPL', 'Neck', 'L_Collar', 'R_Collar', 'Jaw', 'L_Shoulder', 'R_Shoulder',
           'L_Elbow', 'R_Elbow', 'L_Wrist', 'R_Wrist', 'L_Hand', 'R_Hand',
           'Nose', 'R_Eye', 'L_Eye', 'R_Ear', 'L_Ear', 'L_BigToe', 'L_SmallToe', 'L_Heel', 'R_BigToe', 'R_SmallToe', 'R_Heel',
           'L_Hand_thumb', 'L_Hand_index', 'L_Hand_middle', 'L_Hand_ring', 'L_Hand_pinky',
           'R_Hand_thumb', 'R_Hand_index', 'R_Hand_middle', 'R_Hand_ring', 'R_Hand_pinky',
           'R_Hip', 'L_Hip', 'Neck_LSP', 'Head_top', 'Pelvis', 'Thorax_MPII', 'Spine_H36M', 'Jaw_H36M', 'Head')
BK_19 = ('Head_top', 'Nose', 'Neck', 'L_Eye', 'R_Eye', 'L_Shoulder', 'R_Shoulder', 'L_Elbow', 'R_Elbow', 'L_Wrist', 'R_Wrist',
         'L_Hip', 'R_Hip', 'L_Knee', 'R_Knee', 'L_Ankle', 'R_Ankle', 'L_BigToe', 'R_BigToe')
OCHUMAN_19 = ('R_Shoulder', 'R_Elbow', 'R_Wrist', 'L_Shoulder', 'L_Elbow', 'L_Wrist', 'R_Hip', 'R_Knee', 'R_Ankle', 'L_Hip',
              'L_Knee', 'L_Ankle', 'Head_top', 'Neck', 'R_Ear', 'L_Ear', 'Nose', 'R_Eye', 'L_Eye')


def joint_mapping(source, target):
    """Row of `source` for each joint of `target`, by name; -1 where the source has no such joint."""
    return [source.index(name) if name in source else -1 for name in target]


CROWDPOSE14_FROM_SMPL54 = joint_mapping(SMPL_54, CROWDPOSE_14)
BK19_TO_CROWDPOSE14 = joint_mapping(BK_19, CROWDPOSE_14)
OCHUMAN19_TO_CROWDPOSE14 = joint_mapping(OCHUMAN_19, CROWDPOSE_14)
AGES = ('adult', 'teen', 'kid', 'baby')                                    # the `age` labels 0..3; -1: unlabelled

# include/romp_hip_rh.h
RH_EQ_PAIRS, RH_EQ_CORRECT, RH_ORD_PAIRS, RH_ORD_CORRECT, RH_AGE_PAIRS, RH_AGE_CORRECT = 0, 1, 2, 3, 4, 5
RH_MISSED, RH_MISSED_AGE, RH_MATCHED, RH_UNSCORED, RH_OVER_CAP, RH_COUNTS = 12, 13, 17, 18, 19, 20
RH_ACC_PCKH_SUM, RH_ACC_N_GT, RH_ACC_N_PRED, RH_ACC_FALSE_POS, RH_ACC = 20, 21, 22, 23, 24
RH_MAX_GT = 4096


def _i32(t, device):
    return torch.as_tensor(t, device=device).to(torch.int32).contiguous()


def score_rows(pred_kp2d, pred_depth, gt_kp2d, gt_depth_id, gt_age, pred_of_gt, gt_offsets, B, dr_thresh=0.2, pck_thresh=0.143,
               max_gt=MAX_PERSON):
    """romp_rh_score on device tensors -> pckh (Ng,) float32, correct_visible (Ng,2) int32, counts (B, RH_COUNTS) int32."""
    pred_kp2d, gt_kp2d = _f32(pred_kp2d), _f32(gt_kp2d)
    dev = gt_kp2d.device
    Np, Ng, J = pred_kp2d.shape[0], gt_kp2d.shape[0], gt_kp2d.shape[1]
    assert pred_kp2d.shape[1:] == (J, 2) or Np == 0, pred_kp2d.shape
    pred_depth, did, age, pog = _f32(pred_depth, dev), _i32(gt_depth_id, dev), _i32(gt_age, dev), _i32(pred_of_gt, dev)
    assert tuple(pred_depth.shape) == (Np,) and tuple(did.shape) == tuple(age.shape) == tuple(pog.shape) == (Ng,)
    goff = _i32(gt_offsets, dev)
    assert tuple(goff.shape) == (B + 1,)
    pckh = torch.full((Ng,), float('nan'), dtype=torch.float32, device=dev)   # (rows of an image index >= B stay NaN / 0)
    cv = torch.zeros(Ng, 2, dtype=torch.int32, device=dev)
    counts = torch.zeros(B, RH_COUNTS, dtype=torch.int32, device=dev)
    L.check(L.load().romp_rh_score(L.ptr(pred_kp2d), L.ptr(pred_depth), Np, L.ptr(gt_kp2d), L.ptr(did), L.ptr(age), L.ptr(pog), Ng,
                                   L.ptr(goff), B, J, int(max_gt), float(dr_thresh), float(pck_thresh), L.ptr(pckh), L.ptr(cv),
                                   L.ptr(counts), L.stream_ptr(dev)))
    return pckh, cv, counts


class RelativeHumanEvaluator:
    """A running Relative Human score over a dataset, kept on the device.

    Predictions under `kp2d_key` with more joints than the ground truth's 14 (the 54 / 71 of `forward_batch`) are reduced by
    CROWDPOSE14_FROM_SMPL54; `depth_key` is (N,3) (its z is the depth) or (N,).  max_pred / max_gt: caps on one image's people."""

    def __init__(self, device, dr_thresh=0.2, miss_fine=0.3, pck_thresh=0.143, iou_thresh=0.05, max_pred=MAX_PERSON, max_gt=MAX_PERSON,
                 norm='frobenius', kp2d_key='pj2d_org', depth_key='cam_trans'):
        self.device = torch.device(device)
        L.load()
        self.dr_thresh, self.miss_fine, self.pck_thresh, self.iou_thresh = float(dr_thresh), float(miss_fine), float(pck_thresh), float(iou_thresh)
        self.max_pred, self.max_gt, self.norm, self.kp2d_key, self.depth_key = int(max_pred), int(max_gt), norm, kp2d_key, depth_key
        self.joint_index = torch.as_tensor(CROWDPOSE14_FROM_SMPL54, dtype=torch.int64, device=self.device)
        self.acc = torch.zeros(RH_ACC, dtype=torch.float64, device=self.device)

    def reset(self):
        self.acc.zero_()

    def update(self, outputs, batch_ids, gts):
        """outputs: what forward_batch returns (`kp2d_key` (N,>=54,2) or (N,14,2) in the ground truth's pixel frame, `depth_key`);
        None when nobody was detected.  batch_ids (N,) ascending.  gts: 'kp2d' (Ng,14,2) with (-2,-2) for a missing joint, 'valid'
        (Ng,14) (None: all), 'depth_id' (Ng,) (-1: none), 'age' (Ng,) (-1, 0..3), 'batch_ids' (Ng,) ascending, 'B' images of the call.
        Enqueues match -> score -> accumulate on the current stream; returns the per-row tensors of this call."""
        dev = self.device
        g2d = _f32(gts['kp2d'], dev)
        Ng, J = g2d.shape[:2]
        B = int(gts['B'])
        if outputs is None:
            p2d, depth = torch.zeros(0, J, 2, device=dev), torch.zeros(0, device=dev)
            batch_ids = torch.zeros(0, dtype=torch.int64, device=dev)
        else:
            p2d, depth = _f32(outputs[self.kp2d_key], dev), _f32(outputs[self.depth_key], dev)
            if p2d.shape[1] != J:
                assert J == len(CROWDPOSE_14) and p2d.shape[1] >= len(SMPL_54), (p2d.shape, J)
                p2d = p2d.index_select(1, self.joint_index)
            if depth.dim() == 2:
                depth = depth[:, 2].contiguous()
        gt_ids = torch.as_tensor(gts['batch_ids'], device=dev)
        gt_of_pred, pred_of_gt, over = match_2d_greedy(p2d, batch_ids, g2d, gts.get('valid'), gt_ids, B, self.iou_thresh, self.max_pred,
                                                       self.max_gt, self.norm, return_over_cap=True)
        pckh, cv, counts = score_rows(p2d, depth, g2d, gts['depth_id'], gts['age'], pred_of_gt, batch_offsets(gt_ids, B), B,
                                      self.dr_thresh, self.pck_thresh, self.max_gt)
        counts[:, RH_OVER_CAP] |= over                                      # (an image over max_pred: the matcher's flag)
        L.check(L.load().romp_rh_accumulate(L.ptr(counts), B, L.ptr(pckh), Ng, L.ptr(gt_of_pred), gt_of_pred.numel(), L.ptr(self.acc),
                                            L.stream_ptr(dev)))
        return {'pckh': pckh, 'correct_visible': cv, 'counts': counts, 'gt_of_pred': gt_of_pred, 'pred_of_gt': pred_of_gt}

    def summary(self):
        """One download -> summarize()."""
        return summarize(self.acc.cpu().numpy(), self.dr_thresh, self.miss_fine)


def reference_prf1(n_pred, misses, false_pos):
    """compute_prf1 (RH_evaluation/evaluation.py:90-99) as written: tp = n_pred - misses, two decimals -> (precision, recall, F1)."""
    if n_pred == 0:
        return [0, 0, 0]
    tp = n_pred - misses
    div = lambda a, b: round(a / b, 2) if b else float('nan')
    return [div(tp, tp + false_pos), div(tp, tp + misses), div(tp, tp + 0.5 * (false_pos + misses))]


def summarize(acc, dr_thresh=0.2, miss_fine=0.3):
    """The fields of RelativeHumanEvaluator.summary() from an accumulator (RH_ACC float64).  Ratios are fractions, not per cent."""
    acc = np.asarray(acc, np.float64)
    assert acc.shape == (RH_ACC,), acc.shape
    if acc[RH_OVER_CAP]:
        raise L.RompHipError('%d image(s) held more people than the evaluator\'s max_pred / max_gt: raise the caps' % acc[RH_OVER_CAP])
    n = lambda k: int(acc[k])
    ratio = lambda a, b: float(a / b) if b else float('nan')
    eq_p, eq_c, or_p, or_c, missed, matched, unscored = (n(k) for k in (RH_EQ_PAIRS, RH_EQ_CORRECT, RH_ORD_PAIRS, RH_ORD_CORRECT, RH_MISSED,
                                                                        RH_MATCHED, RH_UNSCORED))
    n_gt, n_pred, false_pos = n(RH_ACC_N_GT), n(RH_ACC_N_PRED), n(RH_ACC_FALSE_POS)
    res = {'dr_thresh': dr_thresh, 'miss_fine': miss_fine,
           'PCRD': ratio(eq_c + or_c, eq_p + or_p + miss_fine * missed), 'PCRD_eq': ratio(eq_c, eq_p), 'PCRD_ordered': ratio(or_c, or_p)}
    for a, name in enumerate(AGES):
        pairs, correct, gone = n(RH_AGE_PAIRS + 2 * a), n(RH_AGE_CORRECT + 2 * a), n(RH_MISSED_AGE + a)
        if pairs > 0:                                                       # (get_results :120: only an age that has pairs)
            res['PCRD_' + name] = ratio(correct, pairs + miss_fine * gone)
        res.update({'pairs_' + name: pairs, 'correct_' + name: correct, 'missed_' + name: gone})
    res['mPCKh'] = ratio(acc[RH_ACC_PCKH_SUM] - unscored, matched)          # the reference's mean: a row of -1 counts as -1
    res['mPCKh_scored'] = ratio(acc[RH_ACC_PCKH_SUM], matched - unscored)
    res['precision'] = ratio(matched, matched + false_pos)
    res['recall'] = ratio(matched, n_gt)
    pr = res['precision'] + res['recall']
    res['F1'] = 2 * res['precision'] * res['recall'] / pr if pr and pr == pr else float('nan')
    res['reference_prf1'] = reference_prf1(n_pred, missed, false_pos)
    res.update(pairs_eq=eq_p, correct_eq=eq_c, pairs_ordered=or_p, correct_ordered=or_c, matched=matched, misses=missed,
               unscored=unscored, false_positives=false_pos, n_gt=n_gt, n_pred=n_pred)
    return res


# ---------------------------------------------------------------------------------------------------- the reference's files
def crowdpose14_of_annotation(kp2d, image_name):
    """One annotated person, (14,3) or (19,3) rows of x, y, flag -> kp2d (14,2) float32, valid (14,) bool (:171-190)."""
    joint = np.array(kp2d, np.float64).reshape(-1, 3)
    joint[joint[:, 2] == 0] = -2.
    joint[:, 2] = joint[:, 2] > 0
    if len(joint) == 19:
        is_bk = len(os.path.basename(image_name).replace('.jpg', '')) == 7
        mapper = np.asarray(BK19_TO_CROWDPOSE14 if is_bk else OCHUMAN19_TO_CROWDPOSE14)
        joint = joint[mapper]                                               # (-1 picks the last row: overwritten next)
        joint[mapper == -1] = -2.
    elif len(joint) != 14:
        raise ValueError('%s: an annotation of %d joints (14 or 19 expected)' % (image_name, len(joint)))
    return joint[:, :2].astype(np.float32), joint[:, 2] > 0


def load_rh_annots(path):
    """The reference's `<set>_annots.npz` (a pickled dict image name -> list of persons with 'kp2d', 'depth_id', 'age'; loaded
    with allow_pickle on the host) -> flat arrays, images in the file's order: 'image_names' (B,), 'B', and per person 'kp2d'
    (Ng,14,2), 'valid' (Ng,14), 'depth_id', 'age' (Ng,) int32, 'batch_ids' (Ng,) int64, 'person_index' (Ng,) int32 (the person's
    place in its image's list).  A person without 'kp2d', or without one valid joint, is dropped."""
    with np.load(path, allow_pickle=True) as z:
        annots = z['annots'][()]
    names = list(annots.keys())
    kp, valid, did, age, bid, idx = [], [], [], [], [], []
    for b, name in enumerate(names):
        for i, person in enumerate(annots[name]):
            if person.get('kp2d') is None:
                continue
            k, v = crowdpose14_of_annotation(person['kp2d'], name)
            if not v.any():
                continue
            kp.append(k); valid.append(v); did.append(int(person['depth_id'])); age.append(int(person['age'])); bid.append(b); idx.append(i)
    return {'image_names': np.array(names, dtype=np.str_), 'B': len(names),
            'kp2d': np.asarray(kp, np.float32).reshape(-1, 14, 2), 'valid': np.asarray(valid, bool).reshape(-1, 14),
            'depth_id': np.asarray(did, np.int32), 'age': np.asarray(age, np.int32), 'batch_ids': np.asarray(bid, np.int64),
            'person_index': np.asarray(idx, np.int32)}


def load_rh_results(path, image_names):
    """The reference's results file (a pickled dict image name -> list of persons with 'kp2ds' (14,2), 'trans' (3,), or a dict of
    the stacked arrays) -> 'kp2d' (Np,14,2) float32, 'depth' (Np,) float32 (trans[2]), 'batch_ids' (Np,) int64 into `image_names`
    (the annotation file's order).  An image absent from the results has no rows: all its people are misses."""
    with np.load(path, allow_pickle=True) as z:
        results = z['results'][()]
    kp, depth, bid = [], [], []
    for b, name in enumerate(image_names):
        r = results.get(str(name))
        if r is None:
            continue
        if isinstance(r, dict):
            k, t = np.asarray(r['kp2ds']), np.asarray(r['trans'])
        else:
            k, t = np.array([p['kp2ds'] for p in r]), np.array([p['trans'] for p in r])
        k, t = k.reshape(-1, 14, 2), t.reshape(-1, 3)
        kp.append(k.astype(np.float32)); depth.append(t[:, 2].astype(np.float32)); bid += [b] * len(k)
    cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape, np.float32)
    return {'kp2d': cat(kp, (0, 14, 2)), 'depth': cat(depth, (0,)), 'batch_ids': np.asarray(bid, np.int64)}


# ---------------------------------------------------------------------------------------------------- the flat format
RESULT_KEYS, ANNOT_KEYS = ('kp2d', 'depth', 'batch_ids'), ('kp2d', 'valid', 'depth_id', 'age', 'batch_ids', 'B')


def save_results(path, **arrays):
    """A results file (kp2d (Np,14,2), depth (Np,), batch_ids (Np,)) or an annotation file (kp2d (Ng,14,2), valid (Ng,14), depth_id,
    age, batch_ids (Ng,), B; optionally image_names, person_index) of the CLI: plain arrays, no pickle."""
    np.savez(path, **{k: np.asarray(v) for k, v in arrays.items() if v is not None})


def load_results(path, required=RESULT_KEYS):
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    for k in required:
        if k not in d:
            raise ValueError('%s: no array %r' % (path, k))
    n = len(d['batch_ids'])
    if d['kp2d'].ndim != 3 or d['kp2d'].shape[0] != n or d['kp2d'].shape[2] != 2:
        raise ValueError('%s: kp2d %s / batch_ids %s do not belong together' % (path, d['kp2d'].shape, d['batch_ids'].shape))
    for k in ('depth', 'depth_id', 'age'):
        if k in required and d[k].shape != (n,):
            raise ValueError('%s: %s %s for %d rows' % (path, k, d[k].shape, n))
    if 'valid' in required and d['valid'].shape != d['kp2d'].shape[:2]:
        raise ValueError('%s: valid %s for kp2d %s' % (path, d['valid'].shape, d['kp2d'].shape))
    if n and np.any(np.diff(d['batch_ids']) < 0):
        raise ValueError('%s: batch_ids must ascend' % path)
    if 'B' in required and n and int(d['batch_ids'].max()) >= int(d['B']):
        raise ValueError('%s: batch_ids reach %d with B = %d' % (path, d['batch_ids'].max(), d['B']))
    return d


def load_files(results_path, annots_path):
    """Either format of either file (told apart by the names of the arrays, before anything is unpickled) -> results, annots."""
    def names(path):
        with np.load(path, allow_pickle=False) as z:
            return z.files
    annots = load_rh_annots(annots_path) if 'annots' in names(annots_path) else load_results(annots_path, ANNOT_KEYS)
    if 'results' in names(results_path):
        if 'image_names' not in annots:
            raise ValueError('%s: the reference\'s results need an annotation file with image_names' % annots_path)
        results = load_rh_results(results_path, annots['image_names'])
    else:
        results = load_results(results_path, RESULT_KEYS)
    if results['kp2d'].shape[1:] != annots['kp2d'].shape[1:]:
        raise ValueError('results give %s per person, annotations %s' % (results['kp2d'].shape[1:], annots['kp2d'].shape[1:]))
    if len(results['batch_ids']) and int(results['batch_ids'].max()) >= int(annots['B']):
        raise ValueError('results name image %d, the annotations hold %d' % (results['batch_ids'].max(), annots['B']))
    return results, annots


def score_files(results, annots, device='cuda:0', dr_thresh=0.2, miss_fine=0.3, pck_thresh=0.143, iou_thresh=0.05, norm='frobenius',
                images_per_call=32):
    """Score loaded files (load_files) `images_per_call` images at a time through RelativeHumanEvaluator -> summary dict."""
    B = int(annots['B'])
    cap = lambda ids: max(int(np.bincount(np.asarray(ids, np.int64)).max(initial=1)), 1)
    ev = RelativeHumanEvaluator(device, dr_thresh, miss_fine, pck_thresh, iou_thresh, cap(results['batch_ids']), cap(annots['batch_ids']), norm,
                                kp2d_key='kp2d', depth_key='depth')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ev.device)
    for b0 in range(0, B, images_per_call):
        b1 = min(b0 + images_per_call, B)
        ps, gs = [np.flatnonzero((d['batch_ids'] >= b0) & (d['batch_ids'] < b1)) for d in (results, annots)]
        out = {'kp2d': t(results['kp2d'][ps]), 'depth': t(results['depth'][ps])} if len(ps) else None
        g = {k: t(annots[k][gs]) for k in ('kp2d', 'valid', 'depth_id', 'age')}
        g.update(batch_ids=t(annots['batch_ids'][gs] - b0), B=b1 - b0)
        ev.update(out, t(results['batch_ids'][ps] - b0), g)
    return ev.summary()


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m romp_amd.relative_human',
                                 description='Score stored Relative Human results against stored annotations on the device.')
    ap.add_argument('--results', required=True, help="npz: kp2d (Np,14,2), depth (Np,), batch_ids (Np,); or the reference's pickled `results`")
    ap.add_argument('--annots', required=True, help="npz: kp2d, valid, depth_id, age, batch_ids, B; or the reference's pickled `annots`")
    ap.add_argument('--dr_thresh', type=float, default=0.2)
    ap.add_argument('--miss_fine', type=float, default=0.3)
    ap.add_argument('--pck_thresh', type=float, default=0.143)
    ap.add_argument('--iou_thresh', type=float, default=0.05)
    ap.add_argument('--norm', choices=('frobenius', 'spectral'), default='frobenius')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--check', action='store_true', help='load and validate the two files, print their shapes, score nothing')
    a = ap.parse_args(argv)
    results, annots = load_files(a.results, a.annots)
    if a.check:
        shapes = lambda d: {k: list(np.shape(v)) for k, v in sorted(d.items())}
        res = {'results': shapes(results), 'annots': shapes(annots)}
    else:
        res = score_files(results, annots, a.device, a.dr_thresh, a.miss_fine, a.pck_thresh, a.iou_thresh, a.norm)
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main(sys.argv[1:])
