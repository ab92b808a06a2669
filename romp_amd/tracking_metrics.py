"""Tracking scores on the device (include/romp_hip_mot.h, csrc/mot.hip): HOTA, CLEAR-MOT (MOTA, ID switches, ...) and Identity
(IDF1) for many clips per call, on what ``DeviceTracker.update_frames`` left on the device or on stored results.

The definitions are TrackEval's, as the reference ships them under trace2/evaluation/TrackEval/trackeval/metrics: hota.py,
clear.py, identity.py; field names are TrackEval's.  ``score_clip_host`` restates them in numpy + scipy (the host mirror the tests
and the timing compare against, as tracker.py is for the device tracker); the kernels mirror that.

One known difference from the reference's trace2/evaluation/evaluate_tracking.py: it takes HOTA from TrackEval but MOTA, ID switches
and IDF1 from the ``motmetrics`` package with ``max_iou=0.99``; motmetrics is not part of the reference tree and cannot be pinned, so
it is NOT the definition here.  MOTA, IDSW and IDF1 are TrackEval's CLEAR and Identity with a ``threshold`` parameter.  On hard clips
the two can differ in ID switches, because motmetrics keeps the matches of earlier frames by a different rule.

  similarity   IoU of (x, y, w, h) boxes, 0 where the union is 0; an IoU with 1 - IoU > max_iou is set to 0 (accumulate_results).
               Predictions are boxes, or kp2d (N, J, 2) in original-image pixels boxed as pj2ds_to_bbox does (min / max over the
               joints, half extents about the centre enlarged by enlarge_xy: (1.1, 1.18) MuPoTS, (1.0, 1.05) Dyna3DPW)
  HOTA         19 thresholds 0.05 .. 0.95; pass 1 the alignment A[g, k] of id pairs, pass 2 one assignment per frame maximising
               the sum of A * sim
  CLEAR        frames in order, score 1000 [k is the id g had in the previous frame] + sim, 0 below threshold - eps
  Identity     pm[g, k] = frames with sim >= threshold, one assignment per clip.  TrackEval solves a (G+K)^2 matrix padded with
               1e10; that is not built here (see ``_identity_host``)
  combining    ``summary()['reference']``: HOTA / DetA / AssA as eval_tracking_metrics prints them, the mean over clips of each
               clip's mean over alpha, times 100; ``summary()['combined']``: TrackEval's combine_sequences (counts summed over the
               clips, then finalised; HOTA's Ass* weighted by TP) -- what motmetrics' OVERALL row means for MOTA / IDF1

Frames without ground truth are dropped before scoring when ``skip_frames_without_gt`` (prepare_data does so); the kernels
themselves handle empty frames the TrackEval way.

``python -m romp_amd.tracking_metrics --results R.npz --gt G.npz [--threshold 0.5] [--max_iou 0.99] [--enlarge 1.1 1.18] [--check]``
scores stored files -- the flat pickle-free format of ``save_results`` or the reference's ``*_tracking.npz`` and ground-truth dicts --
and prints one JSON line.  ``--check`` also validates the files and compares the device with the host mirror.
``--bench --persons P`` times ``summary()`` against ``score_clip_host`` on synthetic clips.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

from . import lib as L

ALPHAS = np.arange(0.05, 0.99, 0.05)                    # hota.py:17
EPS = np.finfo('float').eps
MAX_DET, MAX_IDS, N_ALPHA = 256, 512, 19                # ROMP_TRACK_MAX_DET, ROMP_TRACK_MAX_CAPACITY, ROMP_MOT_ALPHAS
HOTA_OUT, CLEAR_OUT, ID_OUT = 7, 12, 3
HOTA_INT = ('HOTA_TP', 'HOTA_FN', 'HOTA_FP')
HOTA_FLOAT = ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA', 'RHOTA', 'HOTA(0)', 'LocA(0)', 'HOTALocA(0)')
CLEAR_INT = ('CLR_TP', 'CLR_FN', 'CLR_FP', 'IDSW', 'MT', 'PT', 'ML', 'Frag', 'CLR_Frames')
CLEAR_FLOAT = ('MOTA', 'MOTP', 'MODA', 'CLR_Re', 'CLR_Pr', 'MTR', 'PTR', 'MLR', 'sMOTA', 'CLR_F1', 'FP_per_frame', 'MOTAL', 'MOTP_sum')
ID_INT = ('IDTP', 'IDFN', 'IDFP')
ID_FLOAT = ('IDF1', 'IDR', 'IDP')


# ------------------------------------------------------------------------------------------------ similarity on the host
def boxes_from_kp2d_host(kp2d, enlarge_xy=(1.1, 1.18)):
    """(N, J, 2) -> (N, 4) float64 left, top, width, height (pj2ds_to_bbox, in float64 throughout)."""
    kp = np.asarray(kp2d, np.float64).reshape(len(kp2d), -1, 2)
    lo, hi = kp.min(1), kp.max(1)
    centre = (hi + lo) / 2
    half = (centre - lo) * np.asarray(enlarge_xy, np.float64)
    return np.concatenate([centre - half, half * 2], 1)


def iou_host(gt_boxes, pred_boxes, max_iou=0.99):
    """(n, 4), (m, 4) boxes x, y, w, h -> (n, m) float64 IoU with the max_iou floor."""
    a, b = np.asarray(gt_boxes, np.float64).reshape(-1, 4)[:, None], np.asarray(pred_boxes, np.float64).reshape(-1, 4)[None]
    iw = np.minimum(a[..., 0] + a[..., 2], b[..., 0] + b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
    ih = np.minimum(a[..., 1] + a[..., 3], b[..., 1] + b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0.)
    union = (a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3]) - inter
    iou = np.where(union > 0, inter / np.where(union > 0, union, 1.), 0.)
    return np.where(1. - iou > max_iou, 0., iou)


# ------------------------------------------------------------------------------------------------ clips
def _side(frames, ids, frame_list, what):
    """The rows of one side whose frame is in frame_list, in frame order (stable) -> (kept row indices, rows per frame, dense ids, number of ids)."""
    frames, ids = np.asarray(frames).reshape(-1), np.asarray(ids).reshape(-1)
    if frames.shape != ids.shape:
        raise ValueError('%s: %d frame numbers for %d ids' % (what, len(frames), len(ids)))
    if len(frame_list) == 0 or len(frames) == 0:
        return np.zeros(0, np.int64), np.zeros(len(frame_list), np.int64), np.zeros(0, np.int32), 0
    at = np.clip(np.searchsorted(frame_list, frames), 0, len(frame_list) - 1)
    keep = np.flatnonzero(frame_list[at] == frames)
    keep = keep[np.argsort(at[keep], kind='stable')]
    uniq, dense = np.unique(ids[keep], return_inverse=True)
    key = at[keep].astype(np.int64) * max(len(uniq), 1) + dense
    if len(np.unique(key)) != len(key):
        raise ValueError('%s: an id owns two rows of one frame' % what)
    rows = np.bincount(at[keep], minlength=len(frame_list))
    if rows.max(initial=0) > MAX_DET or len(uniq) > MAX_IDS:
        raise ValueError('%s: %d rows in a frame (at most %d) or %d ids (at most %d)' % (what, rows.max(initial=0), MAX_DET, len(uniq), MAX_IDS))
    return keep, rows, dense.astype(np.int32), len(uniq)


def _frame_list(gt_frames, other_frames, frames, skip_frames_without_gt):
    """The frames that are scored, ascending: those with ground truth, or every frame of the clip (`frames` when given -- the only
    way to name a frame in which neither side has a row -- else every frame either side names)."""
    if skip_frames_without_gt:
        return np.unique(gt_frames)
    if frames is not None:
        return np.unique(np.asarray(frames).reshape(-1))
    both = [a for a in (gt_frames, other_frames) if len(a)]
    return np.unique(np.concatenate(both)) if both else np.zeros(0, np.int64)


def prepare_clip(pred_ids, pred_frames, gt_boxes, gt_ids, gt_frames, pred_boxes=None, pred_kp2d=None, skip_frames_without_gt=True,
                 frames=None):
    """One clip from per-row arrays -> a dict: the frame list (_frame_list), both sides sorted by frame, ids remapped to dense
    0..G-1 / 0..K-1, rows per frame.  Rows of a frame that is not scored are dropped."""
    if (pred_boxes is None) == (pred_kp2d is None):
        raise ValueError('give pred_boxes or pred_kp2d, one of them')
    gt_frames, pred_frames = np.asarray(gt_frames).reshape(-1), np.asarray(pred_frames).reshape(-1)
    gt_boxes = np.asarray(gt_boxes, np.float32).reshape(-1, 4)
    if len(gt_boxes) != len(gt_frames):
        raise ValueError('ground truth: %d boxes for %d frame numbers' % (len(gt_boxes), len(gt_frames)))
    frame_list = _frame_list(gt_frames, pred_frames, frames, skip_frames_without_gt)
    gk, g_rows, g_ids, G = _side(gt_frames, gt_ids, frame_list, 'ground truth')
    pk, p_rows, p_ids, K = _side(pred_frames, pred_ids, frame_list, 'predictions')
    clip = {'T': len(frame_list), 'frames': frame_list, 'gt_rows': g_rows, 'gt_ids': g_ids, 'n_gt_ids': G, 'gt_boxes': gt_boxes[gk],
            'pred_rows': p_rows, 'pred_ids': p_ids, 'n_pred_ids': K, 'pred_boxes': None, 'pred_kp2d': None}
    if pred_boxes is not None:
        pb = np.asarray(pred_boxes, np.float32).reshape(-1, 4)
        if len(pb) != len(pred_frames):
            raise ValueError('predictions: %d boxes for %d frame numbers' % (len(pb), len(pred_frames)))
        clip['pred_boxes'] = pb[pk]
    else:
        kp = np.asarray(pred_kp2d, np.float32)
        if kp.ndim != 3 or kp.shape[2] != 2 or kp.shape[1] < 1 or len(kp) != len(pred_frames):
            raise ValueError('predictions: kp2d must be (N, J, 2) with a row per frame number')
        clip['pred_kp2d'] = kp[pk]
    return clip


def clip_data(clip, max_iou=0.99, enlarge_xy=(1.1, 1.18)):
    """A prepared clip -> the per-frame lists TrackEval's eval_sequence takes (gt_ids, tracker_ids, similarity_scores, the counts)."""
    go, po = np.concatenate([[0], np.cumsum(clip['gt_rows'])]), np.concatenate([[0], np.cumsum(clip['pred_rows'])])
    pb = clip['pred_boxes'] if clip['pred_boxes'] is not None else boxes_from_kp2d_host(clip['pred_kp2d'], enlarge_xy)
    data = {'num_timesteps': clip['T'], 'num_gt_ids': clip['n_gt_ids'], 'num_tracker_ids': clip['n_pred_ids'],
            'num_gt_dets': int(go[-1]), 'num_tracker_dets': int(po[-1]), 'gt_ids': [], 'tracker_ids': [], 'similarity_scores': []}
    for t in range(clip['T']):
        data['gt_ids'].append(clip['gt_ids'][go[t]:go[t + 1]].astype(np.int64))
        data['tracker_ids'].append(clip['pred_ids'][po[t]:po[t + 1]].astype(np.int64))
        data['similarity_scores'].append(iou_host(clip['gt_boxes'][go[t]:go[t + 1]], pb[po[t]:po[t + 1]], max_iou))
    return data


# ------------------------------------------------------------------------------------------------ final fields (host and device share them)
def _hota_fields(tp, fn, fp, loc_sum, assa_sum, assre_sum, asspr_sum):
    tp, fn, fp = np.asarray(tp, np.float64), np.asarray(fn, np.float64), np.asarray(fp, np.float64)
    r = {'HOTA_TP': tp, 'HOTA_FN': fn, 'HOTA_FP': fp}
    r['AssA'], r['AssRe'], r['AssPr'] = (np.asarray(v, np.float64) / np.maximum(1, tp) for v in (assa_sum, assre_sum, asspr_sum))
    r['LocA'] = np.maximum(1e-10, np.asarray(loc_sum, np.float64)) / np.maximum(1e-10, tp)
    return _hota_final(r)


def _hota_final(r):
    tp, fn, fp = r['HOTA_TP'], r['HOTA_FN'], r['HOTA_FP']
    r['DetRe'], r['DetPr'], r['DetA'] = tp / np.maximum(1, tp + fn), tp / np.maximum(1, tp + fp), tp / np.maximum(1, tp + fn + fp)
    r['HOTA'], r['RHOTA'] = np.sqrt(r['DetA'] * r['AssA']), np.sqrt(r['DetRe'] * r['AssA'])
    r['HOTA(0)'], r['LocA(0)'] = float(r['HOTA'][0]), float(r['LocA'][0])
    r['HOTALocA(0)'] = r['HOTA(0)'] * r['LocA(0)']
    return r


def _clear_final(r):
    """The ratios of CLEAR from its counts (clear.py _compute_final_fields)."""
    tp, fn, fp, sw = float(r['CLR_TP']), float(r['CLR_FN']), float(r['CLR_FP']), float(r['IDSW'])
    ids = max(1.0, float(r['MT'] + r['PT'] + r['ML']))
    gt = max(1.0, tp + fn)
    r['MTR'], r['PTR'], r['MLR'] = r['MT'] / ids, r['PT'] / ids, r['ML'] / ids
    r['CLR_Re'], r['CLR_Pr'] = tp / gt, tp / max(1.0, tp + fp)
    r['MODA'], r['MOTA'] = (tp - fp) / gt, (tp - fp - sw) / gt
    r['MOTP'] = r['MOTP_sum'] / max(1.0, tp)
    r['sMOTA'] = (r['MOTP_sum'] - fp - sw) / gt
    r['CLR_F1'] = tp / max(1.0, tp + 0.5 * fn + 0.5 * fp)
    r['FP_per_frame'] = fp / max(1.0, float(r['CLR_Frames']))
    r['MOTAL'] = (tp - fp - (np.log10(sw) if sw > 0 else sw)) / gt
    return r


def _clear_fields(tp, fn, fp, idsw, mt, pt, ml, frag, frames, motp_sum, gt_dets, trk_dets, num_gt_ids):
    """One clip's CLEAR result from its counts, with the two early returns of eval_sequence (clear.py:46-54), which skip the ratios."""
    r = dict.fromkeys(CLEAR_INT, 0)
    r.update(dict.fromkeys(CLEAR_FLOAT, 0.0))
    if trk_dets == 0:
        r.update(CLR_FN=int(gt_dets), ML=int(num_gt_ids), MLR=1.0)
        return r
    if gt_dets == 0:
        r.update(CLR_FP=int(trk_dets), MLR=1.0)
        return r
    r.update(CLR_TP=int(tp), CLR_FN=int(fn), CLR_FP=int(fp), IDSW=int(idsw), MT=int(mt), PT=int(pt), ML=int(ml), Frag=int(frag),
             CLR_Frames=int(frames), MOTP_sum=float(motp_sum))
    return _clear_final(r)


def _identity_fields(idtp, idfn, idfp):
    r = {'IDTP': int(idtp), 'IDFN': int(idfn), 'IDFP': int(idfp)}
    r['IDR'], r['IDP'] = r['IDTP'] / max(1.0, r['IDTP'] + r['IDFN']), r['IDTP'] / max(1.0, r['IDTP'] + r['IDFP'])
    r['IDF1'] = r['IDTP'] / max(1.0, r['IDTP'] + 0.5 * r['IDFP'] + 0.5 * r['IDFN'])
    return r


def combine_clips(clips):
    """{name: per-clip result} -> ('reference' figures, 'combined' = TrackEval's combine_sequences of each metric)."""
    res = list(clips.values())
    ref = {k: float(np.mean([np.mean(r['HOTA'][k]) for r in res]) * 100) for k in ('HOTA', 'DetA', 'AssA')}
    h = {k: sum(r['HOTA'][k] for r in res) for k in HOTA_INT}
    for k in ('AssRe', 'AssPr', 'AssA'):
        h[k] = sum(r['HOTA'][k] * r['HOTA']['HOTA_TP'] for r in res) / np.maximum(1.0, h['HOTA_TP'])
    h['LocA'] = np.maximum(1e-10, sum(r['HOTA']['LocA'] * r['HOTA']['HOTA_TP'] for r in res)) / np.maximum(1e-10, h['HOTA_TP'])
    c = {k: sum(r['CLEAR'][k] for r in res) for k in CLEAR_INT + ('MOTP_sum',)}
    i = {k: sum(r['Identity'][k] for r in res) for k in ID_INT}
    return ref, {'HOTA': _hota_final(h), 'CLEAR': _clear_final(c), 'Identity': _identity_fields(i['IDTP'], i['IDFN'], i['IDFP'])}


# ------------------------------------------------------------------------------------------------ the host mirror
def _hota_host(data, trace=None):
    from scipy.optimize import linear_sum_assignment
    na = len(ALPHAS)
    tp, fn, fp, loc = np.zeros(na), np.zeros(na), np.zeros(na), np.zeros(na)
    ass = np.zeros((3, na))
    if data['num_tracker_dets'] == 0:
        fn[:] = data['num_gt_dets']
    elif data['num_gt_dets'] == 0:
        fp[:] = data['num_tracker_dets']
    else:
        G, K = data['num_gt_ids'], data['num_tracker_ids']
        potential, gc, tc = np.zeros((G, K)), np.zeros((G, 1)), np.zeros((1, K))
        for g, k, sim in zip(data['gt_ids'], data['tracker_ids'], data['similarity_scores']):
            den = sim.sum(0)[None, :] + sim.sum(1)[:, None] - sim
            ok = den > EPS
            rel = np.zeros_like(sim)
            rel[ok] = sim[ok] / den[ok]
            potential[g[:, None], k[None, :]] += rel
            gc[g] += 1
            tc[0, k] += 1
        with np.errstate(invalid='ignore', divide='ignore'):
            A = potential / (gc + tc - potential)
        matches = np.zeros((na, G, K))
        for t, (g, k, sim) in enumerate(zip(data['gt_ids'], data['tracker_ids'], data['similarity_scores'])):
            if len(g) == 0:
                fp += len(k)
                continue
            if len(k) == 0:
                fn += len(g)
                continue
            score = A[g[:, None], k[None, :]] * sim
            if trace is not None:
                trace.append(('HOTA', t, score))
            rows, cols = linear_sum_assignment(-score)
            got = sim[rows, cols]
            for a, alpha in enumerate(ALPHAS):
                hit = got >= alpha - EPS
                n = int(hit.sum())
                tp[a] += n
                fn[a] += len(g) - n
                fp[a] += len(k) - n
                loc[a] += got[hit].sum()
                matches[a, g[rows[hit]], k[cols[hit]]] += 1
        for a in range(na):
            m = matches[a]
            ass[0, a] = np.sum(m * (m / np.maximum(1, gc + tc - m)))
            ass[1, a] = np.sum(m * (m / np.maximum(1, gc)))
            ass[2, a] = np.sum(m * (m / np.maximum(1, tc)))
    return _hota_fields(tp, fn, fp, loc, ass[0], ass[1], ass[2])


def _clear_host(data, threshold, trace=None):
    from scipy.optimize import linear_sum_assignment
    G = data['num_gt_ids']
    tp = fn = fp = idsw = 0
    motp_sum = 0.0
    present, matched, runs = np.zeros(G), np.zeros(G), np.zeros(G)
    last_id = np.full(G, -1, np.int64)                  # the id g was matched to most recently, in any earlier frame (IDSW)
    prev_id = np.full(G, -1, np.int64)                  # ... in the previous scored frame (the matching bonus, fragments)
    if data['num_tracker_dets'] and data['num_gt_dets']:
        for t, (g, k, sim) in enumerate(zip(data['gt_ids'], data['tracker_ids'], data['similarity_scores'])):
            if len(g) == 0:
                fp += len(k)
                continue
            if len(k) == 0:
                fn += len(g)
                present[g] += 1
                continue
            score = 1000. * (k[None, :] == prev_id[g][:, None]) + sim
            score[sim < threshold - EPS] = 0
            if trace is not None:
                trace.append(('CLEAR', t, score))
            rows, cols = linear_sum_assignment(-score)
            keep = score[rows, cols] > EPS
            rows, cols = rows[keep], cols[keep]
            mg, mk = g[rows], k[cols]
            idsw += int(np.sum((last_id[mg] >= 0) & (last_id[mg] != mk)))
            present[g] += 1
            matched[mg] += 1
            was = prev_id >= 0
            last_id[mg] = mk
            prev_id[:] = -1
            prev_id[mg] = mk
            runs += ~was & (prev_id >= 0)
            tp += len(mg)
            fn += len(g) - len(mg)
            fp += len(k) - len(mg)
            motp_sum += float(sim[rows, cols].sum())
    ratio = matched[present > 0] / present[present > 0]
    mt = int(np.sum(ratio > 0.8))
    pt = int(np.sum(ratio >= 0.2)) - mt
    frag = int(np.sum(runs[runs > 0] - 1))
    return _clear_fields(tp, fn, fp, idsw, mt, pt, G - mt - pt, frag, data['num_timesteps'], motp_sum, data['num_gt_dets'],
                         data['num_tracker_dets'], G)


def _identity_host(data, threshold):
    """identity.py solves min over (G+K)^2 assignments of [fn + fp]: rows 0..G-1 the ground-truth ids, columns 0..K-1 the tracker ids,
    a diagonal of "unmatched" entries for each, 1e10 elsewhere.  Pairing g with k costs gt_count[g] + trk_count[k] - 2 pm[g, k], leaving
    g alone costs gt_count[g], leaving k alone trk_count[k]; the padding lets every id stay alone.  So the optimum is
    sum gt_count + sum trk_count - 2 max (sum of pm over a one-to-one pairing), and IDTP = that maximum: an n x m problem on -pm
    in which an unpaired id costs 0.  IDFN = sum gt_count - IDTP, IDFP = sum trk_count - IDTP.  Tied optima give the same value."""
    from scipy.optimize import linear_sum_assignment
    if data['num_tracker_dets'] == 0:
        return _identity_fields(0, data['num_gt_dets'], 0)
    if data['num_gt_dets'] == 0:
        return _identity_fields(0, 0, data['num_tracker_dets'])
    pm = np.zeros((data['num_gt_ids'], data['num_tracker_ids']))
    for g, k, sim in zip(data['gt_ids'], data['tracker_ids'], data['similarity_scores']):
        r, c = np.nonzero(sim >= threshold)
        pm[g[r], k[c]] += 1
    rows, cols = linear_sum_assignment(-pm)
    idtp = int(pm[rows, cols].sum())
    return _identity_fields(idtp, data['num_gt_dets'] - idtp, data['num_tracker_dets'] - idtp)


def score_data_host(data, threshold=0.5, trace=None):
    """TrackEval-style per-frame lists -> {'HOTA': ..., 'CLEAR': ..., 'Identity': ...}.  trace (a list): receives (metric, frame,
    score matrix) of every per-frame assignment."""
    return {'HOTA': _hota_host(data, trace), 'CLEAR': _clear_host(data, threshold, trace), 'Identity': _identity_host(data, threshold)}


def score_clip_host(pred_ids, pred_frames, gt_boxes, gt_ids, gt_frames, pred_boxes=None, pred_kp2d=None, threshold=0.5, max_iou=0.99,
                    enlarge_xy=(1.1, 1.18), skip_frames_without_gt=True, frames=None):
    """The three metrics of one clip in numpy + scipy.optimize.linear_sum_assignment: the host mirror of the device path."""
    clip = prepare_clip(pred_ids, pred_frames, gt_boxes, gt_ids, gt_frames, pred_boxes, pred_kp2d, skip_frames_without_gt, frames)
    return score_data_host(clip_data(clip, max_iou, enlarge_xy), threshold)


# ------------------------------------------------------------------------------------------------ the raw device calls
def _i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def pack_layout(clip_frames, gt_off, pred_off, n_gt_ids, n_pred_ids):
    """romp_mot_pack: the checked int64 block of a layout, as a numpy array (ROMP_EINVAL raises RompHipError; no device call)."""
    lib = L.load()
    cf, cfp = _i32(clip_frames)
    go, gop = _i32(gt_off)
    po, pop = _i32(pred_off)
    ng, ngp = _i32(n_gt_ids)
    npd, npp = _i32(n_pred_ids)
    S, F = len(cf) - 1, len(go) - 1
    if len(po) != F + 1 or len(ng) != S or len(npd) != S:
        raise ValueError('pack_layout: array lengths do not fit S = %d, F = %d' % (S, F))
    words = lib.romp_mot_pack(S, F, cfp, gop, pop, ngp, npp, None, 0)
    if words < 0:
        L.check(words)
    block = np.zeros(words, np.int64)
    rc = lib.romp_mot_pack(S, F, cfp, gop, pop, ngp, npp, block.ctypes.data_as(C.POINTER(C.c_int64)), words)
    if rc < 0:
        L.check(rc)
    return block


def _bp(block):
    return block.ctypes.data_as(C.POINTER(C.c_int64))


def boxes_from_kp2d(kp2d, enlarge_xy=(1.1, 1.18)):
    """kp2d (N, J, 2) float32 on the device -> (N, 4) float64 boxes left, top, width, height on the device (one launch)."""
    import torch
    lib = L.load()
    assert kp2d.is_cuda and kp2d.dtype == torch.float32 and kp2d.dim() == 3 and kp2d.shape[2] == 2
    kp2d = kp2d.contiguous()
    out = torch.empty(kp2d.shape[0], 4, dtype=torch.float64, device=kp2d.device)
    if kp2d.shape[0]:
        with torch.cuda.device(kp2d.device):
            L.check(lib.romp_mot_boxes(L.ptr(kp2d), kp2d.shape[0], kp2d.shape[1], float(enlarge_xy[0]), float(enlarge_xy[1]), L.ptr(out),
                                       L.stream_ptr(kp2d.device)))
    return out


def score_clips(device, block, gt_boxes, gt_ids, pred_ids, pred_boxes=None, pred_kp2d=None, threshold=0.5, max_iou=0.99,
                enlarge_xy=(1.1, 1.18), out=None, metrics=True):
    """The raw device calls on a packed layout (``pack_layout``): tables -> similarity -> HOTA -> CLEAR -> Identity, 9 launches, no
    synchronisation.  gt_boxes (rows, 4) float32, gt_ids / pred_ids int32, pred_boxes (rows, 4) float32 or pred_kp2d (rows, J, 2)
    float32, all on `device`.  -> dict: sim, rowsum, colsum, hota (S, 19, 7), clear (S, 12), identity (S, 3) float64 device tensors
    (views of `out`, S * 148 doubles, when given) and the number of launches."""
    import torch
    lib = L.load()
    device = torch.device(device)
    S, F, n_gt, n_pred, n_sim = (int(block[i]) for i in (1, 2, 4, 5, 6))
    for t, rows, what in ((gt_boxes, n_gt, 'gt_boxes'), (gt_ids, n_gt, 'gt_ids'), (pred_ids, n_pred, 'pred_ids'), (pred_boxes, n_pred, 'pred_boxes'),
                          (pred_kp2d, n_pred, 'pred_kp2d')):
        if t is not None and (not t.is_cuda or t.shape[0] != rows or not t.is_contiguous()):
            raise ValueError('score_clips: %s must be a contiguous device tensor of %d rows' % (what, rows))
    if n_pred and (pred_boxes is None) == (pred_kp2d is None):
        raise ValueError('score_clips: give pred_boxes or pred_kp2d, one of them')
    assert gt_boxes.dtype == torch.float32 and gt_ids.dtype == torch.int32 and pred_ids.dtype == torch.int32
    assert (pred_boxes is None or pred_boxes.dtype == torch.float32) and (pred_kp2d is None or pred_kp2d.dtype == torch.float32)
    nbytes = C.c_int64(0)
    L.check(lib.romp_mot_workspace_bytes(_bp(block), C.byref(nbytes)))
    f64 = dict(dtype=torch.float64, device=device)
    ws = torch.empty(nbytes.value // 8 + 1, **f64)
    sim, rowsum, colsum = torch.empty(n_sim, **f64), torch.empty(n_gt, **f64), torch.empty(n_pred, **f64)
    blk = torch.from_numpy(block).to(device)
    J = int(pred_kp2d.shape[1]) if pred_kp2d is not None else 0
    p = L.ptr
    launches = 0
    with torch.cuda.device(device):
        st = L.stream_ptr(device)
        L.check(lib.romp_mot_tables(_bp(block), p(blk), p(gt_ids), p(pred_ids), p(ws), st))
        L.check(lib.romp_mot_similarity(_bp(block), p(blk), p(gt_boxes), p(gt_ids), p(pred_boxes), p(pred_kp2d) if pred_boxes is None else None, J,
                                        float(enlarge_xy[0]), float(enlarge_xy[1]), p(pred_ids), float(max_iou), p(sim), p(rowsum), p(colsum), st))
        launches += 2 if F else 0
        res = {'sim': sim, 'rowsum': rowsum, 'colsum': colsum, 'block': blk, 'workspace': ws}
        if metrics:
            if out is None:
                out = torch.empty(S * (N_ALPHA * HOTA_OUT + CLEAR_OUT + ID_OUT), **f64)
            hota, clear, ident = out[:S * N_ALPHA * HOTA_OUT], out[S * N_ALPHA * HOTA_OUT:S * (N_ALPHA * HOTA_OUT + CLEAR_OUT)], \
                out[S * (N_ALPHA * HOTA_OUT + CLEAR_OUT):S * (N_ALPHA * HOTA_OUT + CLEAR_OUT + ID_OUT)]
            alphas = (C.c_double * N_ALPHA)(*ALPHAS.tolist())
            L.check(lib.romp_mot_hota(_bp(block), p(blk), p(gt_ids), p(pred_ids), p(sim), p(rowsum), p(colsum), alphas, p(ws), p(hota), st))
            L.check(lib.romp_mot_clear(_bp(block), p(blk), p(gt_ids), p(pred_ids), p(sim), float(threshold), p(ws), p(clear), st))
            L.check(lib.romp_mot_identity(_bp(block), p(blk), p(gt_ids), p(pred_ids), p(sim), float(threshold), p(ws), p(ident), st))
            pairs = int(block[10]) > 0
            launches += (2 if pairs else 0) + (1 if F else 0) + 1 + 1 + (1 if pairs else 0) + 1
            res.update(hota=hota.view(S, N_ALPHA, HOTA_OUT), clear=clear.view(S, CLEAR_OUT), identity=ident.view(S, ID_OUT), out=out)
    res['launches'] = launches
    return res


def box_iou(gt_boxes, pred_boxes=None, pred_kp2d=None, max_iou=0.99, enlarge_xy=(1.1, 1.18)):
    """The similarity of one frame on the device: gt_boxes (n, 4), pred_boxes (m, 4) or pred_kp2d (m, J, 2), float32, at most 256
    rows each -> (n, m) float64."""
    import torch
    n, m = gt_boxes.shape[0], (pred_boxes if pred_boxes is not None else pred_kp2d).shape[0]
    block = pack_layout([0, 1], [0, n], [0, m], [min(n, MAX_IDS)], [min(m, MAX_IDS)])
    dev = gt_boxes.device
    r = score_clips(dev, block, gt_boxes.contiguous(), torch.arange(n, dtype=torch.int32, device=dev), torch.arange(m, dtype=torch.int32, device=dev),
                    None if pred_boxes is None else pred_boxes.contiguous(), None if pred_kp2d is None else pred_kp2d.contiguous(),
                    max_iou=max_iou, enlarge_xy=enlarge_xy, metrics=False)
    return r['sim'].view(n, m)


def _dense_ids_device(ids):
    """int32 ids with -1 for "nobody", any shape -> (the ids as ranks 0..n-1 of the distinct values, -1 kept; n as a 0-d tensor),
    by a sort and a running count: fixed shapes, so nothing is read back."""
    import torch
    flat = ids.reshape(-1)
    srt, order = torch.sort(flat, stable=True)
    first = torch.ones_like(srt, dtype=torch.bool)
    first[1:] = srt[1:] != srt[:-1]
    rank = torch.cumsum(first, 0) - 1 - (srt[0] < 0).to(torch.int64)
    dense = torch.empty_like(flat)
    dense[order] = rank.to(flat.dtype)
    return dense.reshape(ids.shape), rank[-1] + 1


class TrackingEvaluator(object):
    """Collects clips, scores them all in one pass of nine launches, downloads once.  One evaluator takes predictions of one kind:
    boxes, or kp2d of one joint count."""

    def __init__(self, device, threshold=0.5, max_iou=0.99, enlarge_xy=(1.1, 1.18), skip_frames_without_gt=True):
        import torch
        self.device = torch.device(device)
        if not 0. < threshold <= 1. or not 0. <= max_iou <= 1. or len(enlarge_xy) != 2 or min(enlarge_xy) <= 0:
            raise ValueError('TrackingEvaluator: threshold in (0, 1], max_iou in [0, 1], two positive enlargements')
        self.threshold, self.max_iou, self.enlarge_xy = float(threshold), float(max_iou), (float(enlarge_xy[0]), float(enlarge_xy[1]))
        self.skip_frames_without_gt = bool(skip_frames_without_gt)
        self.lib = L.load()
        self.reset()

    def reset(self):
        self.clips, self.last_launches, self.last_download_bytes, self.last_raw = [], 0, 0, None      # (last_raw: the doubles of the download)

    def _add(self, name, clip):
        if any(c['name'] == name for c in self.clips):
            raise ValueError('a clip named %r is there already' % (name,))
        kinds = {('boxes',) if c['pred_boxes'] is not None else ('kp2d', c['pred_kp2d'].shape[1]) for c in self.clips + [clip]
                 if int(np.sum(c['pred_rows']))}                   # (a clip without predictions has no kind of its own)
        if len(kinds) > 1:
            raise ValueError('one evaluator scores predictions of one kind (boxes, or kp2d of one joint count): %s' % sorted(kinds))
        clip['name'] = name
        self.clips.append(clip)

    def add_clip(self, name, pred_ids, pred_frames, gt_boxes, gt_ids, gt_frames, pred_boxes=None, pred_kp2d=None, frames=None):
        """One clip from host arrays with one row per detection: ids (any integers), frame numbers (any sortable values), boxes
        (x, y, w, h) or kp2d (N, J, 2).  frames: every frame number of the clip, when frames without any row are to count."""
        self._add(name, prepare_clip(pred_ids, pred_frames, gt_boxes, gt_ids, gt_frames, pred_boxes, pred_kp2d, self.skip_frames_without_gt, frames))

    def add_tracked(self, name, out_count, out_ids, out_rows, kp2d, gt_boxes, gt_ids, gt_frames, frames=None):
        """What ``DeviceTracker.update_frames`` returned for T frames (count (T), ids and rows (T, capacity), capacity <= 256), still
        on the device, with the kp2d (N, J, 2) rows (pj2d_org) those frames index; frames: the frame numbers of the T frames
        (default 0..T-1).  Nothing is downloaded: the padded output is the prediction side as it is, ids are ranked on the device."""
        import torch
        T, cap = out_ids.shape
        if cap > MAX_DET:
            raise ValueError('add_tracked: a tracker of capacity %d, at most %d rows per frame can be scored' % (cap, MAX_DET))
        assert out_count.shape == (T,) and out_rows.shape == (T, cap) and kp2d.dim() == 3 and kp2d.shape[2] == 2 and kp2d.dtype == torch.float32
        frames = np.arange(T) if frames is None else np.asarray(frames).reshape(-1)
        if len(frames) != T or len(np.unique(frames)) != T:
            raise ValueError('add_tracked: %d distinct frame numbers needed' % T)
        gt_frames = np.asarray(gt_frames).reshape(-1)
        frame_list = _frame_list(gt_frames, frames, None, self.skip_frames_without_gt)
        gk, g_rows, g_ids, G = _side(gt_frames, gt_ids, frame_list, 'ground truth')
        clip = {'T': len(frame_list), 'frames': frame_list, 'gt_rows': g_rows, 'gt_ids': g_ids, 'n_gt_ids': G,
                'gt_boxes': np.asarray(gt_boxes, np.float32).reshape(-1, 4)[gk], 'pred_boxes': None, 'pred_kp2d': None, 'overflow': None}
        order = np.argsort(frames, kind='stable')
        at = np.clip(np.searchsorted(frame_list, frames[order]), 0, max(len(frame_list) - 1, 0))
        sel = order[frame_list[at] == frames[order]] if len(frame_list) else order[:0]          # the tracker's frames that are scored, in frame order
        rows = np.zeros(len(frame_list), np.int64)
        if len(sel) and kp2d.shape[0]:
            rows[np.searchsorted(frame_list, frames[sel])] = cap
            idx = torch.as_tensor(sel, dtype=torch.long).to(self.device)
            ids = torch.where(torch.arange(cap, device=self.device)[None, :] < out_count[idx][:, None], out_ids[idx], torch.full_like(out_ids[idx], -1))
            dense, n = _dense_ids_device(ids)
            clip['pred_ids'], clip['overflow'] = dense.reshape(-1).contiguous(), (n > MAX_IDS)
            clip['pred_kp2d'] = kp2d[out_rows[idx].reshape(-1).long()].contiguous()
            clip['n_pred_ids'] = min(MAX_IDS, len(sel) * cap)
        else:
            clip['pred_ids'], clip['n_pred_ids'] = np.zeros(0, np.int32), 0
            clip['pred_kp2d'] = np.zeros((0, kp2d.shape[1], 2), np.float32)
        clip['pred_rows'] = rows
        self._add(name, clip)

    def _gather(self, key, dtype, tail):
        """The rows of every clip under `key`, one after the other, on the device: host parts in one upload where all are host arrays."""
        import torch
        parts = [c[key] for c in self.clips]
        if all(isinstance(p, np.ndarray) for p in parts):
            return torch.from_numpy(np.ascontiguousarray(np.concatenate([p.reshape((-1,) + tail) for p in parts]), dtype)).to(self.device)
        tdt = {np.float32: torch.float32, np.int32: torch.int32}[dtype]
        return torch.cat([(torch.from_numpy(np.ascontiguousarray(p, dtype)).to(self.device) if isinstance(p, np.ndarray) else p.to(tdt)).reshape((-1,) + tail)
                          for p in parts]).contiguous()

    def summary(self):
        """-> {'clips': {name: {'HOTA', 'CLEAR', 'Identity'}}, 'reference': {'HOTA', 'DetA', 'AssA'}, 'combined': {...}}; one download."""
        import torch
        if not self.clips:
            raise ValueError('TrackingEvaluator.summary: no clips')
        S = len(self.clips)
        clip_frames = np.concatenate([[0], np.cumsum([c['T'] for c in self.clips])])
        gt_off = np.concatenate([[0], np.cumsum(np.concatenate([c['gt_rows'] for c in self.clips]))])
        pred_off = np.concatenate([[0], np.cumsum(np.concatenate([c['pred_rows'] for c in self.clips]))])
        block = pack_layout(clip_frames, gt_off, pred_off, [c['n_gt_ids'] for c in self.clips], [c['n_pred_ids'] for c in self.clips])
        kp = next((c['pred_kp2d'] for c in self.clips if c['pred_kp2d'] is not None and c['pred_kp2d'].shape[0]), None)
        pred_boxes = pred_kp2d = None
        if kp is not None or all(c['pred_boxes'] is None for c in self.clips):
            J = kp.shape[1] if kp is not None else 1
            pred_kp2d = self._gather_kind('pred_kp2d', (J, 2))
        else:
            pred_boxes = self._gather_kind('pred_boxes', (4,))
        gt_boxes, gt_ids, pred_ids = self._gather('gt_boxes', np.float32, (4,)), self._gather('gt_ids', np.int32, ()), self._gather('pred_ids', np.int32, ())
        n_out = S * (N_ALPHA * HOTA_OUT + CLEAR_OUT + ID_OUT)
        out = torch.empty(n_out + S, dtype=torch.float64, device=self.device)
        res = score_clips(self.device, block, gt_boxes, gt_ids, pred_ids, pred_boxes, pred_kp2d, self.threshold, self.max_iou, self.enlarge_xy, out=out)
        flags = [c.get('overflow') for c in self.clips]
        out[n_out:] = torch.stack([f.to(torch.float64) if f is not None else torch.zeros((), dtype=torch.float64, device=self.device) for f in flags])
        host = out.cpu().numpy()                                   # the ONE download
        self.last_launches, self.last_download_bytes, self.last_raw = res['launches'], host.nbytes, host
        for c, flag in zip(self.clips, host[n_out:]):
            if flag:
                raise L.RompHipError('clip %r: the tracker gave out more than %d ids, more than one clip can hold' % (c['name'], MAX_IDS))
        hota = host[:S * N_ALPHA * HOTA_OUT].reshape(S, N_ALPHA, HOTA_OUT)
        clear = host[S * N_ALPHA * HOTA_OUT:S * (N_ALPHA * HOTA_OUT + CLEAR_OUT)].reshape(S, CLEAR_OUT)
        ident = host[S * (N_ALPHA * HOTA_OUT + CLEAR_OUT):n_out].reshape(S, ID_OUT)
        clips = {}
        for s, c in enumerate(self.clips):
            h, cl = hota[s], clear[s]
            clips[c['name']] = {'HOTA': _hota_fields(*(h[:, i] for i in range(HOTA_OUT))),
                                'CLEAR': _clear_fields(*cl.tolist(), num_gt_ids=c['n_gt_ids']),
                                'Identity': _identity_fields(*ident[s].tolist())}
        ref, comb = combine_clips(clips)
        return {'clips': clips, 'reference': ref, 'combined': comb}

    def _gather_kind(self, key, tail):
        """The predictions of every clip in the evaluator's one kind; a clip without predictions contributes no rows."""
        import torch
        parts = [c[key] for c in self.clips if c[key] is not None and c[key].shape[0]]
        if not parts:
            return torch.zeros((0,) + tail, dtype=torch.float32, device=self.device)
        if all(isinstance(p, np.ndarray) for p in parts):          # one upload
            return torch.from_numpy(np.ascontiguousarray(np.concatenate(parts), np.float32)).to(self.device)
        return torch.cat([torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(self.device) if isinstance(p, np.ndarray) else p.float()
                          for p in parts]).contiguous()


# ------------------------------------------------------------------------------------------------ files
def save_results(path, clips):
    """{name: {'ids', 'frames', 'boxes' | 'kp2d'}} -> a flat npz without pickled objects ('names', then '<i>/ids', '<i>/frames', ...).
    The same format holds predictions and ground truth (boxes)."""
    names = sorted(clips)
    arrays = {'names': np.asarray(names, dtype=np.str_)}
    for i, n in enumerate(names):
        c = clips[n]
        if ('boxes' in c) == ('kp2d' in c):
            raise ValueError('clip %r: boxes or kp2d, one of them' % n)
        arrays['%d/ids' % i], arrays['%d/frames' % i] = np.asarray(c['ids'], np.int64).reshape(-1), np.asarray(c['frames'], np.int64).reshape(-1)
        if 'boxes' in c:
            arrays['%d/boxes' % i] = np.asarray(c['boxes'], np.float32).reshape(-1, 4)
        else:
            arrays['%d/kp2d' % i] = np.asarray(c['kp2d'], np.float32)
        if len(arrays['%d/ids' % i]) != len(arrays['%d/frames' % i]) or len(arrays['%d/ids' % i]) != len(c['boxes'] if 'boxes' in c else c['kp2d']):
            raise ValueError('clip %r: ids, frames and boxes / kp2d differ in length' % n)
    np.savez_compressed(path, **arrays)


def _load_flat(z):
    out = {}
    for i, n in enumerate(z['names'].tolist()):
        c = {'ids': z['%d/ids' % i], 'frames': z['%d/frames' % i]}
        for k in ('boxes', 'kp2d'):
            if '%d/%s' % (i, k) in z.files:
                c[k] = z['%d/%s' % (i, k)]
        out[str(n)] = c
    return out


def _rows_of_frames(per_frame):
    """[(frame, ids, boxes or None, kp2d or None)] -> one clip dict."""
    ids, frames, boxes, kps = [], [], [], []
    for fr, i, b, k in per_frame:
        i = np.asarray(i).reshape(-1)
        ids.append(i.astype(np.int64))
        frames += [fr] * len(i)
        if b is not None and len(i):
            boxes.append(np.asarray(b, np.float32).reshape(-1, 4))
        if k is not None and len(i):
            kps.append(np.asarray(k, np.float32).reshape(len(i), -1, 2))
    c = {'ids': np.concatenate(ids) if ids else np.zeros(0, np.int64), 'frames': np.asarray(frames)}
    if kps and sum(len(k) for k in kps) == len(c['ids']):
        c['kp2d'] = np.concatenate(kps)
    else:
        c['boxes'] = np.concatenate(boxes) if boxes else np.zeros((0, 4), np.float32)
    return c


def load_results(path):
    """A file of ``save_results``, or one of the reference's: '<clip>_tracking.npz' with tracking[frame]['track_ids' | 'track_bbox' |
    'pj2ds'] (predictions of one clip; pj2ds are preferred, as adjust_tracking_results re-boxes from them) or a ground-truth file with
    annots[clip][frame] = [paths, ids, boxes, dense ids] (through allow_pickle).  -> {name: {'ids', 'frames', 'boxes' | 'kp2d'}}."""
    with np.load(path, allow_pickle=False) as z:
        if 'names' in z.files:
            return _load_flat(z)
    with np.load(path, allow_pickle=True) as z:
        if 'tracking' in z.files:
            tr = z['tracking'][()]
            name = os.path.basename(path).replace('_tracking.npz', '').replace('.npz', '')
            return {name: _rows_of_frames([(fr, v['track_ids'], v.get('track_bbox'), v.get('pj2ds')) for fr, v in sorted(tr.items())])}
        if 'annots' in z.files:
            an = z['annots'][()]
            return {str(n): _rows_of_frames([(fr, v[3], v[2], None) for fr, v in sorted(frames.items())]) for n, frames in an.items()}
    raise ValueError('%s: neither a save_results file nor one of the reference\'s (tracking / annots)' % path)


def validate_files(results, gt):
    """What --check looks at before scoring: -> a list of complaints (empty: fine)."""
    bad = []
    for n in sorted(set(results) | set(gt)):
        if n not in results or n not in gt:
            bad.append('clip %r is missing from %s' % (n, 'the results' if n not in results else 'the ground truth'))
            continue
        if 'boxes' not in gt[n]:
            bad.append('clip %r: the ground truth must be boxes' % n)
        for what, c in (('results', results[n]), ('ground truth', gt[n])):
            key = np.stack([np.unique(c['frames'], return_inverse=True)[1].reshape(-1), np.asarray(c['ids']).reshape(-1)], 1) if len(c['ids']) else np.zeros((0, 2))
            if len(np.unique(key, axis=0)) != len(key):
                bad.append('clip %r, %s: an id owns two rows of one frame' % (n, what))
    return bad


def _jsonable(v):
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (np.floating, np.integer)):
        return v.item()
    return v


def _compare(a, b, rel=1e-12):
    """Two results of the same clips: the first field that differs (counts exactly, floats to `rel`), or None."""
    for m, ints in (('HOTA', HOTA_INT), ('CLEAR', CLEAR_INT), ('Identity', ID_INT)):
        for k, v in a[m].items():
            x, y = np.asarray(v, np.float64), np.asarray(b[m][k], np.float64)
            if not (np.array_equal(x, y) if k in ints else np.all(np.abs(x - y) <= rel * np.maximum(np.abs(y), 1e-300))):
                return '%s/%s: %s against %s' % (m, k, x.tolist(), y.tolist())
    return None


# ------------------------------------------------------------------------------------------------ timing
def synthetic_clip(seed, frames, persons, miss=0.05, swap=0.01, extra=0.05):
    """Persons walking at random, tracked with jitter, misses, id swaps and a few false positives -> the arrays of add_clip (boxes)."""
    rs = np.random.RandomState(seed)
    pos = rs.rand(persons, 2) * 1000
    size = 60 + rs.rand(persons, 2) * 80
    track_of = np.arange(persons)
    next_id = persons
    g_box, g_id, g_fr, p_box, p_id, p_fr = [], [], [], [], [], []
    for t in range(frames):
        pos = pos + rs.randn(persons, 2) * 4
        box = np.concatenate([pos, size], 1)
        g_box.append(box); g_id.append(np.arange(persons) * 7 + 3); g_fr.append(np.full(persons, t))
        for i in np.flatnonzero(rs.rand(persons) < swap):
            track_of[i] = next_id
            next_id += 1
        seen = np.flatnonzero(rs.rand(persons) >= miss)
        pb = box[seen] + rs.randn(len(seen), 4) * 3
        n_extra = int(rs.rand() < extra)
        p_box.append(np.concatenate([pb, np.concatenate([rs.rand(n_extra, 2) * 1000, 60 + rs.rand(n_extra, 2) * 80], 1)]))
        p_id.append(np.concatenate([track_of[seen], next_id + np.arange(n_extra)]))
        next_id += n_extra
        p_fr.append(np.full(len(seen) + n_extra, t))
    cat = np.concatenate
    return dict(pred_boxes=cat(p_box).astype(np.float32), pred_ids=cat(p_id), pred_frames=cat(p_fr), gt_boxes=cat(g_box).astype(np.float32),
                gt_ids=cat(g_id), gt_frames=cat(g_fr))


def _bench(persons, clips=16, frames=1000, repeats=3):
    """summary() of `clips` synthetic clips against score_clip_host on the same arrays: wall time from host arrays to the result dict
    on both sides, the device from an idle device to an idle device."""
    import torch
    dev = torch.device('cuda:0')
    data = [synthetic_clip(1000 * persons + i, frames, persons) for i in range(clips)]
    ev = TrackingEvaluator(dev)
    ev.add_clip('warm-up', **synthetic_clip(1, 8, 2))
    ev.summary()
    times = []
    for _ in range(repeats):
        ev.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, c in enumerate(data):
            ev.add_clip('clip%d' % i, **c)
        got = ev.summary()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = {'clip%d' % i: score_clip_host(**c) for i, c in enumerate(data)}
    t_host = time.perf_counter() - t0
    diff = next((d for d in (_compare(got['clips'][n], want[n]) for n in want) if d), None)
    return ('%d clips x %d frames x %d persons (%s, torch %s): device summary() %s ms (each from host arrays to the result), %d launches, '
            '%d bytes downloaded; score_clip_host %.1f ms; device against host: %s'
            % (clips, frames, persons, torch.cuda.get_device_name(0), torch.__version__, ', '.join('%.1f' % (t * 1e3) for t in times),
               ev.last_launches, ev.last_download_bytes, t_host * 1e3, diff or 'counts equal, floats within 1e-12'))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--results', nargs='+')
    ap.add_argument('--gt', nargs='+')
    ap.add_argument('--threshold', type=float, default=0.5)
    ap.add_argument('--max_iou', type=float, default=0.99)
    ap.add_argument('--enlarge', type=float, nargs=2, default=(1.1, 1.18))
    ap.add_argument('--keep_frames_without_gt', action='store_true')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--host', action='store_true', help='score with the host mirror only (no device needed)')
    ap.add_argument('--check', action='store_true', help='validate the files; with a device, compare it with the host mirror')
    ap.add_argument('--bench', action='store_true')
    ap.add_argument('--persons', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    if a.bench:
        text = _bench(a.persons)
        print(text)
        if a.out:
            with open(a.out, 'a') as fh:
                fh.write(text + '\n')
        return 0
    if not a.results or not a.gt:
        ap.error('--results and --gt are needed')
    if not 0. < a.threshold <= 1. or not 0. <= a.max_iou <= 1. or min(a.enlarge) <= 0:
        ap.error('--threshold in (0, 1], --max_iou in [0, 1], --enlarge positive')
    results, gt = {}, {}
    for p in a.results:
        results.update(load_results(p))
    for p in a.gt:
        gt.update(load_results(p))
    bad = validate_files(results, gt)
    if bad:
        print(json.dumps({'ok': False, 'errors': bad}))
        return 1
    args = lambda n: dict(pred_ids=results[n]['ids'], pred_frames=results[n]['frames'], gt_boxes=gt[n]['boxes'], gt_ids=gt[n]['ids'],  # noqa: E731
                          gt_frames=gt[n]['frames'], pred_boxes=results[n].get('boxes'), pred_kp2d=results[n].get('kp2d'))
    skip = not a.keep_frames_without_gt
    host = None
    if a.host or a.check:
        host = {n: score_clip_host(threshold=a.threshold, max_iou=a.max_iou, enlarge_xy=a.enlarge, skip_frames_without_gt=skip, **args(n))
                for n in sorted(results)}
    if a.host:
        ref, comb = combine_clips(host)
        out = {'clips': host, 'reference': ref, 'combined': comb, 'scored_on': 'host'}
    else:
        ev = TrackingEvaluator(a.device, a.threshold, a.max_iou, a.enlarge, skip)
        for n in sorted(results):
            ev.add_clip(n, **args(n))
        out = ev.summary()
        out['scored_on'] = 'device'
        if a.check:
            diff = next((n + ': ' + d for n, d in ((n, _compare(out['clips'][n], host[n])) for n in host) if d), None)
            out['check'] = diff or 'device equals host mirror'
            if diff:
                print(json.dumps(_jsonable(out)))
                return 1
    if a.check:
        out['ok'] = True
    print(json.dumps(_jsonable(out)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
