"""Relative Human scoring (romp_rh_score / romp_rh_accumulate, romp_amd/relative_human.py): the CPU part.
Fixture: tests/golden/relative_human.npz, written by the reference's own RH_Evaluation on synthetic annotations and results
(scripts/make_golden_relative_human.py).  Here: a numpy restatement of the two kernels (`score_np`, `accumulate_np`, and
`summary_np` straight from the rows) behind the restated matcher of tests/test_eval_metrics.py, checked against that fixture
-- matches, misses, every pair count, every correct count and every row's PCKh exactly; PCRD as the same integer ratios to
1e-12; mPCKh within 128 * 2^-24 of the reference's float32 mean over fewer than 128 rows in [-1, 1] -- plus the joint
mappers, the loaders of both file formats, the ABI and the CLI.  tests/test_gpu_relative_human.py holds the kernels to this
restatement."""
import functools
import json
import os
import re

import numpy as np
import pytest

from test_eval_metrics import match2d_np, offsets

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IMAGES, MATCHED = 7, [1, 2, 5, 12, 64, 0, 3]
IMG_BK, IMG_OCH, IMG_FIVE, IMG_TWELVE, IMG_CAP, IMG_ABSENT, IMG_NOIDS = range(7)
N_COUNTS, N_ACC = 20, 24
EQ_P, EQ_C, OR_P, OR_C, AGE_P, AGE_C, MISSED, MISSED_AGE, MATCHED_K, UNSCORED, OVER = 0, 1, 2, 3, 4, 5, 12, 13, 17, 18, 19
ACC_PCKH, ACC_NGT, ACC_NPRED, ACC_FP = 20, 21, 22, 23
AGES = ('adult', 'teen', 'kid', 'baby')


@functools.lru_cache(None)
def golden():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'relative_human.npz'), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def image_names():
    return [bytes(row[row != 0]).decode('ascii') for row in golden()['names']]


def write_reference_files(folder):
    """The fixture's inputs in the reference's own pickled formats -> (results path, annotations path)."""
    g = golden()
    names = image_names()
    annots, results = {n: [] for n in names}, {}
    for b, nj, kp, did, age in zip(g['ann_image'], g['ann_joints'], g['ann_kp'], g['ann_depth_id'], g['ann_age']):
        e = {'bbox': [0, 0, 1, 1], 'depth_id': int(did), 'age': int(age), 'kp2d': None}
        if nj:
            e['kp2d'] = [float(v) for v in kp[:nj].reshape(-1)] if b in g['ann_as_list'] else kp[:nj].copy()
        annots[names[b]].append(e)
    for b in np.unique(g['res_image']):
        rows = g['res_image'] == b
        if b in g['res_stacked']:
            results[names[b]] = {'kp2ds': g['res_kp'][rows], 'trans': g['res_trans'][rows]}
        else:
            results[names[b]] = [{'kp2ds': k, 'trans': t} for k, t in zip(g['res_kp'][rows], g['res_trans'][rows])]
    rp, ap = os.path.join(str(folder), 'ref_results.npz'), os.path.join(str(folder), 'test_annots.npz')
    np.savez(rp, results=results)
    np.savez(ap, annots=annots)
    return rp, ap


@functools.lru_cache(None)
def dataset():
    """The fixture's inputs as flat arrays, built here from the stored rows (NOT through the loaders under test):
    -> results (kp2d, depth, batch_ids), annots (kp2d, valid, depth_id, age, batch_ids, person_index, B)."""
    g = golden()
    names = image_names()
    bk = [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 0, -1]
    och = [3, 0, 4, 1, 5, 2, 9, 6, 10, 7, 11, 8, 12, -1]
    kp, valid, did, age, bid, idx = [], [], [], [], [], []
    seen = {}
    for b, nj, a, d, ag in zip(g['ann_image'], g['ann_joints'], g['ann_kp'], g['ann_depth_id'], g['ann_age']):
        i = seen.get(int(b), 0)
        seen[int(b)] = i + 1
        if not nj:
            continue
        a = a[:nj]
        xy, ok = np.where(a[:, 2:3] == 0, F(-2), a[:, :2]), a[:, 2] > 0
        if nj == 19:
            m = np.array(bk if len(names[b]) - 4 == 7 else och)
            xy, ok = np.where(m[:, None] < 0, F(-2), xy[m]), np.where(m < 0, False, ok[m])
        kp.append(xy); valid.append(ok); did.append(d); age.append(ag); bid.append(b); idx.append(i)
    annots = dict(kp2d=np.asarray(kp, F), valid=np.asarray(valid, bool), depth_id=np.asarray(did, np.int32), age=np.asarray(age, np.int32),
                  batch_ids=np.asarray(bid, np.int64), person_index=np.asarray(idx, np.int32), B=len(names))
    results = dict(kp2d=g['res_kp'], depth=g['res_trans'][:, 2].copy(), batch_ids=g['res_image'].astype(np.int64))
    return results, annots


# ------------------------------------------------------------------------------------------------ restatement
def pckh_row_np(real, pred, thresh=0.143):
    """_calc_matched_PCKh_ for one matched person, (J,2) float32 each -> correct, visible, pckh float32."""
    real, pred = np.asarray(real, F), np.asarray(pred, F)
    vis = (real > F(-1)).all(-1)
    v = int(vis.sum())
    if v < 2:
        return 0, v, F(-1)
    r, d = real[vis], real[vis] - pred[vis]
    w, h = r[:, 0].max() - r[:, 0].min(), r[:, 1].max() - r[:, 1].min()
    scale = np.sqrt(F(w * w + h * h))
    err = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    with np.errstate(all='ignore'):
        c = int((err / scale < F(thresh)).sum())                                # inf and NaN: not correct
    return c, v, F(c) / F(v)


def ratio_gap(pred_kp2d, gt_kp2d, pred_of_gt, thresh):
    """The smallest relative distance of any matched person's error / scale from `thresh`, in float64: how far the inputs keep
    a float32 evaluation of that ratio from a coin toss."""
    gap = np.inf
    for g, p in enumerate(pred_of_gt):
        real, pred = np.asarray(gt_kp2d[g], np.float64), np.asarray(pred_kp2d[max(int(p), 0)], np.float64)
        vis = (real > -1).all(-1)
        if p < 0 or vis.sum() < 2:
            continue
        r = real[vis]
        with np.errstate(all='ignore'):
            q = np.linalg.norm(r - pred[vis], axis=-1) / np.hypot(r[:, 0].max() - r[:, 0].min(), r[:, 1].max() - r[:, 1].min())
        q = q[np.isfinite(q)]
        gap = min(gap, np.abs(q - thresh).min(initial=np.inf) / thresh)
    return gap


def score_np(pred_kp2d, pred_depth, gt_kp2d, gt_depth_id, gt_age, pred_of_gt, goff, dr_thresh=0.2, pck_thresh=0.143, max_gt=64):
    """romp_rh_score -> pckh (Ng,) float32, correct_visible (Ng,2) int32, counts (B,20) int32."""
    Np, Ng, B = len(pred_kp2d), len(gt_kp2d), len(goff) - 1
    pckh, cv, counts = np.full(Ng, np.nan, F), np.zeros((Ng, 2), np.int32), np.zeros((B, N_COUNTS), np.int32)
    thr = F(dr_thresh)
    for b in range(B):
        g0 = min(max(int(goff[b]), 0), Ng)
        g1 = min(max(int(goff[b + 1]), g0), Ng)
        if g1 - g0 > max_gt:
            counts[b, OVER] = 1
            continue
        depth, did, age = [], [], []
        for g in range(g0, g1):
            p = int(pred_of_gt[g])
            if p < 0 or p >= Np:
                counts[b, MISSED] += 1
                if 0 <= gt_age[g] < 4:
                    counts[b, MISSED_AGE + gt_age[g]] += 1
                continue
            c, v, pckh[g] = pckh_row_np(gt_kp2d[g], pred_kp2d[p], pck_thresh)
            cv[g] = c, v
            counts[b, MATCHED_K] += 1
            counts[b, UNSCORED] += v < 2
            if gt_depth_id[g] != -1:
                depth.append(F(pred_depth[p])); did.append(int(gt_depth_id[g])); age.append(int(gt_age[g]))
        if len(depth) < 2:
            continue
        depth, did, age = np.asarray(depth, F), np.asarray(did), np.asarray(age)
        i, j = np.triu_indices(len(depth), 1)
        dist, dd = depth[j] - depth[i], did[j] - did[i]
        ok = np.where(dd == 0, np.abs(dist) < thr, np.where(dd < 0, dist < -thr, dist > thr))
        counts[b, [EQ_P, EQ_C, OR_P, OR_C]] = (dd == 0).sum(), ok[dd == 0].sum(), (dd != 0).sum(), ok[dd != 0].sum()
        for a in range(4):
            m = (age[i] == a) | (age[j] == a)
            counts[b, [AGE_P + 2 * a, AGE_C + 2 * a]] = m.sum(), ok[m].sum()
    return pckh, cv, counts


def accumulate_np(acc, counts, pckh, gt_of_pred):
    """romp_rh_accumulate."""
    acc[:N_COUNTS] += np.asarray(counts, np.float64).reshape(-1, N_COUNTS).sum(0)
    pckh = np.asarray(pckh, F)
    acc[ACC_PCKH] += pckh[pckh >= 0].astype(np.float64).sum()
    acc[ACC_NGT:] += [len(pckh), len(gt_of_pred), (np.asarray(gt_of_pred) < 0).sum()]
    return acc


def restated(results, annots, dr_thresh=0.2, max_pred=64, max_gt=64, pck_thresh=0.143):
    """match -> score over the whole dataset in one call -> gt_of_pred, pred_of_gt, pckh, correct_visible, counts."""
    B = annots['B']
    poff, goff = offsets(results['batch_ids'], B), offsets(annots['batch_ids'], B)
    gop, pog, _ = match2d_np(results['kp2d'], poff, annots['kp2d'], annots['valid'], goff, max_pred=max_pred, max_gt=max_gt)
    pckh, cv, counts = score_np(results['kp2d'], results['depth'], annots['kp2d'], annots['depth_id'], annots['age'], pog, goff, dr_thresh,
                                pck_thresh, max_gt)
    return gop, pog, pckh, cv, counts


def summary_np(pckh, counts, gop, pog, dr_thresh=0.2, miss_fine=0.3):
    """What RelativeHumanEvaluator.summary() reports, straight from the rows of the whole dataset."""
    c = np.asarray(counts, np.int64).sum(0)
    pckh = np.asarray(pckh, np.float64)
    rows = pckh[~np.isnan(pckh)]
    matched, missed, fps = int((np.asarray(pog) >= 0).sum()), int((np.asarray(pog) < 0).sum()), int((np.asarray(gop) < 0).sum())
    nan = float('nan')
    res = {'dr_thresh': dr_thresh, 'miss_fine': miss_fine,
           'PCRD': (c[EQ_C] + c[OR_C]) / (c[EQ_P] + c[OR_P] + miss_fine * missed) if c[EQ_P] + c[OR_P] + missed else nan,
           'PCRD_eq': c[EQ_C] / c[EQ_P] if c[EQ_P] else nan, 'PCRD_ordered': c[OR_C] / c[OR_P] if c[OR_P] else nan}
    for a, name in enumerate(AGES):
        if c[AGE_P + 2 * a]:
            res['PCRD_' + name] = c[AGE_C + 2 * a] / (c[AGE_P + 2 * a] + miss_fine * c[MISSED_AGE + a])
        res.update({'pairs_' + name: int(c[AGE_P + 2 * a]), 'correct_' + name: int(c[AGE_C + 2 * a]), 'missed_' + name: int(c[MISSED_AGE + a])})
    res['mPCKh'] = float(rows.mean()) if len(rows) else nan
    res['mPCKh_scored'] = float(rows[rows >= 0].mean()) if (rows >= 0).any() else nan
    prec, rec = matched / max(matched + fps, 1), matched / max(len(pog), 1)
    tp = len(gop) - missed
    res.update(precision=prec, recall=rec, F1=2 * prec * rec / (prec + rec) if prec + rec else nan,
               reference_prf1=[round(tp / (tp + fps), 2), round(tp / (tp + missed), 2), round(tp / (tp + 0.5 * (fps + missed)), 2)] if len(gop) else [0, 0, 0],
               pairs_eq=int(c[EQ_P]), correct_eq=int(c[EQ_C]), pairs_ordered=int(c[OR_P]), correct_ordered=int(c[OR_C]), matched=matched,
               misses=missed, unscored=int((rows == -1).sum()), false_positives=fps, n_gt=len(pog), n_pred=len(gop))
    return res


def assert_summaries_equal(got, want, rtol=1e-12):
    assert set(got) == set(want), set(got) ^ set(want)
    for k, v in want.items():
        if isinstance(v, (int, np.integer)) or k == 'reference_prf1':
            assert got[k] == v, (k, got[k], v)
        elif v != v:
            assert got[k] != got[k], (k, got[k])
        else:
            assert abs(got[k] - v) <= rtol * abs(v), (k, got[k], v)


# ------------------------------------------------------------------------------------------------ against the reference
def test_restatement_equals_the_reference_on_every_image():
    g = golden()
    results, annots = dataset()
    gop, pog, pckh, cv, counts = restated(results, annots)
    B = annots['B']
    poff, goff = offsets(results['batch_ids'], B), offsets(annots['batch_ids'], B)
    assert B == N_IMAGES
    for b in range(B):
        g0, g1, p0 = goff[b], goff[b + 1], poff[b]
        person = annots['person_index'][g0:g1]
        rows = [q for q in range(g0, g1) if pog[q] >= 0]
        ours = {(int(pog[q] - p0), int(person[q - g0])): q for q in rows}
        assert sorted(person[pog[g0:g1] < 0].tolist()) == sorted(g[f'missed_{b}'].tolist()), b
        assert (g[f'pr_all'][b], g['pr_fp'][b], g['pr_miss'][b]) == (poff[b + 1] - p0, (gop[p0:poff[b + 1]] < 0).sum(), (pog[g0:g1] < 0).sum()), b
        assert counts[b, MISSED] == g['pr_miss'][b] and counts[b, MATCHED_K] == len(rows) == MATCHED[b]
        if f'match_{b}' not in g:
            assert not rows and b == IMG_ABSENT
            continue
        assert sorted(ours) == sorted(map(tuple, g[f'match_{b}'].tolist())), b
        for pair, ref in zip(map(tuple, g[f'match_{b}'].tolist()), g[f'pckh_{b}']):      # every row, bit for bit
            q = ours[pair]
            assert pckh[q].tobytes() == ref.tobytes(), (b, pair, pckh[q], ref)
            c, v = cv[q]
            assert v == (annots['kp2d'][q] > -1).all(-1).sum() and (ref == -1 if v < 2 else F(c) / F(v) == ref)
    assert np.isnan(pckh[pog < 0]).all() and not cv[pog < 0].any()


def reference_counts(thr=F(0.2)):
    """The counts of get_results (:101-123) from the pair lists the reference handed to it."""
    g = golden()
    eq, cd, fd = g['eq_dist'], g['cd_dist'], g['fd_dist']
    assert eq.dtype == cd.dtype == fd.dtype == F
    ok = np.concatenate([np.abs(eq) < thr, cd < -thr, fd > thr])
    ages = np.concatenate([g['eq_age'], g['cd_age'], g['fd_age']])
    per_age = [((ages == a).any(-1).sum(), ok[(ages == a).any(-1)].sum(), (g['missed_age'] == a).sum()) for a in range(4)]
    return len(eq), (np.abs(eq) < thr).sum(), len(cd) + len(fd), (cd < -thr).sum() + (fd > thr).sum(), per_age, len(g['missed_age'])


def test_pair_counts_and_pcrd_equal_the_reference():
    g = golden()
    results, annots = dataset()
    gop, pog, pckh, cv, counts = restated(results, annots)
    c = counts.astype(np.int64).sum(0)
    eq_p, eq_c, or_p, or_c, per_age, missed = reference_counts()
    assert (c[EQ_P], c[EQ_C], c[OR_P], c[OR_C], c[MISSED]) == (eq_p, eq_c, or_p, or_c, missed)
    assert [(c[AGE_P + 2 * a], c[AGE_C + 2 * a], c[MISSED_AGE + a]) for a in range(4)] == per_age
    assert (counts[:, EQ_P] + counts[:, OR_P]).tolist() == [0, 1, 6, 66, 2016, 0, 0]        # n (n - 1) / 2 of 1, 2, 4, 12, 64, 0, 0 ids
    s = summary_np(pckh, counts, gop, pog)
    want = (eq_c + or_c) / (eq_p + or_p + 0.3 * missed)
    assert abs(s['PCRD'] - want) <= 1e-12 * want
    assert abs(s['PCRD'] - float(g['PCRD'])) <= 2.0 ** -22 * want               # the reference's own float32 quotient: 3 roundings
    assert abs(s['PCRD'] * 100 - g['printed'][1]) < 0.0051
    for a, name in enumerate(AGES):
        pairs, ok, gone = per_age[a]
        assert pairs > 0 and not np.isnan(g['PCRD_age'][a])                      # every age has pairs in this fixture
        want = ok / (pairs + 0.3 * gone)
        assert abs(s['PCRD_' + name] - want) <= 1e-12 * want
        assert abs(s['PCRD_' + name] - float(g['PCRD_age'][a])) <= 2.0 ** -22 * want
        assert abs(s['PCRD_' + name] * 100 - g['printed'][2 + a]) < 0.0051
    assert abs(s['PCRD_eq'] * 100 - g['printed_eq_cd_fd'][0]) < 0.0051
    cd_ok, fd_ok = (g['cd_dist'] < -F(0.2)).sum(), (g['fd_dist'] > F(0.2)).sum()
    assert abs(cd_ok / len(g['cd_dist']) * 100 - g['printed_eq_cd_fd'][1]) < 0.0051 and abs(fd_ok / len(g['fd_dist']) * 100 - g['printed_eq_cd_fd'][2]) < 0.0051
    assert s['correct_ordered'] == cd_ok + fd_ok                                 # close + far together: independent of the pair order
    # mPCKh: the reference's float32 mean of < 128 rows in [-1, 1]
    assert (~np.isnan(pckh)).sum() == sum(MATCHED) < 128
    assert abs(s['mPCKh'] - float(g['mPCKh'])) <= 128 * 2.0 ** -24
    assert abs(s['mPCKh'] * 100 - g['printed'][0]) < 0.0051 + 128 * 2.0 ** -24 * 100
    assert s['unscored'] == 1 and s['mPCKh_scored'] > s['mPCKh']
    assert s['reference_prf1'] == g['prf1'].tolist()
    assert (s['n_pred'], s['n_gt'], s['matched'], s['misses'], s['false_positives']) == (88, 91, 87, 4, 1)


def test_fixture_holds_the_cases_it_was_made_for():
    g = golden()
    results, annots = dataset()
    gop, pog, pckh, cv, counts = restated(results, annots)
    goff = offsets(annots['batch_ids'], annots['B'])
    names = image_names()
    assert len(names[IMG_BK]) - 4 == 7 and len(names[IMG_OCH]) - 4 != 7
    nj = [sorted(set(g['ann_joints'][g['ann_image'] == b].tolist())) for b in range(N_IMAGES)]
    assert nj[IMG_BK] == [19] and nj[IMG_OCH] == [19] and nj[IMG_TWELVE] == [0, 14] and nj[IMG_CAP] == [14]
    assert g['ann_as_list'].tolist() == [IMG_FIVE] and g['res_stacked'].tolist() == [IMG_CAP]
    assert IMG_ABSENT not in g['res_image'] and g['pr_all'][IMG_ABSENT] == 0 and g['pr_miss'][IMG_ABSENT] == 3
    assert float(g['min_gap']) >= 1e-4 and abs(ratio_gap(results['kp2d'], annots['kp2d'], pog, 0.143) - float(g['min_gap'])) < 1e-9
    did = lambda b: annots['depth_id'][goff[b]:goff[b + 1]]
    assert (did(IMG_NOIDS) == -1).all() and did(IMG_BK).tolist() == [2] and did(IMG_OCH).tolist() == [1, 1]
    assert (did(IMG_TWELVE) != -1).all() and (did(IMG_CAP) != -1).all() and (did(IMG_FIVE) == -1).sum() == 1
    assert set(annots['age'].tolist()) == {-1, 0, 1, 2, 3} and set(g['missed_age'].tolist()) == {-1, 0, 2, 3}
    # the threshold is a float32: |0.2f - 0| is not < 0.2f (it is < the double 0.2), one ulp less is, one ulp more is an ordered hit
    thr = F(0.2)
    assert float(thr) > 0.2
    assert counts[IMG_OCH, [EQ_P, EQ_C]].tolist() == [1, 0] and np.abs(g['eq_dist'][0]) == thr
    p = pog[goff[IMG_FIVE]:goff[IMG_FIVE] + 4]
    assert results['depth'][p].tobytes() == np.array([0, thr, np.nextafter(thr, F(1)), np.nextafter(thr, F(0))], F).tobytes()
    # ids 0, 1, 1, 0: (0,3) equal and within thr; (1,2) equal, 1 ulp apart; (0,1) ordered, exactly thr: not beyond;
    # (0,2) ordered, thr + 1 ulp: beyond; (1,3), (2,3): id falls, depth falls by 1 or 2 ulp only
    assert counts[IMG_FIVE, [EQ_P, EQ_C, OR_P, OR_C]].tolist() == [2, 2, 4, 1]
    # PCKh edge rows
    g0 = goff[IMG_TWELVE]
    assert cv[g0].tolist() == [0, 1] and pckh[g0] == -1 and annots['valid'][g0].sum() == 1            # one valid joint
    assert annots['valid'][g0 + 1].all() and (annots['kp2d'][g0 + 1][:, 0] <= -1).sum() == 2 and cv[g0 + 1, 1] == 12   # valid at x <= -1
    assert sorted(annots['kp2d'][g0 + 1][[4, 8], 0].tolist()) == [-5.0, -1.0]
    q = goff[IMG_FIVE] + 3                                                       # coinciding visible joints: scale 0, nothing correct
    assert cv[q].tolist() == [0, 3] and pckh[q] == 0 and len(np.unique(annots['kp2d'][q][annots['valid'][q]], axis=0)) == 1
    assert (results['kp2d'][pog[q], 6] == annots['kp2d'][q, 6]).all()            # 0 / 0 among them
    assert counts[IMG_FIVE, [MISSED, MISSED_AGE + 2]].tolist() == [1, 1] and (gop < 0).sum() == 1
    assert np.abs(results['kp2d'][gop < 0]).min() > 2500                         # the far-away false positive


# ------------------------------------------------------------------------------------------------ mappers, loaders
def test_joint_mappers_equal_the_check_values():
    from romp_amd import relative_human as R
    assert R.CROWDPOSE14_FROM_SMPL54 == [16, 17, 18, 19, 20, 21, 46, 45, 4, 5, 7, 8, 48, 47]
    assert R.BK19_TO_CROWDPOSE14 == [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 0, -1]
    assert R.OCHUMAN19_TO_CROWDPOSE14 == [3, 0, 4, 1, 5, 2, 9, 6, 10, 7, 11, 8, 12, -1]
    assert R.AGES == AGES and len(R.SMPL_54) == 54 and len(set(R.SMPL_54)) == 54 and len(R.BK_19) == len(R.OCHUMAN_19) == 19
    assert R.joint_mapping(R.CROWDPOSE_14, R.CROWDPOSE_14) == list(range(14))


def test_loaders_round_trip_both_file_formats(tmp_path):
    from romp_amd import relative_human as R
    rp, ap = write_reference_files(tmp_path)
    want_r, want_a = dataset()
    annots = R.load_rh_annots(ap)
    results = R.load_rh_results(rp, annots['image_names'])
    assert annots['image_names'].tolist() == image_names() and annots['B'] == N_IMAGES
    for k, v in want_a.items():
        assert np.array_equal(annots[k], v) and (k == 'B' or annots[k].dtype == v.dtype), k
    for k, v in want_r.items():
        assert np.array_equal(results[k], v) and results[k].dtype == v.dtype, k
    assert (annots['kp2d'][~annots['valid']] == -2).all()
    # the flat format
    fr, fa = str(tmp_path / 'r.npz'), str(tmp_path / 'a.npz')
    R.save_results(fr, **results)
    R.save_results(fa, **annots)
    with np.load(fa, allow_pickle=False) as z:                                   # no pickle inside
        assert set(z.files) == set(annots)
    got_r, got_a = R.load_files(fr, fa)
    for got, want in ((got_r, results), (got_a, annots)):
        assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
    mixed_r, mixed_a = R.load_files(rp, ap)                                      # told apart by the array names
    assert all(np.array_equal(mixed_r[k], results[k]) for k in results) and all(np.array_equal(mixed_a[k], annots[k]) for k in annots)
    R.save_results(fr, kp2d=results['kp2d'], depth=results['depth'], batch_ids=results['batch_ids'][::-1])
    with pytest.raises(ValueError, match='ascend'):
        R.load_results(fr)
    R.save_results(fr, kp2d=results['kp2d'], depth=results['depth'][:-1], batch_ids=results['batch_ids'])
    with pytest.raises(ValueError, match='depth'):
        R.load_results(fr)
    with pytest.raises(ValueError, match='14 or 19'):
        R.crowdpose14_of_annotation(np.ones((17, 3)), 'x.jpg')
    # a person without a single valid joint is dropped, and the persons after it keep their own index
    extra = str(tmp_path / 'extra_annots.npz')
    person = lambda flag: {'bbox': [0, 0, 1, 1], 'depth_id': 1, 'age': 0, 'kp2d': np.concatenate([np.full((14, 2), 50.0), np.full((14, 1), flag)], 1)}
    np.savez(extra, annots={'a.jpg': [person(1.0), person(0.0), person(1.0)]})
    assert R.load_rh_annots(extra)['person_index'].tolist() == [0, 2]


def test_cli_check_validates_without_a_gpu(tmp_path, capsys):
    from romp_amd import relative_human as R
    rp, ap = write_reference_files(tmp_path)
    res = R.main(['--results', rp, '--annots', ap, '--check'])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    assert res['results']['kp2d'] == [88, 14, 2] and res['annots']['kp2d'] == [91, 14, 2] and res['annots']['valid'] == [91, 14]
    results, annots = R.load_files(rp, ap)
    fr, fa = str(tmp_path / 'r.npz'), str(tmp_path / 'a.npz')
    R.save_results(fr, **results)
    R.save_results(fa, **annots)
    assert R.main(['--results', fr, '--annots', fa, '--check']) == res
    R.save_results(fr, kp2d=results['kp2d'][:, :13], depth=results['depth'], batch_ids=results['batch_ids'])
    with pytest.raises(ValueError, match='per person'):
        R.main(['--results', fr, '--annots', fa, '--check'])
    R.save_results(fr, kp2d=results['kp2d'], depth=results['depth'], batch_ids=results['batch_ids'] + 1)
    with pytest.raises(ValueError, match='image'):
        R.main(['--results', fr, '--annots', fa, '--check'])


# ------------------------------------------------------------------------------------------------ summary, ABI
def test_summary_arithmetic_from_a_hand_made_accumulator():
    from romp_amd import relative_human as R
    acc = np.zeros(N_ACC)
    acc[[EQ_P, EQ_C, OR_P, OR_C]] = 10, 4, 30, 21
    acc[AGE_P:AGE_P + 8] = 12, 6, 0, 0, 8, 8, 25, 5                              # no teen pairs
    acc[MISSED:MISSED + 5] = 5, 2, 1, 0, 1                                       # (one missed person without an age)
    acc[[MATCHED_K, UNSCORED]] = 20, 2
    acc[ACC_PCKH:] = 13.5, 25, 23, 3
    s = R.summarize(acc, 0.2, 0.3)
    assert s['PCRD'] == 25 / (40 + 0.3 * 5) and s['PCRD_eq'] == 0.4 and s['PCRD_ordered'] == 0.7
    assert s['PCRD_adult'] == 6 / (12 + 0.3 * 2) and 'PCRD_teen' not in s and s['PCRD_kid'] == 8 / 8.0 and s['PCRD_baby'] == 5 / (25 + 0.3)
    assert s['pairs_teen'] == 0 and s['missed_teen'] == 1
    assert s['mPCKh'] == (13.5 - 2) / 20 and s['mPCKh_scored'] == 13.5 / 18
    assert s['precision'] == 20 / 23 and s['recall'] == 20 / 25 and abs(s['F1'] - 2 * 20 / (23 + 25)) < 1e-15
    assert s['reference_prf1'] == [round(18 / 21, 2), round(18 / 23, 2), round(18 / 22, 2)]         # tp = n_pred - misses = 18
    assert s['reference_prf1'] == list(R.reference_prf1(23, 5, 3)) and R.reference_prf1(0, 4, 0) == [0, 0, 0]
    assert (s['matched'], s['misses'], s['false_positives'], s['n_gt'], s['n_pred'], s['unscored']) == (20, 5, 3, 25, 23, 2)
    assert R.summarize(acc, 0.2, 0.5)['PCRD'] == 25 / 42.5
    empty = R.summarize(np.zeros(N_ACC))
    assert all(np.isnan(empty[k]) for k in ('PCRD', 'PCRD_eq', 'PCRD_ordered', 'mPCKh', 'mPCKh_scored', 'precision', 'recall', 'F1'))
    acc[OVER] = 1
    with pytest.raises(Exception, match='max_pred'):
        R.summarize(acc)
    # and the restated accumulator and summary agree with it on the fixture, cut into two calls
    results, annots = dataset()
    gop, pog, pckh, cv, counts = restated(results, annots)
    goff, poff = offsets(annots['batch_ids'], 7), offsets(results['batch_ids'], 7)
    acc = np.zeros(N_ACC)
    for b0, b1 in ((0, 3), (3, 7)):
        accumulate_np(acc, counts[b0:b1], pckh[goff[b0]:goff[b1]], gop[poff[b0]:poff[b1]])
    assert_summaries_equal(R.summarize(acc), summary_np(pckh, counts, gop, pog))


def test_rh_symbols_header_binding_and_library_agree():
    from romp_amd import build, lib
    from romp_amd import relative_human as R
    assert lib.RH_EXPORTS == ['romp_rh_score', 'romp_rh_accumulate']
    others = set(lib.EXPORTS) | set(lib.VIEW_EXPORTS) | set(lib.MAP_EXPORTS) | set(lib.TEXTURE_EXPORTS) | set(lib.EVAL_EXPORTS)
    assert not set(lib.RH_EXPORTS) & others
    assert len(lib.EXPORTS) == 52 and 'rh.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'rh.hip'))
    header = open(os.path.join(ROOT, 'include', 'romp_hip_rh.h')).read()
    declared = re.findall(r'^int\s+(romp_\w+)\(', header, re.M)
    assert declared == lib.RH_EXPORTS
    h = lib.load()
    assert all(hasattr(h, n) and getattr(h, n).argtypes is not None for n in lib.RH_EXPORTS) and h.romp_abi_version() == 7
    for name in declared:                                                        # as many arguments as the header declares
        args = re.search(name + r'\((.*?)\);', header, re.S).group(1)
        assert len(getattr(h, name).argtypes) == len(args.split(',')), name
    defines = {k: int(v) for k, v in re.findall(r'#define ROMP_RH_(\w+)\s+(\d+)', header)}
    assert defines == {'EQ_PAIRS': R.RH_EQ_PAIRS, 'EQ_CORRECT': R.RH_EQ_CORRECT, 'ORD_PAIRS': R.RH_ORD_PAIRS, 'ORD_CORRECT': R.RH_ORD_CORRECT,
                       'AGE_PAIRS': R.RH_AGE_PAIRS, 'AGE_CORRECT': R.RH_AGE_CORRECT, 'MISSED': R.RH_MISSED, 'MISSED_AGE': R.RH_MISSED_AGE,
                       'MATCHED': R.RH_MATCHED, 'UNSCORED': R.RH_UNSCORED, 'OVER_CAP': R.RH_OVER_CAP, 'COUNTS': R.RH_COUNTS,
                       'ACC_PCKH_SUM': R.RH_ACC_PCKH_SUM, 'ACC_N_GT': R.RH_ACC_N_GT, 'ACC_N_PRED': R.RH_ACC_N_PRED,
                       'ACC_FALSE_POS': R.RH_ACC_FALSE_POS, 'ACC': R.RH_ACC}
    assert (R.RH_COUNTS, R.RH_ACC) == (N_COUNTS, N_ACC)
    assert (EQ_P, EQ_C, OR_P, OR_C, AGE_P, AGE_C, MISSED, MISSED_AGE, MATCHED_K, UNSCORED, OVER, ACC_PCKH, ACC_NGT, ACC_NPRED, ACC_FP) == \
        (R.RH_EQ_PAIRS, R.RH_EQ_CORRECT, R.RH_ORD_PAIRS, R.RH_ORD_CORRECT, R.RH_AGE_PAIRS, R.RH_AGE_CORRECT, R.RH_MISSED, R.RH_MISSED_AGE,
         R.RH_MATCHED, R.RH_UNSCORED, R.RH_OVER_CAP, R.RH_ACC_PCKH_SUM, R.RH_ACC_N_GT, R.RH_ACC_N_PRED, R.RH_ACC_FALSE_POS)
