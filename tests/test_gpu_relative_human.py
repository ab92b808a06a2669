"""Relative Human scoring on the GPU: romp_rh_score / romp_rh_accumulate through the C ABI and through
romp_amd/relative_human.py, against the numpy restatement of tests/test_relative_human.py (itself held to the reference's
answers in tests/golden/relative_human.npz).  Bars: every integer output EXACT; pckh bit-equal to float32(correct) /
float32(visible), -1 below two visible joints, NaN for a miss (the fixture keeps every error / scale 2e-3 relative away from
the threshold, four orders above a float32 rounding); two launches byte-identical; accumulators of differently cut
datasets identical; summary ratios within 1e-12 of the restatement's."""
import json

import numpy as np
import pytest
import torch

from test_eval_metrics import match2d_np, offsets
from test_relative_human import (ACC_FP, ACC_NGT, ACC_NPRED, ACC_PCKH, EQ_P, IMG_ABSENT, IMG_CAP, IMG_FIVE, IMG_TWELVE, MATCHED_K, MISSED, N_ACC,
                                 N_COUNTS, OR_P, OVER, accumulate_np, assert_summaries_equal, dataset, ratio_gap, restated, score_np, summary_np,
                                 write_reference_files)

pytestmark = pytest.mark.gpu
F = np.float32
SENT_I, SENT_F, PAD = -77777, -12345.5, 5
ROMP_EINVAL = -1
J = 14


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def whole():
    """The fixture dataset and its restated answer, computed once."""
    results, annots = dataset()
    return results, annots, restated(results, annots)


def t_(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def abi_score(dev, pred_kp, depth, gt_kp, did, age, pog, goff, max_gt=64, dr=0.2, pck=0.143, expect=0, null=(), B=None, Jn=J, raw=False,
              Np=None, Ng=None):
    """romp_rh_score into buffers PAD rows longer than needed, filled with a sentinel -> pckh, correct_visible, counts (numpy),
    or the status code when `expect` is one; asserts that the rows past the end (or, for a refused call, all) hold the sentinel."""
    from romp_amd import lib as L
    B = len(goff) - 1 if B is None else B
    Np, Ng = len(pred_kp) if Np is None else Np, len(gt_kp) if Ng is None else Ng
    nb = max(len(goff) - 1, 0)
    pckh = torch.full((len(gt_kp) + PAD,), SENT_F, dtype=torch.float32, device=dev)
    cv = torch.full(((len(gt_kp) + PAD) * 2,), SENT_I, dtype=torch.int32, device=dev)
    counts = torch.full(((nb + PAD) * N_COUNTS,), SENT_I, dtype=torch.int32, device=dev)
    a = {'pred_kp': t_(np.asarray(pred_kp, F), dev), 'depth': t_(np.asarray(depth, F), dev), 'gt_kp': t_(np.asarray(gt_kp, F), dev),
         'did': t_(np.asarray(did, np.int32), dev), 'age': t_(np.asarray(age, np.int32), dev), 'pog': t_(np.asarray(pog, np.int32), dev),
         'goff': t_(np.asarray(goff, np.int32), dev), 'pckh': pckh, 'cv': cv, 'counts': counts}
    p = {k: L.ptr(None if k in null else v) for k, v in a.items()}
    rc = L.load().romp_rh_score(p['pred_kp'], p['depth'], Np, p['gt_kp'], p['did'], p['age'], p['pog'], Ng, p['goff'], B, Jn, max_gt, dr, pck,
                                p['pckh'], p['cv'], p['counts'], L.stream_ptr(dev))
    torch.cuda.current_stream(dev).synchronize()
    if expect:
        assert rc == expect and L.load().romp_last_error()
        assert (pckh == SENT_F).all() and (cv == SENT_I).all() and (counts == SENT_I).all()          # nothing was written
        return rc
    assert rc == 0, L.load().romp_last_error()
    pckh, cv, counts = pckh.cpu().numpy(), cv.cpu().numpy(), counts.cpu().numpy()
    assert (pckh[Ng:] == F(SENT_F)).all() and (cv[2 * Ng:] == SENT_I).all() and (counts[B * N_COUNTS:] == SENT_I).all()
    if raw:
        return pckh[:Ng].copy(), cv[:2 * Ng].copy(), counts[:B * N_COUNTS].copy()
    return pckh[:Ng], cv[:2 * Ng].reshape(Ng, 2), counts[:B * N_COUNTS].reshape(B, N_COUNTS)


def subset(results, annots, pog, images):
    """The given images (an index, or None for an image without anybody) as one call -> the arguments of abi_score / score_np."""
    B = annots['B']
    poff, goff = offsets(results['batch_ids'], B), offsets(annots['batch_ids'], B)
    pk, dp, gk, did, age, pg, off = [], [], [], [], [], [], [0]
    n_pred = 0
    for b in images:
        if b is not None:
            p0, p1, g0, g1 = poff[b], poff[b + 1], goff[b], goff[b + 1]
            pk.append(results['kp2d'][p0:p1]); dp.append(results['depth'][p0:p1]); gk.append(annots['kp2d'][g0:g1])
            did.append(annots['depth_id'][g0:g1]); age.append(annots['age'][g0:g1])
            pg.append(np.where(pog[g0:g1] < 0, -1, pog[g0:g1] - p0 + n_pred))
            n_pred += p1 - p0
            off.append(off[-1] + g1 - g0)
        else:
            off.append(off[-1])
    cat = lambda xs, shape, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt)
    return (cat(pk, (0, J, 2), F), cat(dp, (0,), F), cat(gk, (0, J, 2), F), cat(did, (0,), np.int32), cat(age, (0,), np.int32),
            cat(pg, (0,), np.int32), np.asarray(off, np.int32))


def assert_rows_equal(got, want):
    pckh, cv, counts = got
    assert pckh.dtype == F and pckh.tobytes() == want[0].tobytes()                # bit for bit, NaN included
    assert np.array_equal(cv, want[1]) and np.array_equal(counts, want[2])
    scored = cv[:, 1] >= 2
    assert (pckh[scored] == cv[scored, 0].astype(F) / cv[scored, 1].astype(F)).all()


# ------------------------------------------------------------------------------------------------ the score kernel
def test_score_every_fixture_image_in_one_launch_and_alone(dev, whole):
    results, annots, (gop, pog, pckh, cv, counts) = whole
    args = subset(results, annots, pog, range(annots['B']))
    got = abi_score(dev, *args)
    assert_rows_equal(got, (pckh, cv, counts))
    assert np.isnan(got[0][pog < 0]).all() and (got[0][got[1][:, 1] < 2][pog[got[1][:, 1] < 2] >= 0] == -1).all()
    assert (got[2][:, EQ_P] + got[2][:, OR_P]).tolist() == [0, 1, 6, 66, 2016, 0, 0] and not got[2][:, OVER].any()
    first, again = abi_score(dev, *args, raw=True), abi_score(dev, *args, raw=True)      # two launches: the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    for b in range(annots['B']):
        one = subset(results, annots, pog, [b])
        got = abi_score(dev, *one)
        assert_rows_equal(got, score_np(*one))
        assert np.array_equal(got[2][0], counts[b]), b
    # the Python layer, the device's own matches
    from romp_amd import evaluation as E
    from romp_amd import relative_human as R
    a, b = E.match_2d_greedy(t_(results['kp2d'], dev), t_(results['batch_ids'], dev), t_(annots['kp2d'], dev), t_(annots['valid'], dev),
                             t_(annots['batch_ids'], dev), annots['B'], max_gt=64)
    assert np.array_equal(a.cpu().numpy(), gop) and np.array_equal(b.cpu().numpy(), pog)
    rows = R.score_rows(t_(results['kp2d'], dev), t_(results['depth'], dev), t_(annots['kp2d'], dev), t_(annots['depth_id'], dev),
                        t_(annots['age'], dev), b, t_(args[6], dev), annots['B'])
    assert_rows_equal([r.cpu().numpy() for r in rows], (pckh, cv, counts))
    assert rows[0].dtype == torch.float32 and rows[1].dtype == rows[2].dtype == torch.int32


def test_score_other_thresholds(dev, whole):
    results, annots, (gop, pog, *_) = whole
    args = subset(results, annots, pog, range(annots['B']))
    seen = set()
    for dr, pck in ((0.5, 0.143), (0.2, 0.05), (1e-3, 0.5)):
        assert ratio_gap(results['kp2d'], annots['kp2d'], pog, pck) >= 1e-4       # (as the fixture guarantees for 0.143)
        got = abi_score(dev, *args, dr=dr, pck=pck)
        assert_rows_equal(got, score_np(*args, dr_thresh=dr, pck_thresh=pck))
        seen.add(got[2].astype(np.int64).sum(0).tobytes() + got[1].tobytes())
    assert len(seen) == 3                                                         # the thresholds do reach the counts


def test_score_empty_sides(dev, whole):
    results, annots, (gop, pog, *_) = whole
    # empty images between full ones, at the start and at the end
    args = subset(results, annots, pog, [None, IMG_FIVE, None, None, IMG_TWELVE, None])
    got = abi_score(dev, *args)
    assert_rows_equal(got, score_np(*args))
    assert not got[2][[0, 2, 3, 5]].any() and got[2][1, MATCHED_K] == 5 and got[2][4, MATCHED_K] == 12
    # no predictions at all: every person is a miss, no pair
    pk, dp, gk, did, age, pg, off = subset(results, annots, pog, [IMG_FIVE, IMG_TWELVE])
    none = (np.zeros((0, J, 2), F), np.zeros(0, F), gk, did, age, np.full(len(gk), -1, np.int32), off)
    got = abi_score(dev, *none, null=('pred_kp', 'depth'))
    assert_rows_equal(got, score_np(*none))
    assert got[2][:, MISSED].tolist() == [6, 12] and np.isnan(got[0]).all() and not got[2][:, :MISSED].any()
    # a prediction row past the end is a miss, not a read
    far = (pk, dp, gk, did, age, np.where(pg == 3, len(pk) + 7, pg).astype(np.int32), off)
    assert_rows_equal(abi_score(dev, *far), score_np(*far))
    # no ground truth: B rows of zeros, nothing else
    empty = (pk, dp, np.zeros((0, J, 2), F), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(4, np.int32))
    got = abi_score(dev, *empty, null=('gt_kp', 'did', 'age', 'pog'))
    assert got[2].shape == (3, N_COUNTS) and not got[2].any() and got[0].size == 0
    # offsets beyond the rows are clamped, never followed
    wild = (pk, dp, gk, did, age, pg, np.array([0, 6, 4000], np.int32))
    assert_rows_equal(abi_score(dev, *wild), score_np(*wild))
    # the outputs per row are optional
    only = abi_score(dev, *args, null=('pckh', 'cv'), raw=True)
    assert (only[0] == F(SENT_F)).all() and (only[1] == SENT_I).all() and np.array_equal(only[2].reshape(-1, N_COUNTS), score_np(*args)[2])


def test_score_over_the_cap_is_flagged_and_contributes_nothing(dev, whole):
    results, annots, (gop, pog, pckh, cv, counts) = whole
    args = subset(results, annots, pog, range(annots['B']))
    got = abi_score(dev, *args, max_gt=63)
    want = score_np(*args, max_gt=63)
    assert_rows_equal(got, want)
    assert got[2][:, OVER].tolist() == [0, 0, 0, 0, 1, 0, 0] and not got[2][IMG_CAP, :OVER].any()
    g0, g1 = args[6][IMG_CAP], args[6][IMG_CAP + 1]
    assert np.isnan(got[0][g0:g1]).all() and not got[1][g0:g1].any()
    keep = np.r_[0:g0, g1:len(pog)]
    assert got[0][keep].tobytes() == pckh[keep].tobytes() and np.array_equal(np.delete(got[2], IMG_CAP, 0), np.delete(counts, IMG_CAP, 0))
    assert_rows_equal(abi_score(dev, *args, max_gt=4096), (pckh, cv, counts))     # the largest cap


def test_score_invalid_arguments_write_nothing(dev, whole):
    results, annots, (gop, pog, *_) = whole
    args = subset(results, annots, pog, [IMG_FIVE, IMG_TWELVE])
    for kw in ({'B': 0}, {'B': -1}, {'Jn': 0}, {'max_gt': 0}, {'max_gt': 4097}, {'Np': -1}, {'Ng': -1}, {'null': ('counts',)}, {'null': ('goff',)},
               {'null': ('gt_kp',)}, {'null': ('did',)}, {'null': ('age',)}, {'null': ('pog',)}, {'null': ('pred_kp',)}, {'null': ('depth',)}):
        assert abi_score(dev, *args, expect=ROMP_EINVAL, **kw) == ROMP_EINVAL, kw
    from romp_amd import relative_human as R
    with pytest.raises(Exception, match='max_gt'):
        R.score_rows(t_(args[0], dev), t_(args[1], dev), t_(args[2], dev), t_(args[3], dev), t_(args[4], dev), t_(args[5], dev), t_(args[6], dev), 2,
                     max_gt=5000)


# ------------------------------------------------------------------------------------------------ the accumulator
def abi_accumulate(dev, acc, counts, pckh, gop, expect=0, null=(), **kw):
    from romp_amd import lib as L
    buf = torch.full((N_ACC + PAD,), SENT_F, dtype=torch.float64, device=dev)
    buf[:N_ACC] = t_(np.asarray(acc, np.float64), dev)
    a = {'counts': t_(np.asarray(counts, np.int32), dev), 'pckh': t_(np.asarray(pckh, F), dev), 'gop': t_(np.asarray(gop, np.int32), dev), 'acc': buf}
    p = {k: L.ptr(None if k in null else v) for k, v in a.items()}
    rc = L.load().romp_rh_accumulate(p['counts'], kw.get('B', len(counts)), p['pckh'], kw.get('Ng', len(pckh)), p['gop'], kw.get('Np', len(gop)),
                                     p['acc'], L.stream_ptr(dev))
    torch.cuda.current_stream(dev).synchronize()
    out = buf.cpu().numpy()
    assert (out[N_ACC:] == SENT_F).all()
    if expect:
        assert rc == expect and L.load().romp_last_error() and np.array_equal(out[:N_ACC], np.asarray(acc, np.float64))
        return rc
    assert rc == 0, L.load().romp_last_error()
    return out[:N_ACC]


def test_accumulate_folds_calls_exactly(dev, whole):
    results, annots, (gop, pog, pckh, cv, counts) = whole
    poff, goff = offsets(results['batch_ids'], 7), offsets(annots['batch_ids'], 7)
    want = accumulate_np(np.zeros(N_ACC), counts, pckh, gop)
    one = abi_accumulate(dev, np.zeros(N_ACC), counts, pckh, gop)
    assert one.tobytes() == want.tobytes()
    assert (one[ACC_NGT], one[ACC_NPRED], one[ACC_FP], one[MATCHED_K], one[MISSED]) == (91, 88, 1, 87, 4)
    assert one[ACC_PCKH] == pckh[pckh >= 0].astype(np.float64).sum()
    acc = np.zeros(N_ACC)
    for b0, b1 in ((0, 3), (3, 4), (4, 5), (5, 6), (6, 7)):                       # (5, 6): the image without predictions
        acc = abi_accumulate(dev, acc, counts[b0:b1], pckh[goff[b0]:goff[b1]], gop[poff[b0]:poff[b1]],
                             null=('gop',) if poff[b0] == poff[b1] else ())
    assert acc.tobytes() == one.tobytes()                                         # exact sums: the cut does not matter
    big = np.tile(counts, (100, 1))                                               # more images than threads
    assert abi_accumulate(dev, np.zeros(N_ACC), big, pckh, gop)[:N_COUNTS].tolist() == (100 * counts.astype(np.int64).sum(0)).tolist()
    nothing = abi_accumulate(dev, one, counts[:0], pckh[:0], gop[:0], null=('counts', 'pckh', 'gop'))
    assert nothing.tobytes() == one.tobytes()
    for kw in ({'null': ('acc',)}, {'B': -1}, {'Ng': -1}, {'Np': -1}, {'null': ('counts',)}, {'null': ('pckh',)}, {'null': ('gop',)}):
        assert abi_accumulate(dev, one, counts, pckh, gop, expect=ROMP_EINVAL, **kw) == ROMP_EINVAL, kw


# ------------------------------------------------------------------------------------------------ the evaluator
def run_evaluator(dev, results, annots, splits, **kw):
    from romp_amd import relative_human as R
    ev = R.RelativeHumanEvaluator(dev, kp2d_key='kp2d', depth_key='depth', **kw)
    rows = []
    for b0, b1 in splits:
        ps = np.flatnonzero((results['batch_ids'] >= b0) & (results['batch_ids'] < b1))
        gs = np.flatnonzero((annots['batch_ids'] >= b0) & (annots['batch_ids'] < b1))
        out = {'kp2d': t_(results['kp2d'][ps], dev), 'depth': t_(results['depth'][ps], dev)} if len(ps) else None
        g = {k: t_(annots[k][gs], dev) for k in ('kp2d', 'valid', 'depth_id', 'age')}
        g.update(batch_ids=t_(annots['batch_ids'][gs] - b0, dev), B=b1 - b0)
        rows.append(ev.update(out, t_(results['batch_ids'][ps] - b0, dev), g))
    return ev, rows


def test_evaluator_one_two_and_three_updates_equal_the_restatement(dev, whole):
    results, annots, (gop, pog, pckh, cv, counts) = whole
    want = summary_np(pckh, counts, gop, pog)
    one, rows1 = run_evaluator(dev, results, annots, [(0, 7)])
    two, _ = run_evaluator(dev, results, annots, [(0, 4), (4, 7)])
    three, rows3 = run_evaluator(dev, results, annots, [(0, IMG_ABSENT), (IMG_ABSENT, IMG_ABSENT + 1), (IMG_ABSENT + 1, 7)])   # the middle one: no predictions
    assert one.acc.dtype == torch.float64 and torch.equal(one.acc, two.acc) and torch.equal(one.acc, three.acc)
    assert one.acc.cpu().numpy().tobytes() == accumulate_np(np.zeros(N_ACC), counts, pckh, gop).tobytes()
    s1 = one.summary()
    assert_summaries_equal(s1, want)
    assert two.summary() == s1 and three.summary() == s1
    assert s1['matched'] == 87 and s1['misses'] == 4 and s1['false_positives'] == 1 and s1['pairs_eq'] + s1['pairs_ordered'] == 2089
    r = rows1[0]
    assert_rows_equal((r['pckh'].cpu().numpy(), r['correct_visible'].cpu().numpy(), r['counts'].cpu().numpy()), (pckh, cv, counts))
    assert np.array_equal(r['pred_of_gt'].cpu().numpy(), pog) and np.array_equal(r['gt_of_pred'].cpu().numpy(), gop)
    assert np.isnan(rows3[1]['pckh'].cpu().numpy()).all() and rows3[1]['gt_of_pred'].numel() == 0
    other, _ = run_evaluator(dev, results, annots, [(0, 7)], dr_thresh=0.5, miss_fine=0.5, pck_thresh=0.05)
    gop2, pog2, pckh2, cv2, counts2 = restated(results, annots, dr_thresh=0.5, pck_thresh=0.05)
    assert_summaries_equal(other.summary(), summary_np(pckh2, counts2, gop2, pog2, 0.5, 0.5))
    one.reset()
    assert not one.acc.any()
    for kw in ({'max_pred': 63}, {'max_gt': 63}):                                 # over either cap: summary() refuses
        over, _ = run_evaluator(dev, results, annots, [(0, 7)], **kw)
        with pytest.raises(Exception, match='max_pred'):
            over.summary()


def test_cli_on_stored_files_equals_the_evaluator(dev, whole, tmp_path, capsys):
    from romp_amd import relative_human as R
    results, annots, _ = whole
    want = run_evaluator(dev, results, annots, [(0, 7)])[0].summary()
    rp, ap = write_reference_files(tmp_path)
    res = R.main(['--results', rp, '--annots', ap, '--device', 'cuda:0'])         # the reference's own files
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    assert res == want
    fr, fa = str(tmp_path / 'r.npz'), str(tmp_path / 'a.npz')
    R.save_results(fr, **results)
    R.save_results(fa, **annots)
    assert R.main(['--results', fr, '--annots', fa]) == want                      # the flat format
    assert R.score_files(*R.load_files(fr, fa), images_per_call=3) == want
    half = R.main(['--results', fr, '--annots', fa, '--dr_thresh', '0.5'])
    assert half['dr_thresh'] == 0.5 and half['correct_eq'] > want['correct_eq'] and half['correct_ordered'] < want['correct_ordered']


# ------------------------------------------------------------------------------------------------ end to end
def test_forward_batch_scored_against_its_own_projections(dev):
    import romp_amd
    from oracle import romp_oracle as O
    from romp_amd import relative_human as R
    from romp_amd.post_parser import body_mesh_projection2image
    settings = romp_amd.romp_settings([])
    settings.GPU, settings.center_thresh, settings.max_batch = 0, 1.3, 2
    model = romp_amd.ROMP(settings, state_dict=O.make_romp_state_dict(0, center_bias=2.0), smpl_model=O.make_synthetic_smpl(0))
    out, bids = model.forward_batch(O.make_images(2, seed=3).to(dev))
    assert out is not None and out['joints'].shape[1:] == (71, 3) and out['cam_trans'].shape[1:] == (3,)
    N = out['joints'].shape[0]
    px = (body_mesh_projection2image(out['joints'], out['cam'], host_pnp=False)['pj2d'] + 1) * 256
    out['pj2d_px'] = px - px.amin() + 10.0                                        # a pixel frame in which every joint is visible (> -1)
    rng = np.random.default_rng(11)
    did, age = rng.integers(-1, 3, N).astype(np.int32), rng.integers(-1, 4, N).astype(np.int32)
    gts = {'kp2d': out['pj2d_px'][:, R.CROWDPOSE14_FROM_SMPL54], 'valid': None, 'depth_id': t_(did, dev), 'age': t_(age, dev), 'batch_ids': bids, 'B': 2}
    ev = R.RelativeHumanEvaluator(dev, kp2d_key='pj2d_px', max_pred=max(N, 64), max_gt=max(N, 64))
    rows = ev.update(out, bids, gts)
    s = ev.summary()
    print(f'{N} persons ({torch.bincount(bids.long(), minlength=2).tolist()} per image): {s}')
    assert torch.equal(rows['pred_of_gt'].cpu(), torch.arange(N, dtype=torch.int32))
    assert s['matched'] == s['n_gt'] == s['n_pred'] == N and s['misses'] == 0 and s['false_positives'] == 0 and s['unscored'] == 0
    assert s['mPCKh'] == 1.0 and s['mPCKh_scored'] == 1.0 and s['precision'] == s['recall'] == s['F1'] == 1.0
    assert (rows['correct_visible'] == 14).all()
    kp, depth, b = gts['kp2d'].cpu().numpy(), out['cam_trans'][:, 2].cpu().numpy(), bids.cpu().numpy()
    goff = offsets(b, 2)
    gop, pog, _ = match2d_np(kp, goff, kp, np.ones((N, J), bool), goff, max_pred=max(N, 64), max_gt=max(N, 64))
    pckh, cv, counts = score_np(kp, depth, kp, did, age, pog, goff, max_gt=max(N, 64))
    assert np.array_equal(rows['counts'].cpu().numpy(), counts) and np.array_equal(rows['correct_visible'].cpu().numpy(), cv)
    assert_summaries_equal(s, summary_np(pckh, counts, gop, pog))
