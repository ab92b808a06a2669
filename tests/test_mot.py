"""Tracking scores without a GPU: the host mirror romp_amd.tracking_metrics.score_clip_host against what the reference's TrackEval
returned (golden/mot_metrics.npz, written by tests/make_golden_mot.py), the file formats, the command line and every argument
check of include/romp_hip_mot.h (all of them come before any device call).

Integer fields are equal.  Float fields: within mot_cases.reference_bound() relative = (146 accumulated terms + 4) * 2^-24 = 8.9e-6,
the float32 resolution of TrackEval's HOTA arrays; the cap-sized clip 'caps' (1024 rows a side) is held to its own bound,
(1024 + 4) * 2^-24 = 6.1e-5, which leaves the bound of the other clips where it was (mot_cases.bound_of).  Largest gap seen: 1.8e-7
(HOTA's arrays, which TrackEval keeps in float32); on 'caps' 7.1e-8.
"""
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mot_cases as MC  # noqa: E402

from romp_amd import tracking_metrics as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES, ARGS, REF, SETTINGS = MC.load()


@pytest.fixture(scope='module')
def host():
    return {n: M.score_clip_host(skip_frames_without_gt=False, **SETTINGS, **ARGS[n]) for n in NAMES}


def test_host_mirror_against_the_reference(host):
    gaps = {n: MC.against_reference(host[n], REF[n], MC.bound_of(n)) for n in NAMES}
    others = [n for n in NAMES if n != 'caps']
    bound = MC.reference_bound(others)
    print('score_clip_host against TrackEval: largest relative gap %.3g, bound %.3g; on caps %.3g, bound %.3g'
          % (max(gaps[n] for n in others), bound, gaps['caps'], MC.bound_of('caps')))
    assert len(NAMES) == 13 and len(others) == 12 and 8e-6 < bound < 1e-5 and all(MC.bound_of(n) == bound for n in others)
    assert MC.bound_of('caps') == MC.reference_bound() == 1028 * 2.0 ** -24


def test_the_fixture_holds_the_edge_cases(host):
    """What each hand-built clip is there for, read off the recorded reference values."""
    clear = {n: REF[n]['CLEAR'] for n in NAMES}
    # IoU exactly 0.5 counts for CLEAR (threshold - eps), for Identity (>=) and for HOTA up to alpha = 0.5; the pair under 1 - max_iou is zeroed
    e = REF['edges']
    assert clear['edges']['CLR_TP'] == 3 and clear['edges']['CLR_FN'] == 3 and e['Identity']['IDTP'] == 3
    assert e['HOTA']['HOTA_TP'].tolist() == [3.] * 10 + [0.] * 9
    sim = M.iou_host(ARGS['edges']['gt_boxes'][:2], ARGS['edges']['pred_boxes'][:2])
    assert sim[0, 0] == 0.5 and sim[1, 1] == 0. and 0.0098 < M.iou_host(ARGS['edges']['gt_boxes'][:2], ARGS['edges']['pred_boxes'][:2], 1.)[1, 1] < 0.01
    assert clear['disjoint']['CLR_TP'] == 0 and REF['disjoint']['HOTA']['HOTA_TP'].max() == 0 and REF['disjoint']['Identity']['IDTP'] == 0
    # one IDSW after three frames of absence, two broken runs, 4/5 is not MT, 1/5 is PT
    c = clear['clear_book']
    assert (c['IDSW'], c['Frag'], c['MT'], c['PT'], c['ML']) == (1, 2, 1, 2, 0)
    # empty sides: the early returns
    assert clear['no_pred']['CLR_FN'] == 3 and clear['no_pred']['ML'] == 2 and clear['no_pred']['MLR'] == 1. and clear['no_pred']['CLR_Frames'] == 0
    assert clear['no_gt']['CLR_FP'] == 3 and clear['no_gt']['MOTA'] == 0. and REF['no_gt']['HOTA']['LocA'].tolist() == [1.] * 19
    assert clear['empty_frames']['CLR_Frames'] == 6 and clear['single_frame']['CLR_Frames'] == 1
    # shapes: past 64 rows on either side, 65 ground-truth ids, raw ids with gaps
    for n, k in (('wide', 'gt_ids'), ('wide', 'pred_ids'), ('ids65', 'gt_ids')):
        assert len(np.unique(ARGS[n][k])) >= 65
    assert np.bincount(ARGS['wide']['gt_frames']).tolist() == [70, 3] and np.bincount(ARGS['wide']['pred_frames']).tolist() == [3, 70]
    assert sorted(set(ARGS['empty_frames']['gt_ids'].tolist())) == [3, 17, 900]
    # the caps: 256 rows a side in every frame, 512 ids a side (Identity's assignment is 512 x 512), predictions with ids of the other half
    a = ARGS['caps']
    assert np.bincount(a['gt_frames']).tolist() == [256] * 4 == np.bincount(a['pred_frames']).tolist()
    assert len(np.unique(a['gt_ids'])) == 512 == len(np.unique(a['pred_ids'])) and M.MAX_DET == 256 and M.MAX_IDS == 512
    assert clear['caps']['IDSW'] > 0 and clear['caps']['CLR_TP'] == 1024 and REF['caps']['Identity']['IDFP'] > 0


def test_a_non_finite_box_is_similar_to_nothing():
    """iou_host: a NaN or +-inf coordinate gives similarity exactly 0 in that row or column; every other element keeps its bits."""
    a = ARGS['seed40']
    gt, pred = a['gt_boxes'][:12].copy(), a['pred_boxes'][:9].copy()
    gt[:9, :2] = pred[:, :2] + 3                          # (overlaps on the diagonal: zeros there would be noticed)
    clean = M.iou_host(gt, pred)
    assert (clean > 0).sum() >= 9
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(4):
            g2, p2 = gt.copy(), pred.copy()
            g2[3, k] = bad
            p2[5, k] = bad
            got = M.iou_host(g2, p2)
            assert np.all(got[3] == 0) and np.all(got[:, 5] == 0) and not np.isnan(got).any(), (bad, k)
            keep = np.ones_like(clean, bool)
            keep[3], keep[:, 5] = False, False
            assert got[keep].tobytes() == clean[keep].tobytes(), (bad, k)


def test_skipping_frames_without_ground_truth(host):
    a = ARGS['empty_frames']
    got = M.score_clip_host(skip_frames_without_gt=True, **SETTINGS, **a)
    keep = np.isin(a['pred_frames'], a['gt_frames'])
    want = M.score_clip_host(a['pred_ids'][keep], a['pred_frames'][keep], a['gt_boxes'], a['gt_ids'], a['gt_frames'], pred_boxes=a['pred_boxes'][keep],
                             skip_frames_without_gt=False, **SETTINGS)
    assert M._compare(got, want, 0.) is None
    assert got['CLEAR']['CLR_Frames'] == 4 and got['CLEAR']['CLR_FP'] < host['empty_frames']['CLEAR']['CLR_FP']


def test_combining_clips(host):
    ref, comb = M.combine_clips({n: host[n] for n in ('single_frame', 'seed7', 'seed40')})
    three = [host[n] for n in ('single_frame', 'seed7', 'seed40')]
    assert ref['HOTA'] == pytest.approx(100 * np.mean([np.mean(r['HOTA']['HOTA']) for r in three]), rel=1e-15)
    assert comb['CLEAR']['CLR_TP'] == sum(r['CLEAR']['CLR_TP'] for r in three) and comb['CLEAR']['IDSW'] == sum(r['CLEAR']['IDSW'] for r in three)
    tp, fn, fp, sw = (sum(r['CLEAR'][k] for r in three) for k in ('CLR_TP', 'CLR_FN', 'CLR_FP', 'IDSW'))
    assert comb['CLEAR']['MOTA'] == pytest.approx((tp - fp - sw) / (tp + fn), rel=1e-15)
    idtp, idfn, idfp = (sum(r['Identity'][k] for r in three) for k in ('IDTP', 'IDFN', 'IDFP'))
    assert comb['Identity']['IDF1'] == pytest.approx(idtp / (idtp + 0.5 * idfp + 0.5 * idfn), rel=1e-15)
    w = np.stack([r['HOTA']['HOTA_TP'] for r in three])
    assert np.allclose(comb['HOTA']['AssA'], (np.stack([r['HOTA']['AssA'] for r in three]) * w).sum(0) / np.maximum(1, w.sum(0)), rtol=1e-15)


# ------------------------------------------------------------------------------------------------ files and the command line
def _files(tmp_path, names):
    res = {n: {'ids': ARGS[n]['pred_ids'], 'frames': ARGS[n]['pred_frames'],
               **({'kp2d': ARGS[n]['pred_kp2d']} if 'pred_kp2d' in ARGS[n] else {'boxes': ARGS[n]['pred_boxes']})} for n in names}
    gt = {n: {'ids': ARGS[n]['gt_ids'], 'frames': ARGS[n]['gt_frames'], 'boxes': ARGS[n]['gt_boxes']} for n in names}
    r, g = str(tmp_path / 'results.npz'), str(tmp_path / 'gt.npz')
    M.save_results(r, res)
    M.save_results(g, gt)
    return r, g, res, gt


def test_file_round_trip(tmp_path):
    r, g, res, gt = _files(tmp_path, ['seed7', 'seed40', 'no_pred'])
    with np.load(r, allow_pickle=False) as z:               # flat and pickle-free
        assert all(z[k].dtype != object for k in z.files)
    for path, want in ((r, res), (g, gt)):
        got = M.load_results(path)
        assert sorted(got) == sorted(want)
        for n in want:
            assert sorted(got[n]) == sorted(want[n])
            for k in want[n]:
                assert np.array_equal(got[n][k], want[n][k]) and got[n][k].dtype == (np.float32 if k in ('boxes', 'kp2d') else np.int64)


def test_reference_file_formats(tmp_path):
    """'<clip>_tracking.npz' with tracking[frame]['track_ids' | 'track_bbox' | 'pj2ds'] and annots[clip][frame] = [paths, ids, boxes, dense ids]."""
    a = ARGS['seed7_kp2d']
    tracking = {'%05d.jpg' % f: {'track_ids': a['pred_ids'][a['pred_frames'] == f], 'track_bbox': np.zeros((int((a['pred_frames'] == f).sum()), 4)),
                                 'pj2ds': a['pred_kp2d'][a['pred_frames'] == f]} for f in range(7)}
    annots = {'seed7_kp2d': {'%05d.jpg' % f: [['x/%05d.jpg' % f] * int((a['gt_frames'] == f).sum()), a['gt_ids'][a['gt_frames'] == f] + 40,
                                              a['gt_boxes'][a['gt_frames'] == f], a['gt_ids'][a['gt_frames'] == f]] for f in range(7)}}
    r, g = str(tmp_path / 'seed7_kp2d_tracking.npz'), str(tmp_path / 'gts.npz')
    np.savez(r, tracking=np.array(tracking, dtype=object))
    np.savez(g, annots=np.array(annots, dtype=object))
    res, gt = M.load_results(r), M.load_results(g)
    assert list(res) == ['seed7_kp2d'] == list(gt) and 'kp2d' in res['seed7_kp2d'] and M.validate_files(res, gt) == []
    got = M.score_clip_host(res['seed7_kp2d']['ids'], res['seed7_kp2d']['frames'], gt['seed7_kp2d']['boxes'], gt['seed7_kp2d']['ids'],
                            gt['seed7_kp2d']['frames'], pred_kp2d=res['seed7_kp2d']['kp2d'], **SETTINGS)
    MC.against_reference(got, REF['seed7_kp2d'], MC.reference_bound())


def test_command_line_check_on_the_host(tmp_path, capsys, host):
    r, g, _, _ = _files(tmp_path, ['seed7', 'seed40'])
    assert M.main(['--results', r, '--gt', g, '--check', '--host', '--keep_frames_without_gt']) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out['ok'] is True and out['scored_on'] == 'host' and sorted(out['clips']) == ['seed40', 'seed7']
    assert out['clips']['seed40']['CLEAR']['IDSW'] == host['seed40']['CLEAR']['IDSW'] == REF['seed40']['CLEAR']['IDSW']
    assert out['clips']['seed7']['HOTA']['HOTA'] == host['seed7']['HOTA']['HOTA'].tolist()
    assert out['combined']['Identity']['IDTP'] == host['seed7']['Identity']['IDTP'] + host['seed40']['Identity']['IDTP']
    # a file in which an id owns two rows of a frame, and a clip without ground truth: --check says so and fails
    bad = {'seed7': {'ids': np.array([1, 1]), 'frames': np.array([0, 0]), 'boxes': np.zeros((2, 4), np.float32)},
           'other': {'ids': np.array([1]), 'frames': np.array([0]), 'boxes': np.zeros((1, 4), np.float32)}}
    b = str(tmp_path / 'bad.npz')
    M.save_results(b, bad)
    assert M.main(['--results', b, '--gt', g, '--check', '--host']) == 1
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out['ok'] is False and any('two rows' in e for e in out['errors']) and any('missing' in e for e in out['errors'])
    with pytest.raises(SystemExit):
        M.main(['--results', r, '--gt', g, '--threshold', '0'])
    with pytest.raises(SystemExit):
        M.main(['--results', r])


def test_python_argument_validation():
    a = ARGS['seed7']
    with pytest.raises(ValueError, match='one of them'):
        M.score_clip_host(a['pred_ids'], a['pred_frames'], a['gt_boxes'], a['gt_ids'], a['gt_frames'])
    with pytest.raises(ValueError, match='one of them'):
        M.score_clip_host(a['pred_ids'], a['pred_frames'], a['gt_boxes'], a['gt_ids'], a['gt_frames'], pred_boxes=a['pred_boxes'],
                          pred_kp2d=np.zeros((len(a['pred_ids']), 3, 2)))
    with pytest.raises(ValueError, match='two rows'):
        M.score_clip_host([1, 1], [0, 0], a['gt_boxes'], a['gt_ids'], a['gt_frames'], pred_boxes=np.zeros((2, 4)))
    with pytest.raises(ValueError, match='frame numbers'):
        M.score_clip_host(a['pred_ids'][:-1], a['pred_frames'], a['gt_boxes'], a['gt_ids'], a['gt_frames'], pred_boxes=a['pred_boxes'])
    with pytest.raises(ValueError, match='at most 256'):
        M.score_clip_host(np.arange(257), np.zeros(257), a['gt_boxes'], a['gt_ids'], a['gt_frames'], pred_boxes=np.zeros((257, 4)), skip_frames_without_gt=False)
    with pytest.raises(ValueError, match='at most 512'):
        M.score_clip_host(np.arange(513), np.arange(513), np.zeros((513, 4)), np.arange(513), np.arange(513), pred_boxes=np.zeros((513, 4)))
    with pytest.raises(ValueError, match='kp2d must be'):
        M.score_clip_host(a['pred_ids'], a['pred_frames'], a['gt_boxes'], a['gt_ids'], a['gt_frames'], pred_kp2d=np.zeros((len(a['pred_ids']), 4)))


# ------------------------------------------------------------------------------------------------ the C seam
def test_mot_symbols_exported():
    from romp_amd import lib
    header = open(os.path.join(ROOT, 'include', 'romp_hip_mot.h')).read()
    declared = re.findall(r'^\s*(?:int|void)\s+(\w+)\s*\(', header, re.M)
    assert declared == lib.MOT_EXPORTS and len(declared) == 8
    others = (lib.EXPORTS + lib.VIEW_EXPORTS + lib.MAP_EXPORTS + lib.TEXTURE_EXPORTS + lib.EVAL_EXPORTS + lib.RH_EXPORTS + lib.CANVAS_EXPORTS +
              lib.SMPL_GRAD_EXPORTS + lib.FIT_EXPORTS + lib.FIT_PRIOR_EXPORTS + lib.TRACK_EXPORTS)
    assert not set(declared) & set(others) and len(lib.EXPORTS) == 52
    h = lib.load()
    assert h.romp_abi_version() == 7 == lib.ABI_VERSION
    for n in declared:
        assert getattr(h, n).restype is ctypes.c_int, n


def test_the_header_compiles_as_c():
    prog = ('#include "romp_hip_mot.h"\nint main(void) { return ROMP_MOT_ALPHAS == 19 && ROMP_MOT_HOTA_OUT == 7 && ROMP_MOT_CLEAR_OUT == 12 && '
            'ROMP_MOT_ID_OUT == 3 ? 0 : 1; }\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, 't.c')
        open(c, 'w').write(prog)
        subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), c, '-o', os.path.join(td, 't')])
        subprocess.check_call([os.path.join(td, 't')])


def _pack(h, S, F, clip_frames, gt_off, pred_off, n_gt, n_pred, block=None, words=0):
    i32 = lambda a: (ctypes.c_int32 * len(a))(*a) if a is not None else None  # noqa: E731
    return h.romp_mot_pack(S, F, i32(clip_frames), i32(gt_off), i32(pred_off), i32(n_gt), i32(n_pred), block, words)


def test_host_side_validation_needs_no_device():
    """Caps and NULL pointers: ROMP_EINVAL before any device call, so the refusals run on a machine without a GPU."""
    from romp_amd import lib
    h = lib.load()
    good = (2, 3, [0, 1, 3], [0, 2, 2, 5], [0, 0, 4, 256], [3, 2], [512, 0])
    words = _pack(h, *good)
    assert words == 16 + 3 + 4 + 9 + 3 + 12
    block = (ctypes.c_int64 * words)()
    assert _pack(h, *good, block, words) == words and list(block[:3]) == [0x4d4f5431, 2, 3]
    assert _pack(h, *good, block, words - 1) == -1 and b'words' in h.romp_last_error()
    for bad, why in (((0, 0, [0], [0], [0], [], []), b'S 0'),
                     ((2, 3, [0, 2, 1], [0, 2, 2, 5], [0, 0, 4, 8], [3, 2], [4, 0]), b'clip_frames'),
                     ((2, 3, [0, 1, 3], [0, 2, 2, 259], [0, 0, 4, 8], [3, 2], [4, 0]), b'rows'),
                     ((2, 3, [0, 1, 3], [0, 2, 2, 5], [0, 0, 4, 261], [3, 2], [4, 0]), b'rows'),
                     ((2, 3, [0, 1, 3], [0, 2, 1, 5], [0, 0, 4, 8], [3, 2], [4, 0]), b'rows'),
                     ((2, 3, [0, 1, 3], [0, 2, 2, 5], [0, 0, 4, 8], [513, 2], [4, 0]), b'ids'),
                     ((2, 3, [0, 1, 3], [0, 2, 2, 5], [0, 0, 4, 8], [3, 2], [4, 513]), b'ids'),
                     ((2, 3, [0, 1, 3], [1, 2, 2, 5], [0, 0, 4, 8], [3, 2], [4, 0]), b'start at 0'),
                     ((2, 3, None, [0, 2, 2, 5], [0, 0, 4, 8], [3, 2], [4, 0]), b'NULL')):
        assert _pack(h, *bad) == -1 and why in h.romp_last_error(), (bad, h.romp_last_error())
    nbytes = ctypes.c_int64(0)
    assert h.romp_mot_workspace_bytes(block, ctypes.byref(nbytes)) == 0 and nbytes.value > 0 and nbytes.value % 8 == 0
    assert h.romp_mot_workspace_bytes(None, ctypes.byref(nbytes)) == -1 and h.romp_mot_workspace_bytes(block, None) == -1
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    alphas = (ctypes.c_double * 19)(*M.ALPHAS.tolist())
    broken = (ctypes.c_int64 * words)(*block)
    broken[16 + 3] = 513                                    # n_gt_ids[0] past the cap in a block that still carries the magic
    for b in (None, broken):
        assert h.romp_mot_tables(b, p, p, p, p, None) == -1 and b'block' in h.romp_last_error()
        assert h.romp_mot_similarity(b, p, p, p, p, None, 0, 1., 1., p, 0.99, p, p, p, None) == -1
        assert h.romp_mot_hota(b, p, p, p, p, p, p, alphas, p, p, None) == -1
        assert h.romp_mot_clear(b, p, p, p, p, 0.5, p, p, None) == -1
        assert h.romp_mot_identity(b, p, p, p, p, 0.5, p, p, None) == -1
    # a good block: every other pointer and value is looked at before anything is launched
    assert h.romp_mot_tables(block, None, p, p, p, None) == -1 and h.romp_mot_tables(block, p, None, p, p, None) == -1
    assert h.romp_mot_tables(block, p, p, p, None, None) == -1
    assert h.romp_mot_similarity(block, p, None, p, p, None, 0, 1., 1., p, 0.99, p, p, p, None) == -1
    assert h.romp_mot_similarity(block, p, p, p, p, p, 5, 1., 1., p, 0.99, p, p, p, None) == -1 and b'one of them' in h.romp_last_error()
    assert h.romp_mot_similarity(block, p, p, p, None, None, 5, 1., 1., p, 0.99, p, p, p, None) == -1
    assert h.romp_mot_similarity(block, p, p, p, None, p, 0, 1., 1., p, 0.99, p, p, p, None) == -1 and b'J 0' in h.romp_last_error()
    assert h.romp_mot_similarity(block, p, p, p, None, p, 5, 0., 1., p, 0.99, p, p, p, None) == -1
    assert h.romp_mot_similarity(block, p, p, p, p, None, 0, 1., 1., p, 1.5, p, p, p, None) == -1 and b'max_iou' in h.romp_last_error()
    assert h.romp_mot_similarity(block, p, p, p, p, None, 0, 1., 1., p, 0.99, None, p, p, None) == -1
    assert h.romp_mot_hota(block, p, p, p, p, p, p, None, p, p, None) == -1 and h.romp_mot_hota(block, p, p, p, p, p, p, alphas, None, p, None) == -1
    assert h.romp_mot_hota(block, p, p, p, p, p, p, alphas, p, None, None) == -1 and h.romp_mot_hota(block, p, p, p, p, None, p, alphas, p, p, None) == -1
    down = (ctypes.c_double * 19)(*M.ALPHAS[::-1].tolist())
    assert h.romp_mot_hota(block, p, p, p, p, p, p, down, p, p, None) == -1 and b'alphas' in h.romp_last_error()
    for fn in (h.romp_mot_clear, h.romp_mot_identity):
        assert fn(block, p, p, p, p, 0., p, p, None) == -1 and b'threshold' in h.romp_last_error()
        assert fn(block, p, p, p, p, 0.5, None, p, None) == -1 and fn(block, p, p, p, p, 0.5, p, None, None) == -1
        assert fn(block, p, None, p, p, 0.5, p, p, None) == -1 and fn(block, p, p, p, None, 0.5, p, p, None) == -1
    assert h.romp_mot_boxes(None, 1, 5, 1.1, 1.18, p, None) == -1 and h.romp_mot_boxes(p, 0, 5, 1.1, 1.18, p, None) == -1
    assert h.romp_mot_boxes(p, 1, 0, 1.1, 1.18, p, None) == -1 and h.romp_mot_boxes(p, 1, 5, 0., 1.18, p, None) == -1
    # the Python wrapper raises with the library's message
    with pytest.raises(lib.RompHipError, match='rows'):
        M.pack_layout([0, 1], [0, 257], [0, 1], [1], [1])
