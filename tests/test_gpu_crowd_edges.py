"""The crowd merge alone (csrc/crowd.hip through romp_bev_crowd_merge and romp_preprocess_crops) on the cases of
tests/crowd_cases.py: the 64-crop launch seam (K = 64, 65, 71, 129), crops of 300 and 1000 rows (the later chunks of the in-place
compaction), a global stage beyond one pass of the pair grid and beyond 1024 survivors, 0-4 rows alive at every stage, ties and
chains, cam_x on the float32 bounds, H > W and hand-made crops, offsets with tails, empty runs and clamps, one non-finite row.

Per case: `keep` equals the restatement's mask over all N rows (tests/test_crowd_cases.py pins the restatement to the reference's
own stage functions); cam_full / cam_trans / pj2d_org match the float64 twin on every finite row that a crop covers -- kept or
not -- at the tolerances of tests/test_bev_crowd.py, and are non-finite where the twin is; outputs and keep live in buffers of
N + 7 rows whose tail must keep its sentinel; the call is made with the workspace filled with -1, with 0, with random words, on
the workspace the first call left, and on a side stream: all five results are the same bytes.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crowd_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu
SENT_F, SENT_I, PAD = -7.25, -77777, 7


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def _merge(dev, case, workspace, side_stream=False):
    """One romp_bev_crowd_merge call into sentinel-filled buffers of N + PAD rows.  workspace: -1 | 0 | 'random' | a tensor to
    re-use.  -> (keep, cam_full, cam_trans, pj2d_org) as host arrays of N + PAD rows, the workspace tensor."""
    from romp_amd import lib as L
    lib = L.load()
    N, K, cap = case['N'], case['K'], case['N'] + PAD
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    dj, dc, dconf = t(case['joints']), t(case['cam']), t(case['conf'])
    offsets = torch.from_numpy(case['offsets']).to(dev)
    out = [torch.full(s, SENT_F, device=dev) for s in ((cap, 3), (cap, 3), (cap, 71, 2))]
    keep = torch.full((cap,), SENT_I, dtype=torch.int32, device=dev)
    if isinstance(workspace, torch.Tensor):
        ws = workspace
    elif isinstance(workspace, str):
        ws = torch.from_numpy(np.random.RandomState(N).randint(-2 ** 31, 2 ** 31, 4 * cap + 4, dtype=np.int64).astype(np.int32)).to(dev)
    else:
        ws = torch.full((4 * cap + 4,), workspace, dtype=torch.int32, device=dev)
    crops = np.ascontiguousarray(case['crops'], np.int32)
    cp = crops.ctypes.data_as(C.POINTER(C.c_int32))
    call = lambda: L.check(lib.romp_bev_crowd_merge(
        L.ptr(dj), L.ptr(dc), L.ptr(dconf), L.ptr(offsets), N, cap, K, cp, case['H'], case['W'], case['pad_length'], case['nms'],
        case['rel'], L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(keep), L.ptr(ws), L.stream_ptr(dev)))
    if side_stream:
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            call()
        s.synchronize()
    else:
        call()
    torch.cuda.synchronize()
    return (keep.cpu().numpy(),) + tuple(o.cpu().numpy() for o in out), ws


def _check_case(dev, case):
    res, cid, N = case['res'], case['crop_id'], case['N']
    print(CC.describe(case))
    (keep, cam_full, trans, pj), ws = _merge(dev, case, -1)
    # keep: the restatement's mask over all N rows; rows no crop covers are dropped
    assert set(np.unique(keep[:N]).tolist()) <= {0, 1}
    assert keep[:N].astype(bool).tolist() == res['keep'].tolist(), np.nonzero(keep[:N].astype(bool) != res['keep'])[0]
    assert not keep[:N][cid < 0].any()
    # untouched memory: the rows beyond N keep their sentinels
    assert np.all(keep[N:] == SENT_I), 'keep was written beyond N'
    for name, a in (('cam_full', cam_full), ('cam_trans', trans), ('pj2d_org', pj)):
        assert np.all(a[N:] == np.float32(SENT_F)), name + ' was written beyond N'
    # values against the float64 twin on every finite covered row, kept or not
    cf64, tr64, pj64 = CC.twin_of(case)
    fin = (cid >= 0) & np.isfinite(cf64).all(1) & np.isfinite(tr64).all(1) & np.isfinite(pj64).all((1, 2))
    err = lambda a, b: float(np.abs(a[:N][fin] - b[fin]).max()) if fin.any() else 0.
    print('    against float64: cam_full %.1e, cam_trans %.1e (relative %.1e), pj2d_org %.1e px' % (
        err(cam_full, cf64), err(trans, tr64), float((np.abs(trans[:N][fin] - tr64[fin]) / np.maximum(np.abs(tr64[fin]), 1e-30)).max())
        if fin.any() else 0., err(pj, pj64)))
    np.testing.assert_allclose(cam_full[:N][fin], cf64[fin], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(trans[:N][fin], tr64[fin], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(pj[:N][fin], pj64[fin], rtol=0, atol=2e-3)
    bad = (cid >= 0) & ~fin                                            # the non-finite row: its finite entries hold as well
    for a, b, rtol, atol in ((cam_full[:N], cf64, 1e-6, 1e-7), (trans[:N], tr64, 1e-6, 1e-6), (pj[:N], pj64, 0, 2e-3)):
        a, b = a[bad], b[bad]
        assert np.array_equal(np.isnan(a), np.isnan(b)), 'NaN in other places than the float64 twin'
        assert np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(np.sign(a[np.isinf(b)]), np.sign(b[np.isinf(b)]))
        np.testing.assert_allclose(a[np.isfinite(b)], b[np.isfinite(b)], rtol=rtol, atol=atol)
    # workspace independence: 0, random words, the workspace the first call left, a side stream
    first = [x.tobytes() for x in (keep, cam_full, trans, pj)]
    for what, kw in (('zeros', dict(workspace=0)), ('random words', dict(workspace='random')), ('its own leftovers', dict(workspace=ws)),
                     ('a side stream', dict(workspace=-1, side_stream=True))):
        again, _ = _merge(dev, case, **kw)
        assert [x.tobytes() for x in again] == first, 'the result depends on the workspace: ' + what
    return keep[:N].astype(bool)


@pytest.mark.parametrize('name', ['seam64', 'seam65', 'seam129', 'plan71', 'big_crop', 'one_crop_1000', 'counts', 'ties', 'bounds',
                                  'geometry', 'offsets', 'nonfinite'])
def test_crowd_merge_case(dev, name):
    for case in CC.cases(name):
        _check_case(dev, case)


def test_crowd_merge_global_stride(dev):
    first, second = CC.cases('global_stride')
    keep = _check_case(dev, first)
    m = int(first['res']['keep1'].sum())
    print('survivors %d, pairs %d, first pass %d; rows whose every removing pair lies beyond it: %s'
          % (m, m * m, CC.FIRST_PASS, first['only_beyond']))
    assert first['only_beyond'] and not keep[first['only_beyond']].any()
    keep = _check_case(dev, second)
    far = second['tags']['far']
    assert not keep[far] and int(second['res']['keep1'][:far].sum()) >= 1024


@pytest.mark.parametrize('name', ['seam65', 'plan71'])
def test_crowd_preprocess_across_the_seam(dev, name):
    """romp_preprocess_crops with K > 64: the second launch's c_base, bit-equal to the oracle on every crop cut from the padded
    frame, with crops that have top > 0, bottom < H, and are narrower and wider than high."""
    from oracle import cv_resize_oracle as CV
    from romp_amd import lib as L
    lib = L.load()
    case = CC.cases(name)[0]
    H, W, pl, crops, K, S = case['H'], case['W'], case['pad_length'], case['crops'], case['K'], 64
    assert K > 64
    frame = np.random.RandomState(K).randint(0, 256, (H, W, 3)).astype(np.uint8)
    out = torch.full((K + 1, S, S, 3), SENT_F, device=dev)
    pads = (C.c_float * (6 * K))()
    arr = np.ascontiguousarray(crops, np.int32)
    dframe = torch.from_numpy(frame).to(dev)
    L.check(lib.romp_preprocess_crops(L.ptr(dframe), H, W, pl, K, arr.ctypes.data_as(C.POINTER(C.c_int32)), L.ptr(out), S, pads,
                                      L.stream_ptr(dev)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[K] == np.float32(SENT_F)), 'written beyond the last crop'
    padded = np.zeros((H, W + 2 * pl, 3), np.uint8)
    padded[:, pl:pl + W] = frame
    shapes = set()
    for c, (l, r, t, b) in enumerate(crops.tolist()):
        ref, info = CV.img_preprocess(padded[t:b, l:r], S)
        assert np.array_equal(got[c], ref[0]), (name, c)
        assert np.array_equal(np.array(pads[6 * c:6 * c + 6], np.float32), info), (name, c)
        assert np.array_equal(info, CC.crop_pad_info(b - t, r - l))
        shapes.add((t > 0, b < H, (r - l > b - t) - (r - l < b - t)))
    print('%s: %d crops at %d x %d, (top > 0, bottom < H, wider / narrower) %s' % (name, K, S, S, sorted(shapes)))
    if name == 'seam65':
        assert {s[0] for s in shapes} == {False, True} and {s[1] for s in shapes} == {False, True} and {s[2] for s in shapes} >= {-1, 1}
