"""BEV post-processing (projection, duplicate suppression, outlier removal) and device pre-processing.
CPU: oracle vs the reference-generated fixtures bev_post.npz and bev_post_edges.npz; the conditions under which the scenes of
tests/test_gpu_bev_post.py have an exact expected keep set.  GPU: HIP kernels (csrc/post.hip) vs both."""
import os

import numpy as np
import pytest
import torch

from oracle import bev_post_oracle as PO


def _gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'bev_post.npz'))


def test_bev_post_oracle_vs_reference(golden_dir):
    g = _gold(golden_dir)
    r = PO.postprocess(g['joints'], g['cam'], g['pad'], 20.0, 1.6)
    np.testing.assert_allclose(r['pj2d_org'], g['pj2d_org'], rtol=1e-5, atol=2e-3)
    np.testing.assert_allclose(r['cam_trans'], g['cam_trans'], rtol=1e-5, atol=1e-6)
    assert np.nonzero(r['keep'])[0].tolist() == g['kept_final'].tolist()
    r2 = PO.postprocess(g['joints'], g['cam'], g['pad'], 20.0, 1e9)      # outlier removal disabled
    assert np.nonzero(r2['keep'])[0].tolist() == g['kept_after_nms'].tolist()


@pytest.mark.gpu
def test_bev_post_hip(golden_dir):
    from romp_amd import lib as L
    lib = L.load()
    dev = torch.device('cuda:0')
    g = _gold(golden_dir)
    # two images: the fixture persons + 3 more persons in a second image (N<3 after nms -> no outlier test)
    rs = np.random.RandomState(1)
    j2 = (0.25 * rs.randn(3, 71, 3)).astype(np.float32)
    c2 = np.array([[0.7, 0.1, 0.2], [0.69, 0.1, 0.2], [0.4, -0.5, 0.3]], np.float32)
    j2[1] = j2[0] + 0.001
    pad2 = np.array([0, 512, 64, 448, 512, 384], np.float32)
    joints = torch.from_numpy(np.concatenate([g['joints'], j2])).to(dev)
    cam = torch.from_numpy(np.concatenate([g['cam'], c2])).to(dev)
    N = cam.shape[0]
    offsets = torch.tensor([0, 9, 12], dtype=torch.int32, device=dev)
    pads = torch.from_numpy(np.stack([g['pad'], pad2])).float().to(dev)
    pj, pjo, tr = torch.empty(N, 71, 2, device=dev), torch.empty(N, 71, 2, device=dev), torch.empty(N, 3, device=dev)
    keep = torch.empty(N, dtype=torch.int32, device=dev)
    L.check(lib.romp_bev_postprocess(L.ptr(joints), L.ptr(cam), L.ptr(offsets), 2, L.ptr(pads), 20.0, 1.6, L.ptr(pj),
                                     L.ptr(pjo), L.ptr(tr), L.ptr(keep), L.stream_ptr(dev)))
    torch.cuda.synchronize()
    np.testing.assert_allclose(pjo[:9].cpu().numpy(), g['pj2d_org'], rtol=1e-5, atol=5e-3)
    np.testing.assert_allclose(tr[:9].cpu().numpy(), g['cam_trans'], rtol=1e-5, atol=1e-6)
    assert np.nonzero(keep[:9].cpu().numpy())[0].tolist() == g['kept_final'].tolist()
    r2 = PO.postprocess(j2, c2, pad2, 20.0, 1.6)
    assert keep[9:].cpu().numpy().astype(bool).tolist() == r2['keep'].tolist()
    np.testing.assert_allclose(pjo[9:].cpu().numpy(), r2['pj2d_org'], rtol=1e-5, atol=5e-3)
    np.testing.assert_allclose(pj[9:].cpu().numpy(), r2['pj2d'], rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(360, 640), (720, 1280), (1080, 1920), (600, 400), (512, 512), (37, 53)])
def test_preprocess_hip_vs_oracle(shape):
    """Device img_preprocess (csrc/post.hip) vs the CPU oracle of the reference's pre-processing (oracle/cv_resize_oracle.py:
    cv2.cvtColor + padding_image + cv2.resize INTER_CUBIC restated in OpenCV's fixed-point arithmetic): BIT-EXACT, single frame
    and batched."""
    import ctypes as C
    from oracle import cv_resize_oracle as CV
    from romp_amd import lib as L
    from romp_amd.utils import img_preprocess_device
    rs = np.random.RandomState(shape[0])
    img = rs.randint(0, 256, shape + (3,)).astype(np.uint8)
    ref, pad_ref = CV.img_preprocess(img)
    dev = torch.device('cuda:0')
    out, pad = img_preprocess_device(img, dev)
    assert pad.tolist() == pad_ref.tolist()
    d = np.abs(out.cpu().numpy() - ref)
    print(shape, 'differing values', int((d > 0).sum()))
    assert d.max() == 0.0
    # batch of 3 different frames in one launch
    frames = rs.randint(0, 256, (3,) + shape + (3,)).astype(np.uint8)
    fd = torch.from_numpy(frames).to(dev)
    ob = torch.empty(3, 512, 512, 3, device=dev)
    pi = (C.c_float * 6)()
    L.check(L.load().romp_preprocess_batch(L.ptr(fd), 3, shape[0], shape[1], L.ptr(ob), 512, pi, L.stream_ptr(dev)))
    torch.cuda.synchronize()
    for b in range(3):
        rb, _ = CV.img_preprocess(frames[b])
        assert np.array_equal(ob[b].cpu().numpy(), rb[0])
    assert list(pi) == pad_ref.tolist()


# ------------------------------------------------------------------------- edge scenes and generated scenes (CPU)
# tests/golden/bev_post_edges.npz: scenes of at most 4 persons through the reference's own functions
# (oracle/make_golden_bev_post_edges.py).  tests/test_gpu_bev_post.py runs the same scenes, and the generated ones below,
# through bev_post_kernel.
NMS, REL = 20.0, 1.6
MARGIN, MIN_DEPTH = 1e-3, 0.3
PADS = ([280, 1000, 0, 1280, 720, 1280], [0, 800, 100, 700, 800, 600], [0, 512, 0, 512, 512, 512])
COUNTS = (1, 2, 3, 4, 63, 64)


def edge_scenes(golden_dir):
    """-> {name: dict(joints, cam, pad, pj2d_org, cam_trans, kept_after_nms, kept_final)} in the fixture's order."""
    g = np.load(os.path.join(golden_dir, 'bev_post_edges.npz'))
    keys = ('joints', 'cam', 'pad', 'pj2d_org', 'cam_trans', 'kept_after_nms', 'kept_final')
    return {str(name): {k: g['%s_%s' % (name, k)] for k in keys} for name in g['scenes']}


def random_scene(seed, n):
    """n detections in the style of _random_detections of tests/test_bev_crowd.py: a few base bodies with jitter, planted
    near-duplicates (alternately the larger and the smaller of the pair comes first), about a tenth of the persons remote and
    tiny -- from 3 persons on the last row always is.  -> float32 joints (n,71,3), cam (n,3), pad (6,)."""
    rs = np.random.RandomState(seed)
    cam = np.stack([rs.uniform(0.2, 1.2, n), rs.uniform(-0.5, 0.5, n), rs.uniform(-1.1, 1.1, n)], 1)
    cam[rs.rand(n) < 0.1, 0] = 0.04
    if n >= 3:
        cam[n - 1, 0] = 0.04
    base = rs.randn(8, 71, 3) * [0.25, 0.45, 0.1]
    joints = base[rs.randint(0, 8, n)] + rs.randn(n, 71, 3) * 0.03
    for i in range(0 if n < 2 else max(1, n // 16)):
        src, dst = 13 * i, 13 * i + 1
        joints[dst] = joints[src] + rs.randn(71, 3) * 0.002
        cam[dst] = cam[src] * [1.03 if i % 2 else 0.97, 1, 1] + [0, 0.002, -0.002]
    return joints.astype(np.float32), cam.astype(np.float32), np.array(PADS[n % 3], np.float32)


def scene_conditions(joints, cam, pad):
    """What makes a scene's expected keep set exact: evaluated with the float64 restatement.  -> (ok, float64 result,
    float32 result, margin, smallest projected depth)."""
    r64 = PO.postprocess(joints, cam, pad, NMS, REL, dtype=np.float64)
    r32 = PO.postprocess(joints, cam, pad, NMS, REL)
    depth = float((np.asarray(joints, np.float64)[:, :, 2] + r64['cam_trans'][:, None, 2]).min())
    ok = r64['margin'] >= MARGIN and depth >= MIN_DEPTH and r32['keep'].tolist() == r64['keep'].tolist()
    return ok, r64, r32, r64['margin'], depth


_FOUND = {}


def find_scene(n):
    """The first of at most 20 seeds whose scene of n persons satisfies scene_conditions (None if there is none)."""
    if n not in _FOUND:
        _FOUND[n] = None
        for seed in range(100 * n, 100 * n + 20):
            scene = random_scene(seed, n)
            res = scene_conditions(*scene)
            if res[0]:
                _FOUND[n] = (seed, scene) + res[1:]
                break
    return _FOUND[n]


def test_bev_post_restatement_vs_edge_fixture(golden_dir):
    """The float32 restatement reproduces every edge scene of the reference: both keep sets exactly, the projections and
    translations within the tolerances of test_bev_post_oracle_vs_reference."""
    for name, s in edge_scenes(golden_dir).items():
        r = PO.postprocess(s['joints'], s['cam'], s['pad'], NMS, REL)
        np.testing.assert_allclose(r['pj2d_org'], s['pj2d_org'], rtol=1e-5, atol=2e-3, err_msg=name)
        np.testing.assert_allclose(r['cam_trans'], s['cam_trans'], rtol=1e-5, atol=1e-6, err_msg=name)
        assert np.nonzero(r['keep'])[0].tolist() == s['kept_final'].tolist(), name
        r2 = PO.postprocess(s['joints'], s['cam'], s['pad'], NMS, 1e9)      # outlier removal disabled
        assert np.nonzero(r2['keep'])[0].tolist() == s['kept_after_nms'].tolist(), name
        assert r2['stages'] == {'suppressed': len(s['cam']) - len(s['kept_after_nms']), 'outliers': 0}, name
        assert r['stages'] == {'suppressed': len(s['cam']) - len(s['kept_after_nms']),
                               'outliers': len(s['kept_after_nms']) - len(s['kept_final'])}, name


def test_bev_post_default_dtype_keeps_its_bits(golden_dir):
    """dtype=np.float32 is the default, and the float64 restatement differs from it by float32 roundings only."""
    g = _gold(golden_dir)
    a, b = PO.postprocess(g['joints'], g['cam'], g['pad']), PO.postprocess(g['joints'], g['cam'], g['pad'], dtype=np.float32)
    c = PO.postprocess(g['joints'], g['cam'], g['pad'], dtype=np.float64)
    for k in ('pj2d', 'pj2d_org', 'cam_trans'):
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]) and c[k].dtype == np.float64
        assert 0 < np.abs(a[k] - c[k]).max() <= 64 * 2.0 ** -24 * np.abs(c[k]).max(), k
    assert a['keep'].tolist() == c['keep'].tolist() and a['stages'] == c['stages'] == {'suppressed': 2, 'outliers': 1}
    assert abs(a['margin'] - c['margin']) < 1e-4 * c['margin']


def test_bev_post_scene_conditions(golden_dir):
    """Every scene the GPU tests use has an exact expected keep set: in float64 no compared value lies within 1e-3
    (relative) of its threshold, every projected depth is at least 0.3, and float32 arithmetic gives the same set.
    tie (distance 0) and same_place (translation distances 0, rel = 0/0) are exact by construction: their margin counts the
    pair distances that are not degenerate in that way."""
    for name, s in edge_scenes(golden_dir).items():
        ok, r64, r32, margin, depth = scene_conditions(s['joints'], s['cam'], s['pad'])
        print('%-15s margin %.3g min depth %.3g kept %s' % (name, margin, depth, np.nonzero(r64['keep'])[0].tolist()))
        assert ok, name
        assert np.nonzero(r64['keep'])[0].tolist() == s['kept_final'].tolist(), name
    for n in COUNTS + (65,):
        found = find_scene(n)
        assert found is not None, 'no seed of 20 gives a scene of %d persons away from the thresholds' % n
        seed, _, r64, _, margin, depth = found
        print('n=%d seed %d margin %.3g min depth %.3g stages %s' % (n, seed, margin, depth, r64['stages']))
    joints, cam, pad = find_scene(65)[1]                                # the first 64 rows of the 65 are a scene too
    assert scene_conditions(joints[:64], cam[:64], pad)[0]
    st = find_scene(64)[2]['stages']
    assert st['suppressed'] > 0 and st['outliers'] > 0


def test_bev_post_every_stage_exercised(golden_dir):
    """Each edge scene shows what it is named for (float64 restatement), and over all scenes both passes removed someone."""
    sc = edge_scenes(golden_dir)
    run = lambda s, **kw: PO.postprocess(s['joints'], s['cam'], s['pad'], **dict(dict(nms_thresh=NMS, relative_scale_thresh=REL,
                                                                                      dtype=np.float64), **kw))
    res = {name: run(s) for name, s in sc.items()}
    kept = {name: np.nonzero(r['keep'])[0].tolist() for name, r in res.items()}
    stages = {name: (r['stages']['suppressed'], r['stages']['outliers']) for name, r in res.items()}
    assert sum(a for a, _ in stages.values()) > 0 and sum(b for _, b in stages.values()) > 0
    assert max(len(s['cam']) for s in sc.values()) <= 4
    assert kept['one'] == [0] and stages['one'] == (0, 0)
    assert kept['pair'] == [1] and sc['pair']['cam'][0, 0] < sc['pair']['cam'][1, 0]         # the smaller scale goes: row 0
    assert kept['tie'] == [0] and np.array_equal(sc['tie']['joints'][0], sc['tie']['joints'][1]) \
        and np.array_equal(sc['tie']['cam'][0], sc['tie']['cam'][1])                          # equal scales: the later row goes
    # chain: A-B and B-C inside the threshold, A-C outside; B, although removed by A, still removes C
    s = sc['chain']
    org = res['chain']['pj2d_org']
    d = np.sqrt(((org[:, None] - org[None]) ** 2).sum(-1)).mean(-1) / (2 * np.maximum(s['cam'][:, None, 0], s['cam'][None, :, 0]))
    thr = NMS * 1280 / 640
    assert d[0, 1] < thr and d[1, 2] < thr and d[0, 2] > thr and kept['chain'] == [0] and stages['chain'] == (2, 0)
    assert kept['outlier3'] == [0, 1] and stages['outlier3'] == (0, 1)                        # m == 3: (m - 2) == 1
    for name in ('gate_at', 'gate_above'):                                                    # the scale gate alone keeps row 2
        assert kept[name] == [0, 1, 2] and np.nonzero(run(sc[name], scale_thresh=0.3)['keep'])[0].tolist() == [0, 1]
    assert sc['gate_at']['cam'][2, 0] == 0.25 and sc['gate_above']['cam'][2, 0] > 0.25
    # nms_then_few: two survivors, so the outlier pass does not run -- over all four rows it would remove the remote row 1
    s = sc['nms_then_few']
    assert kept['nms_then_few'] == [0, 1] and stages['nms_then_few'] == (2, 0)
    all4 = run(s, nms_thresh=1e-9)
    assert all4['stages'] == {'suppressed': 0, 'outliers': 1} and not all4['keep'][1] and s['cam'][1, 0] < 0.25
    # survivors_only: the remote row 1 is an outlier among the survivors and is not one among all four rows
    assert kept['survivors_only'] == [0, 2] and stages['survivors_only'] == (1, 1)
    assert run(sc['survivors_only'], nms_thresh=1e-9)['keep'].all()
    # same_place: equal translations, rel = 0/0 compares false, cam[:, 0] is under the scale gate
    s = sc['same_place']
    assert kept['same_place'] == [0, 1, 2] and np.all(s['cam'][:, 0] < 0.25) and np.ptp(res['same_place']['cam_trans'], 0).max() == 0
    # the three pad layouts: left > 0, top > 0, neither; three pad sizes
    pads = [sc[k]['pad'] for k in ('portrait', 'landscape', 'square')]
    assert pads[0][2] > 0 and pads[0][0] == 0 and pads[1][0] > 0 and pads[1][2] == 0 and pads[2][0] == pads[2][2] == 0
    assert len({float(max(p[4], p[5])) for p in pads}) == 3
    for k in ('portrait', 'landscape', 'square'):
        assert kept[k] == [0, 1] and np.array_equal(sc[k]['joints'], sc['outlier3']['joints'])


def chain_in_crowd(golden_dir):
    """The `chain` persons A, B, C as rows 0, 4, 5 of a 64-person image.  bev_post_kernel takes pair (a, c) in round
    (a * n + c) // 256 of thread (a * n + c) % 256, so with n = 64 the pair (0, 4) belongs to round 0 and the pair (4, 5) to
    round 1 of the same wave: B is already marked when B-C is looked at, and must remove C all the same.  (With 3 rows all
    pairs are looked at in one round, where a kernel that skipped removed rows would not show.)
    -> (seed, (joints, cam, pad)) for the first of at most 20 seeds that satisfies scene_conditions, or None."""
    c = edge_scenes(golden_dir)['chain']
    for seed in range(7000, 7020):
        joints, cam, _ = random_scene(seed, 64)
        for row, k in ((0, 0), (4, 1), (5, 2)):
            joints[row], cam[row] = c['joints'][k], c['cam'][k]
        if scene_conditions(joints, cam, c['pad'])[0]:
            return seed, (joints, cam, c['pad'])
    return None


def test_bev_post_chain_in_crowd(golden_dir):
    found = chain_in_crowd(golden_dir)
    assert found is not None
    joints, cam, pad = found[1]
    nms_only = lambda rows: PO.postprocess(joints[rows], cam[rows], pad, NMS, 1e9, dtype=np.float64)['keep']
    every = np.arange(64)
    keep = nms_only(every)
    assert keep[0] and not keep[4] and not keep[5]
    assert nms_only(every != 4)[5 - 1]                                                     # without B, C stays: C goes through B alone
    without_a = nms_only(every != 0)
    assert without_a[4 - 1] and not without_a[5 - 1]                                       # without A, B stays (and removes C)
