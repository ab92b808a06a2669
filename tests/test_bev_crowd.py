"""BEV crowd mode (bev/main.py:184-258, bev/split2process.py): the long-image sliding window.

CPU part: the numpy restatement of the crop plan and of the merge (tests/crowd_cases.py: boundary exclusion, per-crop projection, conf-based
suppression and outlier removal, the full-frame camera, the global suppression / outlier pass) matches the fixture that
the reference's own process_long_image produced (tests/golden/bev_crowd.npz, scripts/make_golden_bev_crowd.py); the
settings and the two C-ABI entry points exist.

GPU part (-m gpu): romp_preprocess_crops is bit-identical to the oracle pre-processing of each crop cut from the padded
frame; romp_bev_crowd_merge matches the fixture and the restatement (also with more than 64 people in a crop and more
than 256 rows in the global stage); BEV(--crowd) end to end equals the restatement applied to the per-crop detections the
device itself produced.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crowd_cases import F32, crop_pad_info, crowd_merge, frame_pad_info, split_plan  # noqa: E402  (the numpy restatement)


def _cases(golden_dir):
    g = np.load(os.path.join(golden_dir, 'bev_crowd.npz'))
    return [{k[len('c%d_' % i):]: g[k] for k in g.files if k.startswith('c%d_' % i)} for i in range(int(g['n_cases']))]


def _check_merge(res_keep, cam_full, cam_trans, pj2d_org, case):
    kept = np.nonzero(res_keep)[0]
    assert kept.tolist() == case['kept'].tolist()
    np.testing.assert_allclose(cam_full[kept], case['cam_full'], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(cam_trans[kept], case['cam_trans'], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(pj2d_org[kept], case['pj2d_org'], rtol=0, atol=2e-3)


# ----------------------------------------------------------------------------------------------------- CPU tests
def test_crowd_settings():
    from romp_amd import bev
    s = bev.bev_settings(['--crowd'])
    assert s.crowd and (s.center_thresh, s.nms_thresh, s.overlap_ratio, s.relative_scale_thresh) == (0.08, 20, 0.8, 1.6)
    s = bev.bev_settings(['--crowd', '--model_id', '1'])
    assert (s.center_thresh, s.overlap_ratio, s.relative_scale_thresh) == (0.12, 0.46, 1.6)   # the reference's model_id quirk
    s = bev.bev_settings([])
    assert not s.crowd and (s.center_thresh, s.overlap_ratio) == (0.1, 0.8)                  # off by default here
    assert bev.bev_settings(['--show_patch_results']).show_patch_results


def test_crowd_symbols_exported():
    from romp_amd import lib as L
    assert 'romp_preprocess_crops' in L.EXPORTS and 'romp_bev_crowd_merge' in L.EXPORTS and len(L.EXPORTS) == 52
    h = L.load()
    assert hasattr(h, 'romp_preprocess_crops') and hasattr(h, 'romp_bev_crowd_merge')


def test_crowd_plan_matches_fixture(golden_dir):
    from romp_amd import bev
    widths = set()
    for case in _cases(golden_dir):
        H, W, ov = int(case['H']), int(case['W']), float(case['overlap'])
        pl = int(case['pad_length'])
        assert pl == bev.crowd_pad_length(H, ov) == int(H * ov)
        plan = bev.crowd_split_plan(H, W + 2 * pl, ov)
        assert np.array_equal(plan, case['crops']) and np.array_equal(split_plan(H, W + 2 * pl, ov), case['crops'])
        assert np.array_equal(case['crop_shapes'], np.stack([plan[:, 3] - plan[:, 2], plan[:, 1] - plan[:, 0]], 1))
        assert np.array_equal(np.stack([crop_pad_info(h, w) for h, w in case['crop_shapes']]), case['crop_pads'])
        assert np.array_equal(frame_pad_info(H, W), case['pad_info']) and bev.crowd_pad_info(H, W) == case['pad_info'].tolist()
        widths |= set((plan[:, 1] - plan[:, 0] - H).tolist())
    assert min(widths) < 0 and max(widths) == 1                  # a narrow last crop and h + 1 wide crops are covered
    assert len(split_plan(300, 4000 + 2 * 240, 0.8)) == 71 and split_plan(512, 1280 + 2 * 409, 0.8)[-1].tolist()[:2] == [1586, 2047]


def test_crowd_restatement_matches_fixture(golden_dir):
    totals = dict(excluded=0, crop_suppressed=0, crop_outliers=0, suppressed=0, outliers=0)
    for case in _cases(golden_dir):
        r = crowd_merge(case['crop_id'], case['cam'], case['center_confs'], case['joints'], case['crops'], int(case['H']),
                        int(case['W']), int(case['pad_length']))
        _check_merge(r['keep'], r['cam_full'], r['cam_trans'], r['pj2d_org'], case)
        assert r['margin'] > 1e-4, r['margin']                  # nothing on the edge of a threshold: row sets are exact
        for k, v in r['stages'].items():
            totals[k] += v
    assert all(v > 0 for v in totals.values()), totals          # every step of the merge removed someone
    tails = [c for c in _cases(golden_dir) if (c['crop_id'] == len(c['crops']) - 1).sum() == 0]
    assert tails                                                # ... and a trailing crop with nobody is covered


# ----------------------------------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def _crops_c(crops):
    import ctypes as C
    a = np.ascontiguousarray(crops, np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def device_merge(dev, crop_id, cam, conf, joints, crops, H, W, pad_length, nms=20., rel=1.6, capacity=None):
    from romp_amd import lib as L
    lib = L.load()
    N, K = len(cam), len(crops)
    cap = capacity or N
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    counts = np.bincount(np.asarray(crop_id), minlength=K)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
    out = {k: torch.full(s, -7., device=dev) for k, s in (('cam', (cap, 3)), ('trans', (cap, 3)), ('pj', (cap, 71, 2)))}
    keep = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    ws = torch.full((4 * cap + 4,), -1, dtype=torch.int32, device=dev)
    arr, cp = _crops_c(crops)
    dj, dc, dconf = t(joints), t(cam), t(conf)                          # (held: a temporary's memory could be reused at once)
    L.check(lib.romp_bev_crowd_merge(L.ptr(dj), L.ptr(dc), L.ptr(dconf), L.ptr(offsets), N, cap, K, cp, H, W,
                                     pad_length, nms, rel, L.ptr(out['cam']), L.ptr(out['trans']), L.ptr(out['pj']), L.ptr(keep),
                                     L.ptr(ws), L.stream_ptr(dev)))
    torch.cuda.synchronize()
    return keep.cpu().numpy()[:N].astype(bool), out['cam'].cpu().numpy()[:N], out['trans'].cpu().numpy()[:N], out['pj'].cpu().numpy()[:N]


@pytest.mark.gpu
def test_crowd_preprocess_bit_exact(dev):
    import ctypes as C
    from oracle import cv_resize_oracle as CV
    from romp_amd import lib as L
    lib = L.load()
    rs = np.random.RandomState(0)
    for H, W, ov in ((512, 1280, 0.8), (720, 2560, 0.8), (1080, 2160, 0.8), (200, 700, 0.46)):
        frame = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        pl = int(H * ov)
        crops = split_plan(H, W + 2 * pl, ov)
        K = len(crops)
        out = torch.full((K, 512, 512, 3), -1., device=dev)
        pads = (C.c_float * (6 * K))()
        arr, cp = _crops_c(crops)
        dframe = torch.from_numpy(frame).to(dev)
        L.check(lib.romp_preprocess_crops(L.ptr(dframe), H, W, pl, K, cp, L.ptr(out), 512, pads,
                                          L.stream_ptr(dev)))
        got = out.cpu().numpy()
        padded = np.zeros((H, W + 2 * pl, 3), np.uint8)
        padded[:, pl:pl + W] = frame
        widths = set()
        for c, (l, r, t, b) in enumerate(crops):
            ref, info = CV.img_preprocess(padded[t:b, l:r])
            assert np.array_equal(got[c], ref[0]), (H, W, c)
            assert np.array_equal(np.array(pads[6 * c:6 * c + 6], np.float32), info)
            widths.add(int(r - l) - H)
        print('%dx%d: %d crops, widths - h %s' % (H, W, K, sorted(widths)))
        assert min(widths) < 0
    rc = lib.romp_preprocess_crops(L.ptr(out), 10, 30, 5, 1, _crops_c([[0, 41, 0, 10]])[1], L.ptr(out), 512, None,
                                   L.stream_ptr(dev))
    assert rc == -1 and b'padded frame' in lib.romp_last_error()


@pytest.mark.gpu
def test_crowd_merge_matches_fixture(dev, golden_dir):
    for case in _cases(golden_dir):
        res = device_merge(dev, case['crop_id'], case['cam'], case['center_confs'], case['joints'], case['crops'], int(case['H']),
                           int(case['W']), int(case['pad_length']))
        _check_merge(*res, case)


def _random_detections(rs, H, W, ov, per_crop, spread):
    pl = int(H * ov)
    crops = split_plan(H, W + 2 * pl, ov)
    K = len(crops)
    counts = rs.randint(per_crop[0], per_crop[1] + 1, K)
    crop_id = np.repeat(np.arange(K), counts).astype(np.int32)
    N = len(crop_id)
    cam = np.stack([rs.uniform(0.2, 1.2, N), rs.uniform(-0.5, 0.5, N), rs.uniform(-1.1, 1.1, N)], 1).astype(F32)
    cam[rs.rand(N) < 0.1, 0] = 0.04                                     # some remote persons
    base = (rs.randn(8, 71, 3) * [0.25, 0.45, 0.1]).astype(F32)
    joints = (base[rs.randint(0, 8, N)] + rs.randn(N, 71, 3) * spread).astype(F32)
    conf = rs.uniform(0.05, 0.95, N).astype(F32)
    return crop_id, cam, conf, joints, crops, pl


@pytest.mark.gpu
@pytest.mark.parametrize('H,W,ov,per_crop,spread', [(512, 1280, 0.8, (70, 90), 0.03), (720, 2560, 0.8, (10, 20), 0.02),
                                                    (300, 1500, 0.46, (0, 6), 0.05)])
def test_crowd_merge_random_vs_restatement(dev, H, W, ov, per_crop, spread):
    for seed in range(H + W, H + W + 20):                               # (inputs with a value within 1e-5 of a threshold skipped)
        crop_id, cam, conf, joints, crops, pl = _random_detections(np.random.RandomState(seed), H, W, ov, per_crop, spread)
        r = crowd_merge(crop_id, cam, conf, joints, crops, H, W, pl)
        if r['margin'] > 1e-5:
            break
    assert r['margin'] > 1e-5
    keep, cf, tr, pj = device_merge(dev, crop_id, cam, conf, joints, crops, H, W, pl, capacity=len(cam) + 5)
    counts = np.bincount(crop_id, minlength=len(crops))
    survivors_crop_stage = int(r['keep'].sum() + r['stages']['suppressed'] + r['stages']['outliers'])
    print('%dx%d: %d rows, max per crop %d, crop-stage survivors %d, kept %d, stages %s'
          % (H, W, len(cam), counts.max(), survivors_crop_stage, r['keep'].sum(), r['stages']))
    assert keep.tolist() == r['keep'].tolist()
    k = r['keep']
    np.testing.assert_allclose(cf[k], r['cam_full'][k], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(tr[k], r['cam_trans'][k], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(pj[k], r['pj2d_org'][k], rtol=0, atol=2e-3)
    if per_crop[0] > 64:                                                # > 64 people in a crop, > 256 rows in the global stage
        assert counts.max() > 64 and survivors_crop_stage > 256
        assert r['stages']['crop_suppressed'] > 0 and r['stages']['suppressed'] > 0 and r['stages']['outliers'] > 0


@pytest.mark.gpu
def test_crowd_merge_rejects_bad_arguments(dev):
    from romp_amd import lib as L
    lib = L.load()
    x = torch.zeros(16, device=dev)
    ws = torch.zeros(64, dtype=torch.int32, device=dev)
    _, good = _crops_c([[0, 10, 0, 10], [5, 15, 0, 10]])
    _, bad = _crops_c([[0, 10, 0, 10], [5, 31, 0, 10]])
    call = lambda N, cap, K, cp: lib.romp_bev_crowd_merge(L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(ws), N, cap, K, cp, 10, 20, 5, 20.,
                                                          1.6, L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(ws), L.ptr(ws),
                                                          L.stream_ptr(dev))
    assert call(0, 4, 0, good) == -1
    assert call(5, 4, 2, good) == -1 and b'capacity' in lib.romp_last_error()
    assert call(2, 4, 2, bad) == -1 and b'padded frame' in lib.romp_last_error()
    assert call(0, 4, 2, good) == 0


def _bev_model(dev, *flags, max_batch=4):
    from oracle import bev_oracle as BO
    from oracle import romp_oracle as O
    from romp_amd import bev
    s = bev.bev_settings(list(flags))
    s.GPU, s.max_batch = 0, max_batch
    return s, bev.BEV(s, state_dict=BO.make_bev_state_dict(0), smpla_model=O.make_synthetic_smpl(0, 11),
                      smil_model=O.make_synthetic_smpl(5, 10))


def _wide_frame(seed, H=160, W=480):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)


class _Spy:
    """Stands in for BEV.model (BEVv1): records what every network chunk detected."""

    def __init__(self, inner):
        self.inner, self.net, self.seen = inner, inner.net, []

    def __call__(self, images):
        out = self.inner(images)
        self.seen.append(None if out is None else {k: out[k].clone() for k in ('cam', 'center_confs', 'pred_batch_ids')})
        return out


class _SmplSpy(torch.nn.Module):
    """Stands in for BEV.smpl_parser: records the rows it was called with and the joints it returned."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.calls = inner, []

    def forward(self, betas, thetas):
        v, j, f = self.inner(betas, thetas)
        self.calls.append((betas.cpu().numpy(), thetas.cpu().numpy(), j.cpu().numpy()))
        return v, j, f


@pytest.mark.gpu
def test_bev_crowd_end_to_end(dev):
    from oracle import bev_oracle as BO
    from oracle import romp_oracle as O
    s, model = _bev_model(dev, '--crowd')
    frame = _wide_frame(1)
    H, W = frame.shape[:2]
    pl = int(H * s.overlap_ratio)
    crops = split_plan(H, W + 2 * pl, s.overlap_ratio)
    assert len(crops) > s.max_batch                                   # the crops take at least two network chunks
    net = model.model = _Spy(model.model)
    smpl = model.smpl_parser = _SmplSpy(model.smpl_parser)
    for thresh in (0.9995, 0.999, 0.99, 0.9, 0.5, 0.2):              # the highest threshold that still sees a few people
        net.inner.centermap_parser.conf_thresh = thresh
        net.seen.clear()
        smpl.calls.clear()
        res = model(frame)
        n_det = sum(0 if o is None else len(o['cam']) for o in net.seen)
        if res is not None and n_det >= 6:
            break
    print('center threshold %g: %d chunks, %d detections, %d merged' % (thresh, len(net.seen), n_det, len(res['cam'])))
    assert len(net.seen) == -(-len(crops) // s.max_batch) and len(smpl.calls) == 1          # one SMPL call over all rows
    crop_id = np.concatenate([o['pred_batch_ids'].cpu().numpy() + i * s.max_batch for i, o in enumerate(net.seen) if o is not None])
    cam = np.concatenate([o['cam'].cpu().numpy() for o in net.seen if o is not None])
    conf = np.concatenate([o['center_confs'].cpu().numpy() for o in net.seen if o is not None])
    betas, thetas, joints = smpl.calls[0]
    r = crowd_merge(crop_id, cam, conf, joints, crops, H, W, pl, nms=s.nms_thresh, rel=s.relative_scale_thresh)
    assert r['margin'] > 1e-5, r['margin']
    k = np.nonzero(r['keep'])[0]
    assert sorted(res.keys()) == sorted(['smpl_thetas', 'smpl_betas', 'cam', 'cam_trans', 'params_pred', 'center_confs',
                                         'pred_batch_ids', 'verts', 'joints', 'pj2d_org'])
    assert len(res['cam']) == len(k) >= 1 and res['pred_batch_ids'].dtype == np.int64 and np.all(res['pred_batch_ids'] == 0)
    assert np.array_equal(res['smpl_thetas'], thetas[k]) and np.array_equal(res['center_confs'], conf[k])
    assert np.array_equal(res['joints'], joints[k])
    np.testing.assert_allclose(res['cam'], r['cam_full'][k], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(res['cam_trans'], r['cam_trans'][k], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(res['pj2d_org'], r['pj2d_org'][k], rtol=0, atol=2e-3)
    vo, _ = BO.smpla_forward(O.make_synthetic_smpl(0, 11), O.make_synthetic_smpl(5, 10), betas[k], thetas[k])
    assert np.abs(res['verts'] - vo).max() < 1e-4
    net.inner.centermap_parser.conf_thresh = 1e3                      # nobody anywhere -> None
    assert model(frame) is None


@pytest.mark.gpu
def test_bev_crowd_narrow_image_unchanged(dev):
    s, model = _bev_model(dev, '--crowd')
    frame = _wide_frame(2, 240, 470)                                  # aspect < 2: the normal path, crowd or not
    outs = []
    for crowd in (True, False):
        model.settings.crowd = crowd
        for thresh in (0.999, 0.99, 0.9, 0.5, 0.2):
            model.model.centermap_parser.conf_thresh = thresh
            if model(frame) is not None:
                break
        outs.append(model(frame))
    assert outs[0] is not None and sorted(outs[0]) == sorted(outs[1])
    for key in outs[0]:
        assert np.array_equal(outs[0][key], outs[1][key]), key


@pytest.mark.gpu
def test_bev_crowd_render(dev):
    from oracle import bev_oracle as BO
    from oracle import romp_oracle as O
    from oracle import sim3dr_oracle as SO
    from romp_amd import bev
    from romp_amd.vis import mesh_color_left2right
    s = bev.bev_settings(['--crowd', '--render_mesh'])
    s.GPU, s.max_batch = 0, 4
    _, base_tri = SO.ellipsoid_mesh(84, 82, [0, 0, 0], [1, 1, 1])
    faces = np.zeros((13776, 3), np.int64)
    faces[:len(base_tri)] = base_tri
    smpla = dict(O.make_synthetic_smpl(0, 11), f=torch.from_numpy(faces).float())
    smil = dict(O.make_synthetic_smpl(5, 10), f=torch.from_numpy(faces).float())
    model = bev.BEV(s, state_dict=BO.make_bev_state_dict(0), smpla_model=smpla, smil_model=smil)
    frame = _wide_frame(1)
    H, W = frame.shape[:2]
    for thresh in (0.9995, 0.999, 0.99, 0.9, 0.5, 0.2):
        model.model.centermap_parser.conf_thresh = thresh
        out = model(frame)
        if out is not None:
            break
    assert out is not None and 'rendered_image' in out and 'verts_camed_org' not in out and 'smpl_face' not in out
    assert out['rendered_image'].shape == (H, 2 * W, 3) and np.array_equal(out['rendered_image'][:, :W], frame)
    verts, tr = out['verts'].astype(F32), out['cam_trans'].astype(F32)
    p = verts + tr[:, None]
    z = p[..., 2] + F32(1e-6)
    px, py = p[..., 0] / z * F32(443.4) / F32(256), p[..., 1] / z * F32(443.4) / F32(256)
    pad, top = F32(W), F32((W - H) // 2)
    vorg = np.stack([(px + F32(1)) * pad / F32(2), (py + F32(1)) * pad / F32(2) - top, (verts[..., 2] + F32(1)) * pad / F32(2)],
                    -1).astype(F32)
    order = torch.sort(torch.from_numpy(tr[:, 2]), descending=True).indices.numpy()
    vorg = vorg[order]
    vorg[:, :, 2] *= -1
    colors = mesh_color_left2right(torch.from_numpy(tr))[order]
    ref = SO.render_meshes(vorg, faces.astype(np.int32), frame, colors, use_ref=SO.load_ref() is not None)
    nd = int((out['rendered_image'][:, W:] != ref).sum())
    print('%d people; rendered_image vs oracle: differing bytes %d, painted px %d' % (len(tr), nd, int((ref != frame).any(2).sum())))
    assert nd <= 3 * 8
