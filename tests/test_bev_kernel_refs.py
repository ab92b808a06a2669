"""CPU checks of oracle/bev_kernels_ref.py: the float64 / float32 restatements that tests/test_gpu_bev_kernels.py judges the
BEV head's kernels by are themselves pinned to the oracle (oracle/bev_oracle.py), to torch, and to the reference's own
outputs in tests/golden/bev_edges.npz (written by oracle/make_golden_bev_edges.py).  No GPU needed."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import bev_kernels_ref as K
from oracle import bev_oracle as BO


def _block_sd(C, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for cv, bn in (('conv1', 'bn1'), ('conv2', 'bn2')):
        sd[f'{cv}.weight'] = (torch.rand(C, C, 3, 3, 3, generator=g) * 2 - 1) / (27 * C) ** 0.5
        sd[f'{bn}.weight'] = torch.rand(C, generator=g) + 0.5
        sd[f'{bn}.bias'] = torch.randn(C, generator=g) * 0.1
        sd[f'{bn}.running_mean'] = torch.randn(C, generator=g) * 0.1
        sd[f'{bn}.running_var'] = torch.rand(C, generator=g) + 0.5
    return sd


def test_refiner_ref_vs_oracle_block3d():
    """float64 conv3d / refiner == BO._block3d (float32, unfolded BN) to float32 rounding, on a cropped volume."""
    for C in (1, 3):
        sd = _block_sd(C, 10 + C)
        x = torch.randn(2, C, 12, 20, 24, generator=torch.Generator().manual_seed(C))
        s1, b1 = K.bn_fold(sd, 'bn1')
        s2, b2 = K.bn_fold(sd, 'bn2')
        y, bound = K.refiner_ref(x, sd['conv1.weight'], s1, b1, sd['conv2.weight'], s2, b2)
        ref = BO._block3d(x, sd, '')
        err = (y - ref.double()).abs()
        print(f'C={C}: refiner_ref vs _block3d max-abs {err.max():.3e}, bound max {bound.max():.3e}')
        # the oracle's float32 block also divides by sqrt(var + eps) per voxel: a few more roundings than the folded form
        assert (err <= 2 * bound + 8 * K.U * ref.double().abs()).all()
        assert err.max() < 5e-6


def test_conv3d_bound_is_a_bound():
    """A float32 F.conv3d of mixed-magnitude data stays inside the derived per-voxel bound of the float64 result."""
    g = torch.Generator().manual_seed(3)
    C = 3
    x = torch.randn(1, C, 10, 16, 16, generator=g) * 10.0 ** (torch.rand(1, C, 10, 16, 16, generator=g) * 6 - 3)
    w = torch.randn(C, C, 3, 3, 3, generator=g)
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g)
    y, bound = K.conv3d_ref(x, w, sc, sh, x, True)
    y32 = torch.relu(F.conv3d(x, w, None, padding=1) * sc.view(1, C, 1, 1, 1) + sh.view(1, C, 1, 1, 1) + x)
    ratio = ((y32.double() - y).abs() / bound).max().item()
    print('float32 torch conv3d: largest err / bound %.3f' % ratio)
    assert ratio <= 1.0
    assert x.abs().max() > 100 and (y < 0).sum() == 0


def test_impulse_scatter_vs_conv3d_exact():
    """The flipped-kernel scatter IS the 3-D cross-correlation of the impulse volume: exact in float64, every set of sites."""
    sets = K.impulse_sites(3, seed=1)
    for s in sets:
        for i, p in enumerate(s):
            for q in s[:i]:
                assert max(abs(p[0] - q[0]), abs(p[1] - q[1]), abs(p[2] - q[2])) >= 3
    for C, ci in ((1, 0), (3, 0), (3, 2)):
        w = K.distinct_weights(C, seed=C)
        assert len(set(w.reshape(-1).tolist())) == 27 * C * C
        sites = sets[:2] if C == 1 else sets[2:]
        x = K.impulse_volume(sites, C, ci)
        exp = K.impulse_expected(sites, w, ci)
        ref = F.conv3d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), None, padding=1).numpy()
        assert np.array_equal(exp.astype(np.float64), ref)
        assert exp[:, :, 0].any() and exp[:, :, 63].any() and exp[..., 0].any() and exp[..., 127].any()


def test_maps_ref_vs_oracle_localization():
    """bev_maps_ref reproduces the centre / camera volumes the oracle builds inside coarse2fine_localization (model.py:195-196,
    209-212), bit for bit, on random front-view / bird's-eye-view maps."""
    g = torch.Generator().manual_seed(8)
    B = 2
    center_fv, cam_off = torch.randn(B, 1, 128, 128, generator=g), torch.randn(B, 3, 128, 128, generator=g)
    bv = torch.randn(B, 128, 128, generator=g) * 3
    center_bv, cam_off_bv = bv[:, :64], bv[:, 64:]
    c3 = center_fv.repeat(1, 64, 1, 1) * center_bv.unsqueeze(2).repeat(1, 1, 128, 1)
    cam = BO.coordmap_3d() + cam_off.unsqueeze(-1).transpose(4, 1).contiguous()
    cam[:, :, :, :, 2] = cam[:, :, :, :, 2] + cam_off_bv.unsqueeze(2).contiguous()
    cam = cam.unsqueeze(1).transpose(5, 1).squeeze(-1)
    c3r, camr = K.bev_maps_ref(center_fv[:, 0].numpy(), cam_off.numpy(), center_bv.numpy(), cam_off_bv.numpy())
    assert np.array_equal(c3r, c3.numpy())
    assert np.array_equal(camr, cam.numpy())
    # the order matters: the other association differs somewhere on this data
    r = (np.arange(128, dtype=np.float32) / np.float32(128) * np.float32(2) - np.float32(1))[None, None, None, :]
    other = r + (cam_off[:, 2].numpy()[:, None] + cam_off_bv.numpy()[:, :, None, :])
    assert not np.array_equal(other, camr[:, 2])


def test_maps_ref_vs_reference_samples(golden_dir):
    """Through the oracle: its pre-refiner volumes equal bev_maps_ref of its own maps, and its refined volumes match the reference's
    samples in bev_b1.npz (so the restatement sits on the path the reference's numbers came from)."""
    from oracle import romp_oracle as O
    g = np.load(os.path.join(golden_dir, 'bev_b1.npz'))
    sd = BO.make_bev_state_dict(0)
    x = O.backbone_forward(sd, O.make_images(1, seed=4))
    maps_fv = F.conv2d(BO._head_block(x, sd, 'det_head.0.0.'), sd['det_head.1.weight'], sd['det_head.1.bias'])
    f = x
    for i, pad in zip((0, 3, 6), (0, 1, 0)):
        f = torch.relu(BO._bn(F.conv2d(f, sd[f'bv_pre_layers.{i}.weight'], sd[f'bv_pre_layers.{i}.bias'], padding=pad), sd, f'bv_pre_layers.{i + 1}'))
    packed = K.bev_pack_ref(maps_fv, f)                                     # (1, W, 2560)
    bv = packed.permute(0, 2, 1)
    assert torch.equal(bv, torch.cat([maps_fv, f], 1).reshape(1, -1, 128))
    for i in range(3):
        bv = BO._block1d(bv, sd, f'bv_out_layers.{i}.')
    c3, cam = K.bev_maps_ref(maps_fv[:, 0].numpy(), maps_fv[:, 1:4].numpy(), bv[:, :64].numpy(), bv[:, 64:].numpy())
    c3 = BO._block3d(torch.from_numpy(c3).unsqueeze(1), sd, 'center_map_refiner.0.').squeeze(1).numpy()
    cam = BO._block3d(torch.from_numpy(cam), sd, 'cam_map_refiner.0.').numpy()
    co, mo, _ = BO.coarse2fine_localization(sd, x)
    assert np.array_equal(c3, co.numpy()) and np.array_equal(cam, mo.numpy())
    e1 = np.abs(c3[0].reshape(-1)[g['sample_pos']] - g['center3d_samples']).max()
    e2 = np.abs(cam[0].reshape(3, -1)[:, g['sample_pos']] - g['cam3d_samples']).max()
    print(f'vs reference samples: center3d {e1:.3e} cam3d {e2:.3e}')
    assert e1 < 1e-5 and e2 < 1e-5


def test_mlp_bound_holds_for_float32_numpy():
    rs = np.random.RandomState(0)
    x = rs.randn(16, 128).astype(np.float32)
    layers = [((rs.randn(o, i) / np.sqrt(i)).astype(np.float32), (rs.randn(o) * 0.1).astype(np.float32)) for i, o in ((128, 512), (512, 512), (512, 143))]
    y, e = K.mlp_ref(x, layers)
    h = x
    for k, (W, b) in enumerate(layers):
        h = h @ W.T + b
        h = np.maximum(h, 0) if k < 2 else h
    assert h.dtype == np.float32
    ratio = (np.abs(h - y) / e).max()
    print('float32 numpy MLP: largest err / bound %.3f (bound max %.2e)' % (ratio, e.max()))
    assert ratio <= 1.0 and e.max() < 0.1          # (a worst-case bound: three layers of |W| amplification)


def test_edges_fixture_vs_oracle(golden_dir):
    """tests/golden/bev_edges.npz (the reference's own outputs) against the oracle: cam -> centre coordinates exactly, cam ->
    translation to float32 rounding of a possibly cancelling denominator, the planted-peak parses exactly."""
    path = os.path.join(golden_dir, 'bev_edges.npz')
    assert os.path.getsize(path) < 200 * 1024
    g = np.load(path)
    assert all(g[k].dtype.kind in 'fiu' for k in g.files)
    cams = K.edge_cams()
    assert np.array_equal(cams, g['cams'])
    assert np.array_equal(BO.cam_to_czyx(cams), g['cam_czyx'])
    z = g['cam_czyx']
    assert z.min() == 1 and z.max() == 127 and set(range(1, 64)) <= set(z[:, 0].tolist())
    ref = K.cam_trans_ref(cams)
    kappa = (np.abs(cams[:, 0].astype(np.float64)) * BO.TAN_FOV + 1e-3) / np.abs(cams[:, 0].astype(np.float64) * BO.TAN_FOV + 1e-3)
    tol = 8 * K.U * kappa[:, None] * np.abs(ref)
    assert (np.abs(g['cam_trans'].astype(np.float64) - ref) <= tol).all()
    assert (np.abs(BO.cam_to_trans(cams).astype(np.float64) - ref) <= tol).all()
    assert np.abs(ref[:, 2]).max() > 5e4 and (ref[:, 2] < 0).any() and kappa.max() > 100
    cases = K.edge_parse_cases()
    assert sorted(cases) == sorted(k[6:-5] for k in g.files if k.startswith('parse_') and k.endswith('_meta'))
    for name, case in cases.items():
        meta = g[f'parse_{name}_meta']
        assert [case['B'], case['seed'], case['background'][0], case['background'][1], case['thresh'], case['max_person']] == meta.tolist()
        assert np.array_equal(np.array(case['peaks'], np.float64), g[f'parse_{name}_peaks'])
        cm = K.planted_volume(case['B'], case['seed'], case['peaks'], case['background'])
        b, zyx, s = BO.parse_3dcentermap(cm, case['thresh'], case['max_person'])
        assert np.array_equal(b, g[f'parse_{name}_bids'])
        assert np.array_equal(zyx, g[f'parse_{name}_czyx'])
        assert np.array_equal(s, g[f'parse_{name}_confs'])
    assert len(g['parse_border_bids']) == 26 + 13 and len(g['parse_threshold_bids']) == 3


def test_anchor_ties_exist_and_oracle_takes_the_lower_index():
    ties = K.anchor_tie_scales()
    print('float32 anchor ties found:', len(ties))
    assert len(ties) > 0
    for s, k in ties:
        assert BO.cam_to_czyx(np.array([[s, 0, 0]], np.float32))[0, 0] == max(k, 1)          # (depth index 0 clamps to 1)
