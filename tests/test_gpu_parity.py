"""GPU parity tests (run with -m gpu on the MI355X box): the HIP path, called through the
C ABI of libromp_hip.so, against the CPU oracle on identical seeded inputs and against the
committed reference-generated fixtures in tests/golden/.

Tolerances (float32 path):
  * SMPL verts / joints on identical theta/beta: 1e-4 max-abs (the north-star gate; measured
    float32 noise floor is ~3e-7)
  * network maps: 1e-4 max-abs on center_maps / params_maps (reference fp32-vs-fp64 noise floor
    is ~3e-6)
  * parse: index sets bit-exact, scores bit-exact; axis-angle 2e-5 except near-pi rotations,
    which are compared through the rotation matrix they encode.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import romp_oracle as O

pytestmark = pytest.mark.gpu


def _has_bx3():
    from romp_amd import lib
    return lib.has_bf16x3()


# the bf16x3 kernel family is an optional part of the library since round 6 (ROMP_WITH_BX3=1 python -m romp_amd.build): its
# parametrisations run in a build that has it
BX3 = pytest.param('bf16x3', marks=pytest.mark.skipif(not _has_bx3(), reason='library built without the bf16x3 family (ROMP_WITH_BX3=1)'))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from romp_amd import lib
    lib.load()                       # fail loudly if the HIP extension is missing
    return torch.device('cuda:0')


def _g(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


# ------------------------------------------------------------------------------ SMPL
@pytest.mark.parametrize('tag,nb', [('smpl', 10), ('smpla', 11)])
def test_smpl_golden(dev, golden_dir, tag, nb):
    from romp_amd.smpl import SMPL
    g = _g(golden_dir, f'{tag}_n4.npz')
    model = O.make_synthetic_smpl(seed=0, n_betas=nb)
    smpl = SMPL(model, model_type=tag).to(dev)
    for ra in (0, 1):
        v, j, f = smpl(g['betas'], g['poses'], root_align=bool(ra))
        assert v.shape == (4, 6890, 3) and j.shape == (4, 71, 3) and f.shape == (13776, 3)
        ev = np.abs(v.cpu().numpy() - g[f'verts_ra{ra}']).max()
        ej = np.abs(j.cpu().numpy() - g[f'joints_ra{ra}']).max()
        print(f'{tag} root_align={ra}: verts max-abs {ev:.3e} joints {ej:.3e}')
        assert ev < 1e-4 and ej < 1e-4


@pytest.mark.parametrize('N', [1, 7, 64, 200])
def test_smpl_vs_oracle(dev, N):
    from romp_amd.smpl import SMPL
    model = O.make_synthetic_smpl(seed=0)
    smpl = SMPL(model).to(dev)
    g = torch.Generator().manual_seed(0)
    betas = torch.randn(N, 10, generator=g)
    poses = 0.3 * torch.randn(N, 72, generator=g)
    v, j, _ = smpl(betas, poses)
    vo, jo, _ = O.smpl_forward(model, betas.numpy(), poses.numpy())
    ev, ej = np.abs(v.cpu().numpy() - vo).max(), np.abs(j.cpu().numpy() - jo).max()
    print(f'N={N}: verts {ev:.3e} joints {ej:.3e}')
    assert ev < 1e-4 and ej < 1e-4


def test_smpl_properties_full_size(dev):
    """Config-2 worst case (32 images x 64 persons = 2048 meshes): size-independent properties.
    (a) zero pose: verts == v_template + shapedirs.beta;  (b) a global rotation R0 about the root
    joint rotates the mesh rigidly: verts' = R0 (verts - J0) + J0."""
    from romp_amd.smpl import SMPL
    model = O.make_synthetic_smpl(seed=0)
    smpl = SMPL(model).to(dev)
    N = 2048
    g = torch.Generator().manual_seed(4)
    betas = torch.randn(N, 10, generator=g)
    v0, j0, _ = smpl(betas, torch.zeros(N, 72))
    vs = model['v_template'][None] + torch.einsum('bl,mkl->bmk', betas, model['shapedirs'])
    assert (v0.cpu() - vs).abs().max() < 2e-5
    poses = 0.3 * torch.randn(N, 72, generator=g)
    poses[:, :3] = 0
    v1, j1, _ = smpl(betas, poses)
    aa = torch.randn(N, 3, generator=g)
    poses2 = poses.clone()
    poses2[:, :3] = aa
    v2, j2, _ = smpl(betas, poses2)
    R0 = torch.from_numpy(O.batch_rodrigues(aa.numpy()))
    J0 = j1[:, 0:1].cpu()
    v_exp = torch.einsum('nij,nvj->nvi', R0, v1.cpu() - J0) + J0
    assert (v2.cpu() - v_exp).abs().max() < 5e-5


# ------------------------------------------------------------------------------ parse
def test_rot6d_golden(dev, golden_dir):
    from romp_amd.post_parser import rot6D_to_angular
    g = _g(golden_dir, 'rot6d_cases.npz')
    aa = rot6D_to_angular(torch.from_numpy(g['x']).to(dev)).cpu().numpy()
    assert np.isfinite(aa).all()
    err = np.abs(aa - g['aa']).max(1)
    loose = err > 2e-5
    print('rot6d: max err', err.max(), 'ill-conditioned cases', int(loose.sum()))
    assert loose.sum() <= 12
    np.testing.assert_allclose(O.batch_rodrigues(aa[loose]), O.batch_rodrigues(g['aa'][loose]), atol=2e-3)


def _parse_inputs():
    gen = torch.Generator().manual_seed(11)
    cm = torch.rand(3, 1, 64, 64, generator=gen)
    pm = torch.randn(3, 145, 64, 64, generator=gen)
    cm[2] *= 0.2
    return cm, pm


def test_parse_golden(dev, golden_dir):
    from romp_amd.post_parser import CenterMap, parsing_outputs
    g = _g(golden_dir, 'parse_b3.npz')
    cm, pm = _parse_inputs()
    parser = CenterMap(float(g['thresh']))
    out, bids = parsing_outputs(cm.to(dev), pm.permute(0, 2, 3, 1).contiguous().to(dev), parser, return_batch_ids=True)
    assert np.array_equal(bids.cpu().numpy(), g['batch_ids'])
    assert np.array_equal(out['center_preds'].cpu().numpy(), g['center_preds'])
    assert out['center_preds'].dtype == torch.int64
    assert np.array_equal(out['center_confs'].cpu().numpy(), g['center_confs'])
    np.testing.assert_allclose(out['cam'].cpu().numpy(), g['cam'], rtol=2e-6, atol=1e-6)
    assert np.array_equal(out['smpl_betas'].cpu().numpy(), g['smpl_betas'])
    np.testing.assert_allclose(out['smpl_thetas'].cpu().numpy(), g['smpl_thetas'], atol=5e-5)
    np.testing.assert_allclose(out['body_pose'].cpu().numpy(), g['body_pose'], atol=5e-5)
    np.testing.assert_allclose(out['global_orient'].cpu().numpy(), g['global_orient'], atol=5e-5)
    # NCHW view input gives the same answer
    out2 = parsing_outputs(cm.to(dev), pm.to(dev), parser)
    assert torch.equal(out2['smpl_thetas'], out['smpl_thetas'])
    # nobody detected -> None (post_parser.py:138-140)
    assert parsing_outputs(cm.to(dev) * 0.01, pm.to(dev), parser) is None


@pytest.mark.parametrize('B,thresh', [(1, 0.9), (32, 0.5), (32, 0.995), (5, 0.0)])
def test_parse_vs_oracle(dev, B, thresh):
    """Includes the saturated case (64 persons in every image) and ties/plateaus."""
    from romp_amd.post_parser import CenterMap, parsing_outputs
    gen = torch.Generator().manual_seed(B)
    cm = torch.rand(B, 1, 64, 64, generator=gen)
    cm[0, 0, 10:13, 10:13] = 2.0                      # a 3x3 plateau: all 9 are maxima (exact equality)
    cm[-1, 0, 40, 40] = 2.0                           # ties across positions
    pm = torch.randn(B, 145, 64, 64, generator=gen)
    ref = O.parsing_outputs(cm.numpy(), pm.numpy(), thresh)
    out, bids = parsing_outputs(cm.to(dev), pm.to(dev), CenterMap(thresh), return_batch_ids=True)
    assert np.array_equal(bids.cpu().numpy(), ref['batch_ids'])
    assert np.array_equal(out['center_preds'].cpu().numpy(), ref['center_preds'])
    assert np.array_equal(out['center_confs'].cpu().numpy()[:, 0], ref['scores'])
    np.testing.assert_allclose(out['cam'].cpu().numpy(), ref['cam'], rtol=2e-6, atol=1e-6)
    d = np.abs(out['smpl_thetas'].cpu().numpy() - ref['smpl_thetas']).reshape(-1, 3).max(1)
    assert (d > 5e-5).mean() < 0.01                   # near-pi rotations are ill-conditioned


# ------------------------------------------------------------------------------ conv layers
CONV_CASES = [
    # (Cin, Cout, k, stride, H, relu, residual)
    (32, 32, 3, 1, 128, True, True), (64, 64, 3, 1, 64, True, False), (128, 128, 3, 1, 32, True, True),
    (256, 256, 3, 1, 16, True, True), (256, 32, 3, 1, 128, True, False), (64, 64, 3, 2, 256, True, False),
    (256, 64, 3, 2, 128, True, False), (32, 64, 3, 2, 128, False, False), (32, 32, 3, 2, 128, True, False),
    (64, 128, 3, 2, 64, False, False), (128, 256, 3, 2, 32, False, False), (32, 256, 3, 2, 32, False, False),
    (40, 192, 3, 2, 128, True, False), (48, 192, 3, 2, 128, True, False),
    # merged sibling convs of the fuse layers (plan.hr_module, romp_op.relu_from): [no-ReLU channels | ReLU channels]
    (32, 96, 3, 2, 128, True, False, 64), (32, 128, 3, 2, 128, True, False, 64), (64, 192, 3, 2, 64, True, False, 128),
    (64, 64, 1, 1, 128, True, False), (64, 256, 1, 1, 128, False, False), (256, 64, 1, 1, 128, True, True),
    (64, 32, 1, 1, 64, False, False), (128, 32, 1, 1, 32, False, False), (256, 128, 1, 1, 16, False, False),
    (128, 96, 1, 1, 32, False, False), (256, 224, 1, 1, 16, False, False),     # merged up-convs (conv_h2k at B = 1)
    (64, 142, 1, 1, 64, False, False), (64, 1, 1, 1, 64, False, False), (64, 3, 1, 1, 64, False, False),
    # ResNet-50's Bottleneck 1x1 convs, layers 2-4 (resnet_50.py:64-78: C -> 4C + residual, 4C -> C, the strided downsample):
    # the shapes csrc/conv_h2g.hip was written for (K streamed in 64-channel stages)
    (256, 128, 1, 1, 64, True, False), (128, 512, 1, 1, 64, True, True), (512, 128, 1, 1, 64, True, False), (256, 512, 1, 2, 128, False, False),
    (256, 1024, 1, 1, 32, True, True), (1024, 256, 1, 1, 32, True, False), (512, 1024, 1, 2, 64, False, False),
    (512, 2048, 1, 1, 16, True, True), (2048, 512, 1, 1, 16, True, False), (1024, 2048, 1, 2, 32, False, False),
    (96, 64, 1, 1, 32, True, False), (64, 64, 1, 2, 64, True, False),          # 32-channel stages; a small strided 1x1
    # the BEV head's 2-D layers (bev/model.py:154-175): the merged 32 -> 256 first conv of det_head | param_head and the 16-channel
    # bv_pre layers (its two-group conv2 and the channel-slice 128 -> 4 output conv are in tests/test_gpu_bev_kernels.py)
    (32, 256, 3, 1, 128, True, False), (32, 16, 1, 1, 128, True, False), (16, 16, 3, 1, 128, True, False), (16, 16, 1, 1, 128, True, False),
]


# (an H2 tensor needs whole 16-channel chunks: the 40-channel head input of round 1 exists as a float32 layer only)
CONV_PARAMS = [(c, f) for f in ('f32', 'h2') for c in CONV_CASES if not (f == 'h2' and c[0] % 16)]


def _lower_conv_layer(dev, case, H, W, w, scale, shift, fmt):
    """One fused conv+BN(+res)(+ReLU) layer of CONV_CASES' form on an H x W map, lowered with every weight pack (the bf16x3 and
    f16x2 variants join a sweep over romp_conv_describe); fmt='h2': input / residual / output tensors in the pre-split H2 format.
    -> (program, op, output is H2)."""
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math, ACT_SHIFT
    cin, cout, k, s = case[:4]
    relu, use_res = case[5:7]
    relu_from = case[7] if len(case) > 7 else 0
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    P = Program(dev)
    set_conv_math(P, 'all')              # pack the split weights too: bf16x3 and f16x2 variants join the sweep below
    xa = Act(0, cin, H, W, cin)
    P.buf_floats.append(cin * H * W)
    ra = None
    if use_res:
        P.buf_floats.append(cout * Ho * Wo)
        ra = Act(1, cout, Ho, Wo, cout)
    P.conv('t', xa, [w], [scale], [shift], k, s, relu, res=ra, relu_from=relu_from)
    op = P.ops[0]
    assert op.relu_from == relu_from
    out_h2 = False
    if fmt == 'h2':
        assert cin % 8 == 0 and op.weight_h2, 'layer cannot read an H2 tensor (Cin %d)' % cin
        out_h2 = op.Cout == op.cout_pad and cout % 8 == 0
        op.act_shift = ACT_SHIFT
        op.in_fmt = L.FMT_H2
        op.out_fmt = L.FMT_H2 if out_h2 else L.FMT_F32
        op.res_fmt = L.FMT_H2 if (out_h2 and use_res) else L.FMT_F32
    return P, op, out_h2


def _conv_variants(lib, op, B):
    """The indices of the kernel variants romp_conv_describe accepts for the layer."""
    import ctypes as C
    buf = C.create_string_buffer(128)
    return [v for v in range(lib.romp_conv_num_variants()) if lib.romp_conv_describe(C.byref(op), B, v, buf, 128) == 0]


@pytest.mark.parametrize('case,fmt', CONV_PARAMS, ids=lambda v: v if isinstance(v, str) else 'c%d_%d_k%d_s%d_h%d' % v[:5])
@pytest.mark.parametrize('B', [1, 3])
def test_conv_layer(dev, case, B, fmt):
    """One fused conv+BN(+res)(+ReLU) layer through romp_conv_forward vs torch CPU conv2d: the naive cross-check kernel, the
    heuristic variant, then EVERY kernel variant able to run the layer.  fmt='h2': input / residual / output tensors in the
    pre-split H2 format (only the f16x2 kernels read it; every kernel family's epilogue can write it)."""
    import ctypes as C
    from romp_amd import lib as L
    from romp_amd.plan import encode_h2, decode_h2
    cin, cout, k, s, H, relu, use_res = case[:7]
    relu_from = case[7] if len(case) > 7 else 0
    g = torch.Generator().manual_seed(cin * 1000 + cout + k + s + H)
    x = torch.randn(B, H, H, cin, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    Ho = (H + 2 * (k // 2) - k) // s + 1
    res = torch.randn(B, Ho, Ho, cout, generator=g) if use_res else None
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, None, stride=s, padding=k // 2)
    ref = ref * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if res is not None:
        ref = ref + res.permute(0, 3, 1, 2)
    if relu:
        ref = torch.cat([ref[:, :relu_from], torch.relu(ref[:, relu_from:])], 1)
    ref = ref.permute(0, 2, 3, 1)
    P, op, out_h2 = _lower_conv_layer(dev, case, H, H, w, scale, shift, fmt)
    if fmt == 'h2':
        x_in = encode_h2(x)
        res_in = encode_h2(res) if (res is not None and op.res_fmt == L.FMT_H2) else res
    else:
        x_in, res_in = x, res
    xd, rd = x_in.to(dev), (res_in.to(dev) if res_in is not None else None)
    lib = L.load()
    buf = C.create_string_buffer(128)
    runs = ([(1, -1)] if fmt == 'f32' else []) + [(0, -1)] + [(0, v) for v in _conv_variants(lib, op, B)]
    assert len(runs) >= 2
    for mode, variant in runs:
        out = torch.full((B, Ho, Ho, cout), float('nan'), device=dev)
        L.check(lib.romp_conv_forward(C.byref(op), L.ptr(xd), L.ptr(rd), L.ptr(out), B, mode, variant, L.stream_ptr(dev)))
        torch.cuda.synchronize()
        o = out.cpu()
        if out_h2:
            o = decode_h2(o)
        err = (o - ref).abs().max().item()
        name = 'naive'
        if mode == 0:
            L.check(lib.romp_conv_describe(C.byref(op), B, variant, buf, 128))
            name = buf.value.decode()
        print(f'{name} (variant {variant}, {fmt}): max-abs err {err:.3e} (ref absmax {ref.abs().max():.2f})')
        assert err < 3e-5, f'{name} err {err}'


@pytest.mark.parametrize('mag', [1e4, 1e-6])
@pytest.mark.parametrize('case', [(32, 32, 3, 1, 64, True, True), (64, 128, 3, 2, 64, False, False), (64, 64, 1, 1, 64, True, False)],
                         ids=lambda c: 'c%d_%d_k%d_s%d' % c[:4])
def test_conv_layer_range_guard(dev, case, mag):
    """f16x2 range safety: a layer whose input is 1e4x / 1e-6x the usual magnitude.  With the measured range
    handed to plan.assign_formats the layer leaves the f16x2 kernels (float32 tensors, f32 / bf16x3 kernels) and EVERY variant
    still on offer meets the usual 3e-5 bound relative to the output's magnitude; without it the f16x2 kernels saturate at
    65504 / 2^shift -- finite garbage for the large input, never inf / NaN."""
    import ctypes as C
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math, h2_range_ok
    cin, cout, k, s, H, relu, use_res = case
    g = torch.Generator().manual_seed(7 + cin + cout + k)
    x = torch.randn(2, H, H, cin, generator=g) * mag
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1 * mag
    Ho = (H + 2 * (k // 2) - k) // s + 1
    res = torch.randn(2, Ho, Ho, cout, generator=g) * mag if use_res else None
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), None, stride=s, padding=k // 2)
    ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if res is not None:
        ref = ref + res.permute(0, 3, 1, 2).double()
    if relu:
        ref = torch.relu(ref)
    ref = ref.permute(0, 2, 3, 1).float()
    assert not h2_range_ok(float(x.abs().max()))
    lib = L.load()
    buf = C.create_string_buffer(128)

    def lower(guard):
        P = Program(dev)
        set_conv_math(P, 'all')
        P.buf_floats.append(cin * H * H)
        ra = None
        if res is not None:
            P.buf_floats.append(cout * Ho * Ho)
            ra = Act(1, cout, Ho, Ho, cout)
        P.conv('t', Act(0, cin, H, H, cin), [w], [scale], [shift], k, s, relu, res=ra)
        if guard:
            P.op_maxabs = [None] * len(P.ops)
            P.buf_maxabs = {0: float(x.abs().max())}
        P.op_array()                                     # assign_formats
        P.ops[0].out_fmt = L.FMT_F32                     # (nothing consumes the output here: read it back as plain floats)
        return P, P.ops[0]

    xd, rd = x.to(dev), (res.to(dev) if res is not None else None)
    P, op = lower(True)
    assert not op.weight_h2 and len(P.range_fallback) == 1, 'the guard must take the f16x2 weights away'
    runs = [-1] + [v for v in range(lib.romp_conv_num_variants()) if lib.romp_conv_describe(C.byref(op), 2, v, buf, 128) == 0]
    assert len(runs) >= 2
    for v in runs:
        out = torch.full((2, Ho, Ho, cout), float('nan'), device=dev)
        L.check(lib.romp_conv_forward(C.byref(op), L.ptr(xd), L.ptr(rd), L.ptr(out), 2, 0, v, L.stream_ptr(dev)))
        L.check(lib.romp_conv_describe(C.byref(op), 2, v, buf, 128))
        assert b'h2' not in buf.value, buf.value
        err = (out.cpu() - ref).abs().max().item() / ref.abs().max().item()
        print(f'{buf.value.decode()} (variant {v}) x{mag:g}: relative err {err:.3e}')
        assert err < 3e-5, (buf.value, err)
    # without the guard: the f16x2 kernels stay on offer and must at least stay finite
    P2, op2 = lower(False)
    assert op2.weight_h2
    for v in range(lib.romp_conv_num_variants()):
        if lib.romp_conv_describe(C.byref(op2), 2, v, buf, 128) != 0 or b'h2' not in buf.value:
            continue
        out = torch.full((2, Ho, Ho, cout), float('nan'), device=dev)
        L.check(lib.romp_conv_forward(C.byref(op2), L.ptr(xd), L.ptr(rd), L.ptr(out), 2, 0, v, L.stream_ptr(dev)))
        assert bool(torch.isfinite(out).all()), '%s produced inf / NaN' % buf.value.decode()


def test_net_range_calibration(dev):
    """Whole net with activations far outside the fp16 pieces' range (the stem's BatchNorm scaled so that everything downstream
    is ~3e3 x larger): RompNet's calibration moves the affected tensors / layers to the float32 path (range_fallback), the maps
    stay finite and agree with the exact-f32 net to 1e-4 of their magnitude; without calibration the f16x2 net saturates but
    stays finite (the kernels clamp), and ROMP_CHECK_FINITE-style checking passes.  With the ordinary weights nothing falls back."""
    from romp_amd.net import RompNet
    sd = O.make_romp_state_dict(0)
    img = O.make_images(2, seed=3).to(dev)
    net_ok = RompNet(sd, dev, max_batch=2, bf16x3='f16x2')
    assert net_ok.op_maxabs is not None and net_ok.range_fallback == [], net_ok.range_fallback
    big = {k: v.clone() for k, v in sd.items()}
    key_w = [k for k in big if k.endswith('bn2.weight') and k.count('.') <= 2][0]
    big[key_w] *= 3e3
    big[key_w.replace('weight', 'bias')] *= 3e3
    ref = RompNet(big, dev, max_batch=2, bf16x3='f32')
    cm_r, pm_r = ref(img)
    mag = max(cm_r.abs().max().item(), pm_r.abs().max().item())
    assert mag > 50.0, 'the scaled stem must blow the activations up (%g)' % mag
    net = RompNet(big, dev, max_batch=2, bf16x3='f16x2')
    assert len(net.range_fallback) > 10, 'calibration must flag the blown-up layers'
    cm, pm = net(img)
    assert bool(torch.isfinite(cm).all()) and bool(torch.isfinite(pm).all())
    e = max((cm - cm_r).abs().max().item(), (pm - pm_r).abs().max().item()) / mag
    print(f'{len(net.range_fallback)} layers on the float32 path, maps relative err {e:.3e} (magnitude {mag:.3g})')
    assert e < 1e-4
    raw = RompNet(big, dev, max_batch=2, bf16x3='f16x2', calibrate=False)
    cm2, pm2 = raw(img)
    assert bool(torch.isfinite(cm2).all()) and bool(torch.isfinite(pm2).all()), 'saturation, not inf / NaN'


@pytest.mark.parametrize('B,H,Cc,impl', [(1, 32, 32, 'r'), (3, 64, 32, 'r'), (2, 48, 32, 'r'), (1, 32, 32, 'v1'), (3, 64, 32, 'v1'), (2, 48, 32, 'v1'),
                                         (1, 16, 64, 'r'), (3, 64, 64, 'r'), (2, 48, 64, 'r'),
                                         # the production shapes (VERDICT r3 weak #1b): 128^2 x 32 (stage 2-4 branch 0) and 64^2 x 64 (branch 1)
                                         (2, 128, 32, 'r'), (2, 128, 32, 'v1'), (2, 64, 64, 'r')])
def test_fused_basic_block(dev, B, H, Cc, impl, monkeypatch):
    monkeypatch.setenv('ROMP_BBLOCK_RUN', '0')               # the plain tile order (the strip form: test_fused_basic_block_strip)
    _fused_basic_block(dev, B, H, Cc, impl, monkeypatch)


@pytest.mark.parametrize('B,H,Cc,run', [(3, 64, 64, 2), (3, 64, 64, 4), (2, 64, 64, 8), (1, 16, 64, 2), (2, 48, 64, 3), (2, 48, 64, 6),
                                        (3, 64, 32, 2), (3, 64, 32, 4), (3, 64, 32, 8), (2, 128, 32, 16), (2, 48, 32, 3), (1, 32, 32, 4),
                                        # the production launches: B = 32, the run length the launcher picks itself (4 of 8 tile rows / 8 of 16)
                                        (32, 64, 64, None), (32, 128, 32, None), (5, 64, 64, None), (24, 128, 32, None),
                                        # more runs than workgroups (256 / 512): 2.5 / 1.25 runs per workgroup, the run counter moves on inside the tile loop
                                        (40, 64, 64, 2), (20, 128, 32, 4)])
def test_fused_basic_block_strip(dev, B, H, Cc, run, monkeypatch):
    """conv_h2c.h's halo-carrying form (bblockr_kernel<C, 0, true>): a workgroup walks RUNS of vertically consecutive tiles, every tile
    but a run's first takes rows 8, 9 of the previous tile's intermediate over as its rows 0, 1 instead of recomputing them.  Every run
    length that divides the tile rows (2 .. the whole column), runs that start at / end on the image border, odd run counts per
    workgroup, and the launcher's own choice at the production batch."""
    if run is None:
        monkeypatch.delenv('ROMP_BBLOCK_RUN', raising=False)
    else:
        assert (H // 8) % run == 0
        monkeypatch.setenv('ROMP_BBLOCK_RUN', str(run))
    _fused_basic_block(dev, B, H, Cc, 'r', monkeypatch)


def _fused_basic_block(dev, B, H, Cc, impl, monkeypatch, W=None, run=True, ref_dtype=torch.float32):
    """csrc/conv_h2b.hip ('v1', 32 channels) / conv_h2c.h ('r', 32 and 64 channels): a BasicBlock as ONE launch (intermediate tile in LDS).  A three-conv program -- an
    ordinary conv producing the H2 block input, then the block -- lowered by plan.py (which must fuse the pair), run through
    romp_net_create / romp_net_forward, against torch on the CPU: image borders (the intermediate's zero padding), interior
    tiles, odd tile counts, batch > 1.  Same bound as the single layers, two layers deeper: 5e-5 of the output's magnitude.
    W: the map's width (default: square); run=False: lower and check the fusion only (no device; -> the program); ref_dtype: the reference's arithmetic."""
    import ctypes as C
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math, decode_h2
    monkeypatch.setenv('ROMP_FUSE_BLOCKS', 'all')
    W = H if W is None else W
    g = torch.Generator().manual_seed(100 * B + H + Cc)
    x = torch.randn(B, H, W, Cc, generator=g)
    ws = [torch.randn(Cc, Cc, 3, 3, generator=g) / (Cc * 9) ** 0.5 for _ in range(3)]
    sc = [torch.rand(Cc, generator=g) + 0.5 for _ in range(3)]
    sh = [torch.randn(Cc, generator=g) * 0.2 for _ in range(3)]

    def cbr(t, i, res=None):
        y = F.conv2d(t, ws[i].to(ref_dtype), None, padding=1) * sc[i].to(ref_dtype).view(1, -1, 1, 1) + sh[i].to(ref_dtype).view(1, -1, 1, 1)
        return torch.relu(y if res is None else y + res)
    t0 = cbr(x.permute(0, 3, 1, 2).to(ref_dtype), 0)
    ref = cbr(cbr(t0, 1), 2, res=t0).permute(0, 2, 3, 1).float()
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    a0 = P.conv('c0', Act(L.BUF_IMAGE, Cc, H, W, Cc), [ws[0]], [sc[0]], [sh[0]], 3, 1, True)
    a1 = P.conv('c1', a0, [ws[1]], [sc[1]], [sh[1]], 3, 1, True)
    a2 = P.conv('c2', a1, [ws[2]], [sc[2]], [sh[2]], 3, 1, True, res=a0)
    ops = P.op_array()
    fused_kind = L.OP_BBLOCK32 if Cc == 32 else L.OP_BBLOCK64
    assert P.fused_blocks == 1 and [o.kind for o in P.ops] == [L.OP_CONV, L.OP_NOP, fused_kind], [o.kind for o in P.ops]
    assert P.ops[2].out_fmt == L.FMT_H2
    if impl == 'v1':                                         # conv_h2b.hip's 16x16-tile kernel (single-image plans): no per-wave weight packs
        ops[1].flags &= ~L.OPF_WAVE16
        ops[2].flags &= ~L.OPF_WAVE16
    else:                                                    # conv_h2c.h's row-pipelined kernels
        assert ops[1].weight_aux and ops[2].weight_aux and (ops[1].flags & ops[2].flags & L.OPF_WAVE16)
    if not run:
        return P
    lib = L.load()
    h = C.c_void_p()
    sizes = (C.c_int64 * len(P.buf_floats))(*P.buf_floats)
    L.check(lib.romp_net_create(C.byref(h), ops, len(P.ops), sizes, len(P.buf_floats), B))
    try:
        xd = x.to(dev).contiguous()
        dummy = torch.empty(16, device=dev)
        n = P.buf_floats[a2.buf] * B
        out = torch.empty(n, device=dev)
        for rep in range(2):                                  # twice: the second run reuses warm buffers / queues
            L.check(lib.romp_net_forward(h, L.ptr(xd), B, L.ptr(dummy), L.ptr(dummy), L.stream_ptr(dev)))
            L.check(lib.romp_net_read_buffer(h, a2.buf, B, L.ptr(out), n, L.stream_ptr(dev)))
            torch.cuda.synchronize()
            y = decode_h2(out.cpu().reshape(B, H, W, Cc))
            err = (y - ref).abs().max().item() / ref.abs().max().item()
            print(f'fused BasicBlock B={B} {H}x{W}x{Cc} run {rep}: relative err {err:.3e}')
            assert err < 5e-5, err
    finally:
        lib.romp_net_destroy(h)


def _block_chain(dev, B, H, n_blocks, monkeypatch):
    """A conv producing an H2 tensor followed by `n_blocks` fused 32-channel BasicBlocks, each one's residual the tensor in front
    of it (as _fused_basic_block's program, any number of blocks) -> (program, op array, input, torch's result on the CPU, the
    last activation)."""
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math
    monkeypatch.setenv('ROMP_FUSE_BLOCKS', 'all')
    monkeypatch.setenv('ROMP_BBLOCK_RUN', '0')
    Cc, n = 32, 1 + 2 * n_blocks
    g = torch.Generator().manual_seed(100 * B + H + n)
    x = torch.randn(B, H, H, Cc, generator=g)
    ws = [torch.randn(Cc, Cc, 3, 3, generator=g) / (Cc * 9) ** 0.5 for _ in range(n)]
    sc = [torch.rand(Cc, generator=g) + 0.5 for _ in range(n)]
    sh = [torch.randn(Cc, generator=g) * 0.2 for _ in range(n)]

    def cbr(t, i, res=None):
        y = F.conv2d(t, ws[i], None, padding=1) * sc[i].view(1, -1, 1, 1) + sh[i].view(1, -1, 1, 1)
        return torch.relu(y if res is None else y + res)
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    t = cbr(x.permute(0, 3, 1, 2), 0)
    a = P.conv('c0', Act(L.BUF_IMAGE, Cc, H, H, Cc), [ws[0]], [sc[0]], [sh[0]], 3, 1, True)
    for b in range(n_blocks):
        i = 1 + 2 * b
        t = cbr(cbr(t, i), i + 1, res=t)
        m = P.conv('c%d' % i, a, [ws[i]], [sc[i]], [sh[i]], 3, 1, True)
        a = P.conv('c%d' % (i + 1), m, [ws[i + 1]], [sc[i + 1]], [sh[i + 1]], 3, 1, True, res=a)
    ops = P.op_array()
    assert P.fused_blocks == n_blocks and [o.kind for o in P.ops] == [L.OP_CONV] + [L.OP_NOP, L.OP_BBLOCK32] * n_blocks, [o.kind for o in P.ops]
    assert all(ops[i].weight_aux and ops[i].weight_h2 and (ops[i].flags & L.OPF_WAVE16) for i in range(1, n))
    return P, ops, x, t.permute(0, 2, 3, 1).contiguous(), a


def test_both_bblock32_kernels_in_one_program_graph_first(dev, monkeypatch):
    """One program with BOTH kernels behind ROMP_OP_BBLOCK32 -- block A on conv_h2c.h's row-pipelined one (ROMP_OPF_WAVE16), block B
    on conv_h2b.hip's v1 (the flag cleared, as test_fused_basic_block's 'v1' arm does) -- whose FIRST forward is a graph forward:
    every launch is captured, so neither kernel's one-time set-up may be left to its first launch.  The graph replay, an eager
    forward after it and torch on the CPU agree: bit-equal between the two, _fused_basic_block's 5e-5 of the output's magnitude
    against torch."""
    import ctypes as C
    from romp_amd import lib as L
    from romp_amd.plan import decode_h2
    B, H = 2, 32
    P, ops, x, ref, a = _block_chain(dev, B, H, 2, monkeypatch)
    ops[3].flags &= ~L.OPF_WAVE16
    ops[4].flags &= ~L.OPF_WAVE16
    lib = L.load()
    h = C.c_void_p()
    sizes = (C.c_int64 * len(P.buf_floats))(*P.buf_floats)
    L.check(lib.romp_net_create(C.byref(h), ops, len(P.ops), sizes, len(P.buf_floats), B))
    try:
        xd = x.to(dev).contiguous()
        dummy = torch.empty(16, device=dev)
        n = P.buf_floats[a.buf] * B
        got = []
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for graph in (1, 0):
                L.check(lib.romp_net_set_graph(h, graph))
                out = torch.empty(n, device=dev)
                L.check(lib.romp_net_forward(h, L.ptr(xd), B, L.ptr(dummy), L.ptr(dummy), L.stream_ptr(dev)))
                L.check(lib.romp_net_read_buffer(h, a.buf, B, L.ptr(out), n, L.stream_ptr(dev)))
                s.synchronize()
                got.append(decode_h2(out.cpu().reshape(B, H, H, 32)))
        err = (got[0] - ref).abs().max().item() / ref.abs().max().item()
        print(f'two fused BasicBlocks (row-pipelined, v1), graph first: relative err {err:.3e}')
        assert torch.equal(got[0], got[1])
        assert err < 5e-5, err
    finally:
        lib.romp_net_destroy(h)


def test_each_net_reports_clamps_to_its_own_counter(dev, monkeypatch):
    """Two nets driven alternately from one host thread: the launches of each report clamped values to THAT net's counter.  Net A's
    input is far outside the range its H2 tensors hold (65504 / 2^act_shift: c0's epilogue and the block clamp), net B's is not."""
    import ctypes as C
    from romp_amd import lib as L
    B, H = 1, 32
    P, ops, x, _, _ = _block_chain(dev, B, H, 1, monkeypatch)
    lib = L.load()
    sizes = (C.c_int64 * len(P.buf_floats))(*P.buf_floats)
    nets = [C.c_void_p(), C.c_void_p()]
    try:
        for h in nets:
            L.check(lib.romp_net_create(C.byref(h), ops, len(P.ops), sizes, len(P.buf_floats), B))
        dummy = torch.empty(16, device=dev)
        xs = [(x * 1e6).to(dev).contiguous(), x.to(dev).contiguous()]
        for rep in range(2):                                  # A, B, A, B
            for h, xd in zip(nets, xs):
                L.check(lib.romp_net_forward(h, L.ptr(xd), B, L.ptr(dummy), L.ptr(dummy), L.stream_ptr(dev)))
        counts = []
        for h in nets:
            c = C.c_int64(-1)
            L.check(lib.romp_net_saturated(h, C.byref(c), 0, L.stream_ptr(dev)))
            counts.append(c.value)
        print('saturation events: out-of-range net %d, in-range net %d' % tuple(counts))
        assert counts[0] > 0 and counts[1] == 0, counts
    finally:
        for h in nets:
            if h:
                lib.romp_net_destroy(h)


@pytest.mark.parametrize('CO,NUP,ND,H,B', [(32, 1, 1, 64, 1), (32, 2, 1, 64, 3), (32, 3, 1, 128, 2), (64, 1, 2, 32, 3), (64, 2, 2, 64, 2), (128, 1, 3, 32, 3)])
def test_fuseup(dev, CO, NUP, ND, H, B):
    _fuseup(dev, CO, NUP, ND, H, B)


def _fuseup(dev, CO, NUP, ND, H, B, W=None, run=True, ref_dtype=torch.float32):
    """csrc/conv_fup.hip (ROMP_OP_FUSEUP): a fuse-layer output with its 1x1 up-convs inside, lowered by plan.fuse_up_sums from the
    ordinary [1x1 convs ..., fusesum] form -- here with the up-convs MERGED over two outputs like plan.hr_module emits them (the
    output under test takes channel slice [16 : 16 + CO) of each) -- against torch: y = relu(sum of ND direct tensors +
    sum_k up_{2^k}(bn_k(W_k x_k))), x_k with CO << k channels at 1 / 2^k of the resolution.  HRNet's production shapes and small ones,
    B > 1, every instantiation of the kernel.  W: the map's width (default: square); run=False: lower and check the fusion only (no device; -> the program);
    ref_dtype: the reference's arithmetic."""
    import ctypes as C
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math, decode_h2
    g = torch.Generator().manual_seed(CO + 10 * NUP + H)
    W = H if W is None else W
    cin0 = 32
    img = torch.randn(B, H, W, cin0, generator=g)

    def mk(co, ci, k):
        return (torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5, torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g) * 0.2)

    def tconv(t, wsb, stride, relu):
        w, sc, sh = wsb
        y = F.conv2d(t, w.to(ref_dtype), None, stride=stride, padding=w.shape[-1] // 2) * sc.to(ref_dtype).view(1, -1, 1, 1) + sh.to(ref_dtype).view(1, -1, 1, 1)
        return torch.relu(y) if relu else y
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    x_img = Act(L.BUF_IMAGE, cin0, H, W, cin0)
    xin = img.permute(0, 3, 1, 2).to(ref_dtype)
    # sources: x_0 (CO @ H, a direct term), x_k (CO << k @ H >> k): a chain of stride-2 convs; extra direct terms from x_0
    srcs_w = [mk(CO, cin0, 3)] + [mk(CO << k, CO << (k - 1), 3) for k in range(1, NUP + 1)]
    acts, refs = [], []
    a, r = P.conv('x0', x_img, [srcs_w[0][0]], [srcs_w[0][1]], [srcs_w[0][2]], 3, 1, True), tconv(xin, srcs_w[0], 1, True)
    acts.append(a); refs.append(r)
    for k in range(1, NUP + 1):
        a = P.conv('x%d' % k, acts[-1], [srcs_w[k][0]], [srcs_w[k][1]], [srcs_w[k][2]], 3, 2, True)
        r = tconv(refs[-1], srcs_w[k], 2, True)
        acts.append(a); refs.append(r)
    directs, dref = [acts[0]], [refs[0]]
    for d in range(1, ND):
        wsb = mk(CO, CO, 1)
        directs.append(P.conv('d%d' % d, acts[0], [wsb[0]], [wsb[1]], [wsb[2]], 1, 1, False))
        dref.append(tconv(refs[0], wsb, 1, False))
    ups, uref = [], []
    for k in range(1, NUP + 1):                               # merged 1x1 conv: 16 other channels | CO channels of THIS output | 16 more
        wsb = mk(CO + 32, CO << k, 1)
        m = P.conv('up%d' % k, acts[k], [wsb[0]], [wsb[1]], [wsb[2]], 1, 1, False)
        ups.append(Act(m.buf, CO, m.H, m.W, m.cstride, 16))
        u = tconv(refs[k], wsb, 1, False)[:, 16:16 + CO]
        uref.append(u.repeat_interleave(1 << k, 2).repeat_interleave(1 << k, 3))
    out = P.fusesum('fuse', directs + ups, [0] * ND + list(range(1, NUP + 1)), True)
    sink = P.conv('sink', out, [mk(32, CO, 1)[0]], [torch.ones(32)], [torch.zeros(32)], 1, 1, False)    # an H2 consumer: keeps `out` in the H2 format
    ref = dref[0]
    for t in dref[1:] + uref:
        ref = ref + t
    ref = torch.relu(ref).permute(0, 2, 3, 1).float()
    ops = P.op_array()
    assert P.fused_ups == 1, 'plan.fuse_up_sums must fuse the output (kinds %s)' % [o.kind for o in P.ops]
    fup = [o for o in P.ops if o.kind == L.OP_FUSEUP][0]
    assert [o.kind for o in P.ops if o.kind == L.OP_FUSESUM] == [] and sum(o.kind == L.OP_NOP for o in P.ops) == NUP
    assert fup.out_fmt == L.FMT_H2 and fup.n_terms == ND + NUP
    if not run:
        return P
    lib = L.load()
    h = C.c_void_p()
    sizes = (C.c_int64 * len(P.buf_floats))(*P.buf_floats)
    L.check(lib.romp_net_create(C.byref(h), ops, len(P.ops), sizes, len(P.buf_floats), B))
    try:
        xd = img.to(dev).contiguous()
        dummy = torch.empty(16, device=dev)
        n = P.buf_floats[out.buf] * B
        got = torch.empty(n, device=dev)
        for rep in range(2):
            L.check(lib.romp_net_forward(h, L.ptr(xd), B, L.ptr(dummy), L.ptr(dummy), L.stream_ptr(dev)))
            L.check(lib.romp_net_read_buffer(h, out.buf, B, L.ptr(got), n, L.stream_ptr(dev)))
            torch.cuda.synchronize()
            y = decode_h2(got.cpu().reshape(B, H, W, CO))
            err = (y - ref).abs().max().item() / ref.abs().max().item()
            print(f'fuseup CO={CO} NUP={NUP} ND={ND} B={B} {H}x{W} run {rep}: relative err {err:.3e}')
            assert err < 5e-5, err
    finally:
        lib.romp_net_destroy(h)


def test_fusesum_formats(dev):
    """The fuse sum (model.py:233-244) with float32 and H2 terms / outputs gives the same values (the power-of-two scaling of
    the H2 format commutes with every rounding of the sum)."""
    from romp_amd.net import RompNet
    from romp_amd.plan import encode_h2, decode_h2
    from romp_amd import lib as L
    import ctypes as C
    lib = L.load()
    g = torch.Generator().manual_seed(5)
    B, Hh, Cc = 2, 32, 64
    t0 = torch.randn(B, Hh, Hh, Cc, generator=g)
    t1 = torch.randn(B, Hh // 2, Hh // 2, Cc, generator=g)
    t2 = torch.randn(B, Hh // 4, Hh // 4, Cc, generator=g)
    up = lambda t, f: t.repeat_interleave(f, 1).repeat_interleave(f, 2)
    ref = torch.relu(t0 + up(t1, 2) + up(t2, 4))
    # run through a two-op program: the fuse sum is reachable through the network executor only
    from romp_amd.plan import Program, Act
    from romp_amd.lib import RompOp, OP_FUSESUM, BUF_NONE
    # (last configuration: term 1 is a channel SLICE of a wider tensor -- a merged sibling conv's output, romp_op.term_coff)
    for fmts, ofmt, coff1 in (((0, 0, 0), 0, 0), ((1, 1, 1), 1, 0), ((1, 0, 1), 0, 0), ((0, 1, 0), 1, 0), ((1, 1, 1), 1, 32), ((0, 0, 1), 0, 64)):
        op = RompOp()
        op.kind, op.in_buf, op.res_buf, op.out_buf = OP_FUSESUM, BUF_NONE, BUF_NONE, 3
        op.H, op.W, op.Cin, op.Cout, op.relu, op.n_terms = Hh, Hh, Cc, Cc, 1, 3
        op.out_cstride, op.out_fmt, op.act_shift = Cc, ofmt, 4
        wide = Cc + 96 if coff1 else Cc                      # channel stride of term 1's buffer
        for k in range(3):
            op.term_buf[k], op.term_shift[k], op.term_cstride[k], op.term_fmt[k] = k, k, Cc, fmts[k]
        op.term_cstride[1], op.term_coff[1] = wide, coff1
        sizes = [Hh * Hh * Cc, Hh * Hh * wide // 4, Hh * Hh * Cc // 16, Hh * Hh * Cc]
        h = C.c_void_p()
        arr = (RompOp * 1)(op)
        L.check(lib.romp_net_create(C.byref(h), arr, 1, (C.c_int64 * 4)(*sizes), 4, B))
        try:
            for k, t in enumerate((t0, t1, t2)):
                if k == 1 and coff1:                         # embed the term in a wider tensor of other data
                    w_ = torch.randn(B, Hh // 2, Hh // 2, wide, generator=g) * 7.0
                    w_[..., coff1:coff1 + Cc] = t
                    t = w_
                td = (encode_h2(t) if fmts[k] else t).to(dev).contiguous()
                L.check(lib.romp_net_write_buffer(h, k, L.ptr(td), td.numel(), L.stream_ptr(dev)))
            dummy = torch.zeros(B * 16, device=dev)
            L.check(lib.romp_net_forward(h, L.ptr(dummy), B, L.ptr(dummy), L.ptr(dummy), L.stream_ptr(dev)))
            out = torch.empty(B * sizes[3], device=dev)
            L.check(lib.romp_net_read_buffer(h, 3, B, L.ptr(out), out.numel(), L.stream_ptr(dev)))
            torch.cuda.synchronize()
            o = out.cpu().reshape(B, Hh, Hh, Cc)
            if ofmt:
                o = decode_h2(o)
            err = (o - ref).abs().max().item()
            print('fusesum term fmts', fmts, 'out fmt', ofmt, 'max-abs err %.3e' % err)
            assert err < 2e-6
        finally:
            lib.romp_net_destroy(h)


# ------------------------------------------------------------------------------ network
@pytest.fixture(scope='module')
def net0(dev):
    from romp_amd.net import RompNet
    return RompNet(O.make_romp_state_dict(0), dev, max_batch=4)


def test_net_golden(dev, golden_dir, net0):
    g = _g(golden_dir, 'romp_net_b1.npz')
    img = O.make_images(1, seed=1).to(dev)
    for mode in (1, 0):
        net0.set_mode(mode)
        cm, pm = net0(img)
        assert cm.shape == (1, 1, 64, 64) and pm.shape == (1, 145, 64, 64)
        ec = np.abs(cm.cpu().numpy() - g['center_maps']).max()
        p = pm[0].reshape(145, -1).cpu().numpy()
        ep = np.abs(p[:, g['sample_pos']] - g['params_samples']).max()
        es = np.abs(p.astype(np.float64).sum(1) - g['params_chan_sum']).max()
        print(f'mode {mode}: center max-abs {ec:.3e} params max-abs {ep:.3e} chan-sum {es:.3e}')
        assert ec < 1e-4 and ep < 1e-4 and es < 5e-2
    net0.set_mode(0)


def test_net_vs_oracle_batch(dev, net0):
    sd = O.make_romp_state_dict(0)
    img = O.make_images(3, seed=5)
    cm_o, pm_o = O.romp_net_forward(sd, img)
    cm, pm = net0(img.to(dev))
    ec = (cm.cpu() - cm_o).abs().max().item()
    ep = (pm.cpu() - pm_o).abs().max().item()
    print(f'B=3 center {ec:.3e} params {ep:.3e}')
    assert ec < 1e-4 and ep < 1e-4
    # batch position independence: image 2 alone == image 2 in the batch
    cm1, pm1 = net0(img[2:3].to(dev))
    assert (cm1 - cm[2:3]).abs().max().item() < 2e-5 and (pm1 - pm[2:3]).abs().max().item() < 2e-5
    # branch-parallel side streams vs one stream: same kernels, same arithmetic -> identical maps
    net0.set_streams(False)
    cm_s, pm_s = net0(img.to(dev))
    net0.set_streams(True)
    assert torch.equal(cm_s, cm) and torch.equal(pm_s, pm)
    # autotuned kernel variants keep parity
    net0.autotune(3, iters=1)
    cm_t, pm_t = net0(img.to(dev))
    assert (cm_t.cpu() - cm_o).abs().max().item() < 1e-4 and (pm_t.cpu() - pm_o).abs().max().item() < 1e-4
    cm, pm = cm_t, pm_t
    # hipGraph replay gives the same maps as eager launches
    net0.set_graph(True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = img.to(dev)
        c1, p1 = net0.forward_nhwc(x)
        c2, p2 = net0.forward_nhwc(x, c1.clone(), p1.clone())
    s.synchronize()
    net0.set_graph(False)
    assert torch.equal(c1.unsqueeze(1), cm) and torch.equal(c2, c1)


@pytest.mark.parametrize('conv_math', [BX3, 'f16x2'])
def test_net_bf16x3_parity(dev, golden_dir, conv_math):
    """conv_math='bf16x3' / 'f16x2': every conv the autotuner moves onto the 16-bit matrix pipe (3 bf16 pieces and six
    piece products, or 2 fp16 pieces and three, f32 accumulation) must pass the SAME gates as the f32-MFMA network:
    1e-4 max-abs against the reference fixture and against the oracle."""
    from romp_amd.net import RompNet
    sd = O.make_romp_state_dict(0)
    net = RompNet(sd, dev, max_batch=4, bf16x3=conv_math)
    net.autotune(3, iters=1)
    names = net.variant_names(3)
    tag = 'conv_bx' if conv_math == 'bf16x3' else 'conv_h2'
    n_bx3 = sum(tag in n for n in names)
    print('convs on the %s kernels at B=3: %d of %d ops' % (conv_math, n_bx3, len(names)))
    assert n_bx3 > 0
    img = O.make_images(3, seed=5)
    cm_o, pm_o = O.romp_net_forward(sd, img)
    cm, pm = net(img.to(dev))
    ec, ep = (cm.cpu() - cm_o).abs().max().item(), (pm.cpu() - pm_o).abs().max().item()
    print(f'{conv_math} B=3 vs oracle: center {ec:.3e} params {ep:.3e}')
    assert ec < 1e-4 and ep < 1e-4
    g = _g(golden_dir, 'romp_net_b1.npz')
    net.autotune(1, iters=1)
    cm, pm = net(O.make_images(1, seed=1).to(dev))
    p = pm[0].reshape(145, -1).cpu().numpy()
    ec = np.abs(cm.cpu().numpy() - g['center_maps']).max()
    ep = np.abs(p[:, g['sample_pos']] - g['params_samples']).max()
    print(f'{conv_math} B=1 vs reference fixture: center {ec:.3e} params {ep:.3e}')
    assert ec < 1e-4 and ep < 1e-4


def test_translation_lsq_vs_reference_fixture(dev, golden_dir):
    """romp_estimate_translation (the cam_trans of body_mesh_projection2image when OpenCV is absent) against the
    reference's estimate_translation recorded with cv2 absent (oracle/make_golden_translation.py)."""
    from romp_amd import lib as L
    g = _g(golden_dir, 'translation_lsq.npz')
    lib = L.load()
    j, pj = torch.from_numpy(g['joints']).to(dev).contiguous(), torch.from_numpy(g['pj2d']).to(dev).contiguous()
    N = j.shape[0]
    out = torch.empty(N, 3, device=dev)
    L.check(lib.romp_estimate_translation(L.ptr(j), N, 71, 24, L.ptr(pj), 443.4, 512., L.ptr(out), L.stream_ptr(dev)))
    err = np.abs(out.cpu().numpy() - g['trans']).max()
    print('device least-squares translation vs reference: max-abs %.3e' % err)
    np.testing.assert_allclose(out.cpu().numpy(), g['trans'], rtol=2e-5, atol=2e-6)
    # through the post-processing entry point
    from romp_amd.post_parser import body_mesh_projection2image, _HAVE_CV2
    if not _HAVE_CV2:
        r = body_mesh_projection2image(j, torch.from_numpy(g['cam']).to(dev))
        np.testing.assert_allclose(r['cam_trans'].cpu().numpy(), g['trans'], rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(r['pj2d'].cpu().numpy(), g['pj2d'], atol=1e-6)


@pytest.mark.parametrize('conv_math', ['f32', 'f16x2'])
def test_net_split_k_single_image(dev, golden_dir, conv_math):
    """Single-image nets (max_batch <= 2) lower the layers with few pixels and many input channels as split-K convs (grouped
    conv over input-channel slices -> float32 partials -> ksum with the layer's epilogue); with the f16x2 kernels on offer the deep
    layers stay ONE conv instead and csrc/conv_h2k.hip splits their input channels across the waves of a workgroup (round 4:
    171 -> 0 ksum launches; the tuned single-image table must actually pick conv_h2k for them).  Same gates as every other plan:
    1e-4 against the reference fixture (B=1) and the oracle (B=2)."""
    from romp_amd.net import RompNet
    from romp_amd.lib import OP_KSUM
    sd = O.make_romp_state_dict(0)
    net = RompNet(sd, dev, max_batch=2, bf16x3=conv_math)
    n_ksum = sum(o.kind == OP_KSUM for o in net.program.ops)
    assert net.split_k == 128 and (n_ksum > 150 if conv_math == 'f32' else n_ksum == 0), n_ksum
    if conv_math == 'f16x2':
        net.autotune(1, iters=1)
        assert sum('conv_h2k' in n for n in net.variant_names(1)) > 100, 'the deep 3x3 layers of a single image belong on conv_h2k'
        net.autotune(2, iters=1)
    g = _g(golden_dir, 'romp_net_b1.npz')
    cm, pm = net(O.make_images(1, seed=1).to(dev))
    p = pm[0].reshape(145, -1).cpu().numpy()
    ec = np.abs(cm.cpu().numpy() - g['center_maps']).max()
    ep = np.abs(p[:, g['sample_pos']] - g['params_samples']).max()
    print(f'split-K {conv_math} ({n_ksum} split layers) B=1 vs reference fixture: center {ec:.3e} params {ep:.3e}')
    assert ec < 1e-4 and ep < 1e-4
    img = O.make_images(2, seed=5)
    cm_o, pm_o = O.romp_net_forward(sd, img)
    cm, pm = net(img.to(dev))
    ec, ep = (cm.cpu() - cm_o).abs().max().item(), (pm.cpu() - pm_o).abs().max().item()
    print(f'split-K {conv_math} B=2 vs oracle: center {ec:.3e} params {ep:.3e}')
    assert ec < 1e-4 and ep < 1e-4
    # the default plan of a larger net has none
    assert RompNet(sd, dev, max_batch=4).split_k == 0


def test_plan_file_c_abi_only(dev, tmp_path):
    """export.save_plan -> romp_net_load: a net created by the C ABI from the file alone (no state_dict, no lowering) gives
    BIT-IDENTICAL maps to the net the file was exported from, for the batch plan (autotuned table travels) and for the
    single-image split-K plan; and through RompNet.from_plan."""
    import ctypes as C
    from romp_amd import lib as L
    from romp_amd.export import save_plan
    from romp_amd.net import RompNet
    lib = L.load()
    sd = O.make_romp_state_dict(0)
    for max_batch, B in ((4, 3), (1, 1)):
        net = RompNet(sd, dev, max_batch=max_batch, bf16x3='f16x2')
        img = O.make_images(B, seed=5).to(dev)
        c0, p0 = net.forward_nhwc(img)                       # (autotunes B: the table goes into the file)
        path = str(tmp_path / ('romp_b%d.plan' % max_batch))
        save_plan(net, path)
        h = C.c_void_p()
        L.check(lib.romp_net_load(C.byref(h), path.encode(), max_batch))
        try:
            size, cf, pf, n_ops = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32()
            L.check(lib.romp_net_plan_info(h, C.byref(size), C.byref(cf), C.byref(pf), C.byref(n_ops)))
            assert (size.value, cf.value, pf.value, n_ops.value) == (512, 64 * 64, 64 * 64 * 145, len(net.program.ops))
            kind = C.c_int32(-1)
            L.check(lib.romp_net_plan_kind(h, C.byref(kind)))                # the plan KIND travels in the header (single-image: 128 items)
            assert kind.value == net.split_k == (128 if max_batch == 1 else 0)
            assert [lib.romp_net_tuned_variant(h, B, i) for i in range(n_ops.value)] == net.tuned_variants(B)
            c1, p1 = torch.empty_like(c0), torch.empty_like(p0)
            L.check(lib.romp_net_forward(h, L.ptr(img), B, L.ptr(c1), L.ptr(p1), L.stream_ptr(dev)))
            torch.cuda.synchronize()
            assert torch.equal(c1, c0) and torch.equal(p1, p0)
        finally:
            lib.romp_net_destroy(h)
        net2 = RompNet.from_plan(path, dev, max_batch=max_batch)
        c2, p2 = net2.forward_nhwc(img)
        assert torch.equal(c2, c0) and torch.equal(p2, p0) and net2.split_k == net.split_k == (128 if max_batch == 1 else 0)
    # the drop-in API from the plan file (the reference's --onnx branch, main.py:86-89): same result dict as from the state_dict
    import romp_amd
    rs = np.random.RandomState(0)
    frame = rs.randint(0, 256, (360, 640, 3)).astype(np.uint8)
    sd2 = O.make_romp_state_dict(0, center_bias=2.0)
    path2 = str(tmp_path / 'romp_api.plan')
    outs = []
    for kw in (dict(state_dict=sd2), dict()):
        s_ = romp_amd.romp_settings([] if kw else ['--plan_path', path2])
        s_.GPU, s_.center_thresh, s_.max_batch = 0, 1.25, 1
        m_ = romp_amd.ROMP(s_, smpl_model=O.make_synthetic_smpl(0), **kw)
        outs.append(m_(frame))
        if kw:
            save_plan(m_.model, path2)                       # with the kernel table its first forward measured
    assert outs[0] is not None and set(outs[0]) == set(outs[1])
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    # a truncated file is refused with a message, not a crash
    bad = str(tmp_path / 'bad.plan')
    open(bad, 'wb').write(open(path, 'rb').read()[:-100])
    h = C.c_void_p()
    assert lib.romp_net_load(C.byref(h), bad.encode(), 1) != 0 and b'size' in lib.romp_last_error()


def test_c_host_without_python(dev, tmp_path):
    """examples/host_no_python.cpp: a compiled host that knows only include/romp_hip.h and a plan file (romp_net_load ->
    romp_net_forward (graph replay) -> romp_parse) must write the same bytes as the Python path."""
    import subprocess
    from romp_amd.export import save_plan
    from romp_amd.net import RompNet
    from romp_amd.post_parser import CenterMap, parsing_outputs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'host_no_python')
    r = subprocess.run(['hipcc', '--offload-arch=gfx950', '-O2', '-I', os.path.join(root, 'include'), os.path.join(root, 'examples', 'host_no_python.cpp'),
                        '-L', os.path.join(root, 'romp_amd'), '-lromp_hip', '-Wl,-rpath,' + os.path.join(root, 'romp_amd'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    sd = O.make_romp_state_dict(0, center_bias=2.0)
    net = RompNet(sd, dev, max_batch=2, bf16x3='f16x2')
    img = O.make_images(2, seed=7)
    c0, p0 = net.forward_nhwc(img.to(dev))
    ref = parsing_outputs(c0.unsqueeze(1), p0, CenterMap(1.25))
    plan, frames, prefix = str(tmp_path / 'net.plan'), str(tmp_path / 'frames.f32'), str(tmp_path / 'out')
    save_plan(net, plan)
    img.numpy().astype(np.float32).tofile(frames)
    r = subprocess.run([exe, plan, frames, '2', '1.25', prefix], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.fromfile(prefix + '.center.f32', np.float32), c0.cpu().numpy().ravel())
    assert ref is not None
    assert np.array_equal(np.fromfile(prefix + '.thetas.f32', np.float32), ref['smpl_thetas'].cpu().numpy().ravel())
    assert np.array_equal(np.fromfile(prefix + '.cam.f32', np.float32), ref['cam'].cpu().numpy().ravel())
    assert len(np.fromfile(prefix + '.flat.i32', np.int32)) == ref['cam'].shape[0]


def test_romp_api_fast_path(dev):
    """ROMP(settings)(frame) takes the latency-arranged path by default (everything enqueued for all candidate rows, one
    synchronisation): its result dict must be the standard flow's, key for key and byte for byte, over several frames
    (stale candidate rows from earlier frames must not leak), including the nobody-detected case."""
    import romp_amd
    sd = O.make_romp_state_dict(0, center_bias=2.0)
    smpl = O.make_synthetic_smpl(0)
    s = romp_amd.romp_settings([])
    s.GPU, s.center_thresh, s.max_batch = 0, 1.25, 1
    model = romp_amd.ROMP(s, state_dict=sd, smpl_model=smpl)
    rs = np.random.RandomState(5)
    for shape in ((360, 640, 3), (720, 1280, 3), (512, 512, 3), (300, 200, 3)):
        frame = rs.randint(0, 256, shape).astype(np.uint8)
        model.fast_single = True
        a = model(frame)
        model.fast_single = False
        b = model(frame)
        assert a is not None and b is not None and set(a) == set(b), (set(a), set(b))
        for k in b:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        print('frame', shape, ':', a['cam'].shape[0], 'persons, fast path == standard path')
    model.centermap_parser.conf_thresh = 1e3
    model.fast_single = True
    assert model(frame) is None


def test_net_batch_lanes(dev):
    """set_split(2): the forward runs as two half-batch lanes on two streams (convs capped at one
    workgroup per CU).  Same maps as the oracle for every image of the batch, eagerly and from a hipGraph;
    odd batches fall back to one lane."""
    from romp_amd.net import RompNet
    sd = O.make_romp_state_dict(0)
    net = RompNet(sd, dev, max_batch=4)
    img = O.make_images(4, seed=6)
    cm_o, pm_o = O.romp_net_forward(sd, img)
    x = img.to(dev)
    cm1, pm1 = net(x)
    net.set_split(2, 1)
    cm2, pm2 = net(x)
    for name, (c, p) in {'one lane': (cm1, pm1), 'two lanes': (cm2, pm2)}.items():
        ec, ep = (c.cpu() - cm_o).abs().max().item(), (p.cpu() - pm_o).abs().max().item()
        print(f'{name}: center {ec:.3e} params {ep:.3e}')
        assert ec < 1e-4 and ep < 1e-4
    assert (cm2 - cm1).abs().max().item() < 2e-5 and (pm2 - pm1).abs().max().item() < 2e-5
    c3, p3 = net(x[:3])                                    # odd batch: single lane
    assert (c3 - cm2[:3]).abs().max().item() < 2e-5 and (p3 - pm2[:3]).abs().max().item() < 2e-5
    net.set_graph(True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xs = img.to(dev)
        c4, p4 = net.forward_nhwc(xs)
        c5, p5 = net.forward_nhwc(xs, c4.clone(), p4.clone())
    s.synchronize()
    assert torch.equal(c4.unsqueeze(1), cm2) and torch.equal(c5, c4) and torch.equal(p5, p4)


def test_net_full_batch_properties(dev):
    """BASELINE config 2 size (B=32): images repeated inside the batch must give identical maps
    (no cross-image leakage, tile/batch indexing correct at full size), and a permuted batch must
    give permuted outputs."""
    from romp_amd.net import RompNet
    net = RompNet(O.make_romp_state_dict(0), dev, max_batch=32)
    base = O.make_images(4, seed=2).to(dev)
    idx = torch.arange(32) % 4
    cm, pm = net.forward_nhwc(base[idx])
    for r in range(4, 32):
        assert torch.equal(cm[r], cm[r % 4]) and torch.equal(pm[r], pm[r % 4])
    perm = torch.randperm(32, generator=torch.Generator().manual_seed(0))
    cm2, pm2 = net.forward_nhwc(base[idx][perm])
    assert torch.equal(cm2, cm[perm]) and torch.equal(pm2, pm[perm])
    assert torch.isfinite(pm).all()


@pytest.mark.parametrize('B,conv_math', [(32, 'f16x2'), pytest.param(32, 'bf16x3', marks=BX3.marks), (128, 'f16x2')])
def test_net_benchmark_batch_vs_oracle(dev, B, conv_math):
    """The sizes bench.py times (BASELINE configs[1]: B=32; the per-GPU shard of configs[2]: B=128), with the kernel
    variants the autotuner picks AT THAT SIZE: images {0, 7, 19, B-1} of the batch against the oracle network (1e-4), and the
    whole net -> parse -> SMPL result of those images against the oracle pipeline (detections exact, verts 1e-4 on
    identical theta / beta, verts 1e-3 end to end)."""
    import romp_amd
    settings = romp_amd.romp_settings([])
    settings.GPU, settings.center_thresh, settings.max_batch, settings.conv_math = 0, 1.3, B, conv_math
    sd = O.make_romp_state_dict(0, center_bias=2.0)         # bench.py's weights (romp_amd.synthetic default): ~12 persons / image
    smpl_model = O.make_synthetic_smpl(0)
    model = romp_amd.ROMP(settings, state_dict=sd, smpl_model=smpl_model)
    model.model.autotune(B, iters=1)
    names = model.model.variant_names(B)
    tag = 'conv_bx' if conv_math == 'bf16x3' else 'conv_h2'
    assert sum(tag in n for n in names) > 0
    img = O.make_images(B, seed=1)
    x = img.to(dev)
    cm, pm = model.model(x)
    pick = [0, 7, 19, B - 1]
    cm_o, pm_o = O.romp_net_forward(sd, img[pick])
    ec = (cm[pick].cpu() - cm_o).abs().max().item()
    ep = (pm[pick].cpu() - pm_o).abs().max().item()
    print(f'B={B} {conv_math}: images {pick} vs oracle: center {ec:.3e} params {ep:.3e}')
    assert ec < 1e-4 and ep < 1e-4
    out, bids = model.forward_batch(x)
    ref = O.parsing_outputs(cm_o.numpy(), pm_o.numpy(), settings.center_thresh)
    assert out is not None and ref is not None
    bids = bids.cpu().numpy()
    rows = np.concatenate([np.nonzero(bids == b)[0] for b in pick])
    assert np.array_equal(np.searchsorted(pick, bids[rows]), ref['batch_ids'])
    assert np.array_equal(out['center_preds'].cpu().numpy()[rows], ref['center_preds'])
    th, be = out['smpl_thetas'].cpu().numpy()[rows], out['smpl_betas'].cpu().numpy()[rows]
    vo, jo, _ = O.smpl_forward(smpl_model, be, th)                                       # identical theta / beta
    ev = np.abs(out['verts'].cpu().numpy()[rows] - vo).max()
    vr, _, _ = O.smpl_forward(smpl_model, ref['smpl_betas'], ref['smpl_thetas'])       # the oracle's own theta / beta
    ee = np.abs(out['verts'].cpu().numpy()[rows] - vr).max()
    print(f'B={B} {conv_math}: {len(rows)} persons in the 4 images; verts max-abs {ev:.3e} (same theta), {ee:.3e} (end to end)')
    assert ev < 1e-4 and ee < 1e-3


@pytest.mark.parametrize('kernel', ['mfma', 'valu'])
@pytest.mark.parametrize('B,H,W', [(1, 64, 64), (3, 96, 64)])
def test_stem_mfma_vs_torch(dev, kernel, B, H, W):
    """The stem in isolation (model.py:384-387: x / 255 * 2 - 1, conv 3x3 s2 3 -> 64, BN, ReLU) against F.conv2d with the
    normalisation: stem_mfma_kernel (K = 27 as one f16x2 MFMA step, H2 output -- the default path) and stem_conv_kernel (float32
    VALU; ROMP_OPF_STEM_VALU), image borders included (every tile of these sizes touches one), B in {1, 3}, a non-square frame.
    Also: a checkpoint whose stem weights do not fit the MFMA form's fp16 pieces is lowered onto the VALU kernel."""
    import ctypes as C
    from romp_amd import lib as L
    from romp_amd.plan import Program, assign_formats, set_conv_math, decode_h2, ACT_SHIFT
    g = torch.Generator().manual_seed(11 * B + H)
    img = torch.rand(B, H, W, 3, generator=g) * 255.0
    w = torch.randn(64, 3, 3, 3, generator=g) * 0.3
    scale, shift = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    ref = F.conv2d((img / 255.0 * 2.0 - 1.0).permute(0, 3, 1, 2), w, None, stride=2, padding=1)
    ref = torch.relu(ref * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    P.stem('stem', w, scale, shift, H, W)
    op = P.ops[0]
    assert not (op.flags & L.OPF_STEM_VALU), 'ordinary weights take the MFMA stem'
    op.out_fmt, op.act_shift = L.FMT_H2, ACT_SHIFT
    if kernel == 'valu':
        op.flags |= L.OPF_STEM_VALU
    lib = L.load()
    out = torch.full((B, H // 2, W // 2, 64), float('nan'), device=dev)
    L.check(lib.romp_conv_forward(C.byref(op), L.ptr(img.to(dev).contiguous()), None, L.ptr(out), B, 0, -1, L.stream_ptr(dev)))
    torch.cuda.synchronize()
    err = (decode_h2(out.cpu()) - ref).abs().max().item()
    print(f'stem {kernel} B={B} {H}x{W}: max-abs err {err:.3e} (ref absmax {ref.abs().max():.2f})')
    assert err < 3e-5, err
    big = Program(dev)
    set_conv_math(big, 'f16x2')
    big.stem('stem', w * 2000.0, scale, shift, H, W)
    assert big.ops[0].flags & L.OPF_STEM_VALU, '256 |w| beyond fp16: the plan must pick the float32 stem'


@pytest.mark.parametrize('B,H,W', [(1, 64, 64), (3, 128, 64), (2, 512, 512)])
def test_stem2_fused_vs_torch(dev, B, H, W, monkeypatch):
    """csrc/stem2.hip (round 6, ROMP_OP_STEM2): HRNet's stem and conv2 (model.py:384-390) as ONE kernel whose 64-channel
    half-resolution intermediate never leaves the CU, against torch on the CPU (x / 255 * 2 - 1, conv 3x3 s2 3 -> 64 + BN + ReLU,
    conv 3x3 s2 64 -> 64 + BN + ReLU; zero padding of BOTH convs at the image borders: every tile of the small sizes touches one)
    and against the ROMP_FUSE_STEM2=0 lowering of the same program (two launches: the tensors agree to float32 rounding of the
    intermediate's fp16 pieces, which the fused kernel forms the same way)."""
    import ctypes as C
    from romp_amd import lib as L
    from romp_amd.plan import Program, set_conv_math, decode_h2
    g = torch.Generator().manual_seed(13 * B + H)
    img = torch.rand(B, H, W, 3, generator=g) * 255.0
    w1 = torch.randn(64, 3, 3, 3, generator=g) * 0.3
    w2 = torch.randn(64, 64, 3, 3, generator=g) / (64 * 9) ** 0.5
    w3 = torch.randn(64, 64, 1, 1, generator=g) / 8.0
    sc = [torch.rand(64, generator=g) + 0.5 for _ in range(3)]
    sh = [torch.randn(64, generator=g) * 0.2 for _ in range(3)]
    m = F.conv2d((img / 255.0 * 2.0 - 1.0).permute(0, 3, 1, 2), w1, None, stride=2, padding=1)
    m = torch.relu(m * sc[0].view(1, -1, 1, 1) + sh[0].view(1, -1, 1, 1))
    y = F.conv2d(m, w2, None, stride=2, padding=1)
    ref = torch.relu(y * sc[1].view(1, -1, 1, 1) + sh[1].view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    lib = L.load()
    outs = {}
    for fuse in ('1', '0'):
        monkeypatch.setenv('ROMP_FUSE_STEM2', fuse)
        P = Program(dev)
        set_conv_math(P, 'f16x2')
        a = P.stem('stem.conv1', w1, sc[0], sh[0], H, W)
        b = P.conv('stem.conv2', a, [w2], [sc[1]], [sh[1]], 3, 2, True)
        P.conv('reader', b, [w3], [sc[2]], [sh[2]], 1, 1, True)          # (keeps conv2's output an H2 tensor with a consumer)
        ops = P.op_array()
        assert P.fused_stem2 == int(fuse) and [o.kind for o in P.ops[:2]] == ([L.OP_NOP, L.OP_STEM2] if fuse == '1' else [L.OP_STEM, L.OP_CONV])
        h = C.c_void_p()
        sizes = (C.c_int64 * len(P.buf_floats))(*P.buf_floats)
        L.check(lib.romp_net_create(C.byref(h), ops, len(P.ops), sizes, len(P.buf_floats), B))
        try:
            dummy = torch.empty(16, device=dev)
            xd = img.to(dev).contiguous()
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for graph in (0, 1):                                   # eagerly, and with the stem2 op as the eager prefix of a graph replay
                    L.check(lib.romp_net_set_graph(h, graph))
                    for rep in range(2):
                        L.check(lib.romp_net_forward(h, L.ptr(xd), B, L.ptr(dummy), L.ptr(dummy), L.stream_ptr(dev)))
                    n = P.buf_floats[b.buf] * B
                    out = torch.empty(n, device=dev)
                    L.check(lib.romp_net_read_buffer(h, b.buf, B, L.ptr(out), n, L.stream_ptr(dev)))
                    s.synchronize()
                    got = decode_h2(out.cpu().reshape(B, H // 4, W // 4, 64))
                    err = (got - ref).abs().max().item() / ref.abs().max().item()
                    print(f'stem2 fuse={fuse} graph={graph} B={B} {H}x{W}: relative err {err:.3e}')
                    assert err < 3e-5, (fuse, graph, err)
                    outs[(fuse, graph)] = got
        finally:
            lib.romp_net_destroy(h)
    assert torch.equal(outs[('1', 0)], outs[('1', 1)])
    d = (outs[('1', 0)] - outs[('0', 0)]).abs().max().item()
    assert d < 2e-5 * max(1.0, ref.abs().max().item()), d


@pytest.mark.parametrize('max_batch', [1, 2])
def test_net_conv_math_all_single_image(dev, max_batch, monkeypatch):
    """conv_math='all' in a single-image plan: every conv carries the bf16x3 pack in weight_aux, the
    32-channel blocks are fused WITHOUT the per-wave repack -- the fused launcher must dispatch on ROMP_OPF_WAVE16, not on
    weight_aux != NULL (it used to run the row-pipelined kernel on bf16x3 bytes: silently wrong maps).  (The bf16x3 KERNELS are an
    optional part of the library since round 6; the host-side pack is forced on here -- stale bytes in weight_aux are the point.)"""
    from romp_amd import lib as L
    from romp_amd.net import RompNet
    monkeypatch.setattr(L, 'has_bf16x3', lambda: True)
    sd = O.make_romp_state_dict(0)
    net = RompNet(sd, dev, max_batch=max_batch, bf16x3='all')
    blocks = [o for o in net.program.ops if o.kind == L.OP_BBLOCK32]
    assert len(blocks) == 32 and all(o.weight_aux and not (o.flags & L.OPF_WAVE16) for o in blocks), 'single-image plan: conv_h2b.hip kernel, stale bf16x3 pack in weight_aux'
    img = O.make_images(max_batch, seed=5)
    cm_o, pm_o = O.romp_net_forward(sd, img)
    cm, pm = net(img.to(dev))
    ec, ep = (cm.cpu() - cm_o).abs().max().item(), (pm.cpu() - pm_o).abs().max().item()
    print(f"conv_math='all' max_batch={max_batch}: center {ec:.3e} params {ep:.3e}")
    assert ec < 1e-4 and ep < 1e-4


@pytest.mark.parametrize('max_batch', [2, 8])
def test_net_stage_region_edges_vs_barriers(dev, monkeypatch, max_batch):
    """Round 4: the HRNet stages run as ONE open fork .. join region whose streams hand tensors over through ROMP_OP_RECORD /
    ROMP_OP_WAIT edges (plan.hr_module, `dataflow`).  Same kernels as the barrier form of rounds 1-3 (ROMP_DATAFLOW=0), so the
    outputs must be IDENTICAL -- eagerly and from a replayed graph, and from replay to replay (a missing edge shows up as a
    difference here long before it shows up as a wrong pose; plan.stream_races is the static half of this check)."""
    from romp_amd import lib as L
    from romp_amd.net import RompNet
    sd = O.make_romp_state_dict(0)
    img = O.make_images(max_batch, seed=9).to(dev)
    net = RompNet(sd, dev, max_batch=max_batch, bf16x3='f16x2')
    assert sum(o.kind == L.OP_WAIT for o in net.program.ops) > 40 and sum(o.kind == L.OP_JOIN for o in net.program.ops) <= 3
    monkeypatch.setenv('ROMP_DATAFLOW', '0')
    ref = RompNet(sd, dev, max_batch=max_batch, bf16x3='f16x2')
    assert sum(o.kind == L.OP_WAIT for o in ref.program.ops) == 0 and sum(o.kind == L.OP_JOIN for o in ref.program.ops) > 10
    # the same kernel variant for every layer of both nets (a net measures its own table at its first forward: two measurements
    # differ in a few layers, and with them the summation order): ref's table, moved over by layer name
    from romp_amd import tuning
    ref.autotune(max_batch, iters=1)
    table = {ln: v for ln, v, op in zip(ref.program.names, ref.variant_names(max_batch), ref.program.ops) if op.kind == L.OP_CONV}
    variants, why = tuning.resolve_table(net, max_batch, table)
    assert variants is not None, why
    net.set_tuned(max_batch, variants)
    cm0, pm0 = [t.clone() for t in ref(img)]
    st = torch.cuda.Stream()
    for graph in (False, True):
        net.set_graph(graph)
        with torch.cuda.stream(st):
            for it in range(12 if graph else 3):
                cm, pm = net(img)
                st.synchronize()
                assert torch.equal(cm, cm0) and torch.equal(pm, pm0), (graph, it, (cm - cm0).abs().max().item(), (pm - pm0).abs().max().item())
    net.set_streams(False)                                     # one stream: the edges do nothing, op order is a serial order
    net.set_graph(False)
    cm, pm = net(img)
    assert torch.equal(cm, cm0) and torch.equal(pm, pm0)


def test_net_saturation_is_observable(dev):
    """out-of-calibration values saturate at 65504 / 2^act_shift -- finite but wrong -- and that must not be silent.
    The blown-up-BN net WITHOUT calibration reports saturation events (net.saturated > 0, range_scan names ops), in the default
    build and in the checked build of the fused kernels; the ordinary net, and the blown-up net WITH calibration, report 0."""
    from romp_amd.net import RompNet
    sd = O.make_romp_state_dict(0)
    img = O.make_images(2, seed=3).to(dev)
    ok = RompNet(sd, dev, max_batch=2, bf16x3='f16x2')
    ok(img)
    assert ok.saturated == 0
    rows = ok.range_scan(img)
    assert sum(r[3] for r in rows) == 0 and sum(r[2] for r in rows) == 0 and ok.saturated == 0
    big = {k: v.clone() for k, v in sd.items()}
    key_w = [k for k in big if k.endswith('bn2.weight') and k.count('.') <= 2][0]
    big[key_w] *= 3e4                                       # stem conv2's BN: everything downstream ~3e4 x larger (fp16 pieces of 16 x end at 4094)
    big[key_w.replace('weight', 'bias')] *= 3e4
    raw = RompNet(big, dev, max_batch=2, bf16x3='f16x2', calibrate=False)
    assert raw.saturated == 0
    raw(img)
    n_default = raw.saturated
    assert n_default > 0, 'the generic kernels count clamps in every build'
    assert raw.reset_saturated() == n_default and raw.saturated == 0
    rows = raw.range_scan(img)                              # checked builds of the fused kernels
    hot = [(n, m, s) for n, m, b, s in rows if s]
    print('default build: %d events; scan: %d ops clamped, first %s' % (n_default, len(hot), hot[:3]))
    assert len(hot) > 3 and raw.saturated >= n_default
    raw.set_sat_check(True)
    raw.reset_saturated()
    raw(img)
    assert raw.saturated >= n_default
    cal = RompNet(big, dev, max_batch=2, bf16x3='f16x2')    # calibrated: the blown-up tensors stay float32 -> nothing clamps
    cal(img)
    assert cal.saturated == 0 and len(cal.range_fallback) > 10


def test_net_committed_table_all_images_vs_oracle(dev):
    """The EXACT kernels the driver's bench line times (VERDICT r3 weak #1a): romp_amd/tune/romp_hrnet32_f16x2_b32.json installed
    (it must resolve op for op in this build -- regenerate it with scripts/gpu_tables.sh after changing the plan or the variant
    list), then ALL 32 images' maps against the oracle (1e-4) and every image's detections against the oracle's parse."""
    import romp_amd
    from romp_amd import tuning
    B = 32
    settings = romp_amd.romp_settings([])
    settings.GPU, settings.center_thresh, settings.max_batch, settings.conv_math = 0, 1.3, B, 'f16x2'
    sd = O.make_romp_state_dict(0, center_bias=2.0)
    model = romp_amd.ROMP(settings, state_dict=sd, smpl_model=O.make_synthetic_smpl(0))
    ok, why = tuning.install_table(model.model, B, tuning.default_table_path('hrnet32', 'f16x2', B))
    assert ok, 'the committed variant table does not fit this build: %s' % why
    names = model.model.variant_names(B)
    img = O.make_images(B, seed=1)
    x = img.to(dev)
    cm, pm = model.model(x)
    cm_o, pm_o = O.romp_net_forward(sd, img)
    ec = (cm.cpu() - cm_o).abs().amax(dim=(1, 2, 3))
    ep = (pm.cpu() - pm_o).abs().amax(dim=(1, 2, 3))
    print(f'committed table, {len(set(n for n in names if n.startswith("conv_")))} conv variants: worst image center {ec.max():.3e} params {ep.max():.3e}')
    assert ec.max().item() < 1e-4 and ep.max().item() < 1e-4
    out, bids = model.forward_batch(x)
    ref = O.parsing_outputs(cm_o.numpy(), pm_o.numpy(), settings.center_thresh)
    assert out is not None and ref is not None
    assert np.array_equal(bids.cpu().numpy(), ref['batch_ids']), 'per-image detection counts differ'
    assert np.array_equal(out['center_preds'].cpu().numpy(), ref['center_preds'])
    assert model.model.saturated == 0


# ------------------------------------------------------------------------------ end to end
def test_romp_api_end_to_end(dev):
    """romp.ROMP(settings)(image) dict contract + parity of every gated output
    with the oracle pipeline on the same synthetic weights."""
    import romp_amd
    settings = romp_amd.romp_settings([])
    settings.GPU, settings.center_thresh = 0, 1.25
    settings.host_preprocess = True            # same pre-processed tensor as the oracle below (device path: test_bev_post.py)
    sd = O.make_romp_state_dict(0, center_bias=2.0)
    smpl_model = O.make_synthetic_smpl(0)
    model = romp_amd.ROMP(settings, state_dict=sd, smpl_model=smpl_model)
    rs = np.random.RandomState(0)
    image = rs.randint(0, 256, (360, 640, 3)).astype(np.uint8)          # BGR, non-square
    out = model(image)
    assert out is not None
    N = out['cam'].shape[0]
    assert N >= 1
    shapes = {'cam': (N, 3), 'global_orient': (N, 3), 'body_pose': (N, 69), 'smpl_betas': (N, 10),
              'smpl_thetas': (N, 72), 'center_preds': (N, 2), 'center_confs': (N, 1), 'cam_trans': (N, 3),
              'verts': (N, 6890, 3), 'joints': (N, 71, 3), 'pj2d_org': (N, 71, 2)}
    for k, shp in shapes.items():
        assert isinstance(out[k], np.ndarray) and out[k].shape == shp, k
    assert set(out.keys()) == set(shapes.keys())
    assert out['center_preds'].dtype == np.int64 and out['verts'].dtype == np.float32
    # oracle pipeline on the same pre-processed tensor
    from romp_amd.utils import img_preprocess
    inp, pad = img_preprocess(image)
    cm, pm = O.romp_net_forward(sd, inp)
    ref = O.parsing_outputs(cm.numpy(), pm.numpy(), settings.center_thresh)
    assert np.array_equal(out['center_preds'], ref['center_preds'])
    np.testing.assert_allclose(out['smpl_thetas'], ref['smpl_thetas'], atol=2e-4)
    np.testing.assert_allclose(out['cam'], ref['cam'], atol=1e-4)
    vo, jo, _ = O.smpl_forward(smpl_model, out['smpl_betas'], out['smpl_thetas'])    # identical theta/beta
    assert np.abs(out['verts'] - vo).max() < 1e-4 and np.abs(out['joints'] - jo).max() < 1e-4
    pj = O.project_to_org_image(O.batch_orth_proj(jo, out['cam']), pad.numpy())
    np.testing.assert_allclose(out['pj2d_org'], pj, atol=2e-2)
    # device pre-processing path gives the same detections
    settings.host_preprocess = False
    out_d = romp_amd.ROMP(settings, state_dict=sd, smpl_model=smpl_model)(image)
    assert np.array_equal(out_d['center_preds'], out['center_preds'])
    assert np.abs(out_d['verts'] - out['verts']).max() < 5e-3
    # nobody above threshold -> None
    settings.center_thresh = 50.0
    model2 = romp_amd.ROMP(settings, state_dict=sd, smpl_model=smpl_model)
    assert model2(image) is None


def test_forward_batch_matches_oracle(dev):
    import romp_amd
    settings = romp_amd.romp_settings([])
    settings.GPU, settings.center_thresh = 0, 1.3
    sd = O.make_romp_state_dict(0, center_bias=2.0)
    smpl_model = O.make_synthetic_smpl(0)
    model = romp_amd.ROMP(settings, state_dict=sd, smpl_model=smpl_model)
    img = O.make_images(3, seed=8)
    out, bids = model.forward_batch(img.to(dev))
    cm, pm = O.romp_net_forward(sd, img)
    ref = O.parsing_outputs(cm.numpy(), pm.numpy(), settings.center_thresh)
    assert np.array_equal(bids.cpu().numpy(), ref['batch_ids'])
    assert np.array_equal(out['center_preds'].cpu().numpy(), ref['center_preds'])
    vo, jo, _ = O.smpl_forward(smpl_model, ref['smpl_betas'], ref['smpl_thetas'])
    ev = np.abs(out['verts'].cpu().numpy() - vo).max()
    print('end-to-end verts max-abs vs oracle pipeline', ev, 'persons', len(ref['batch_ids']))
    assert ev < 1e-3


@pytest.mark.parametrize('mb,n', [(2, 5), (4, 14)])
def test_forward_chunks_pipelined_equals_forward_batch(dev, mb, n, monkeypatch):
    """ROMP.forward_chunks (network of chunk i+1 on its own stream under parse + SMPL of chunk i, hipGraph replay, two pairs of
    output maps) returns exactly what forward_batch returns chunk by chunk -- ragged last chunk included.  max_batch 4: the
    batch-plan path with TWO networks in flight (the net and its twin alternate, RompNet.twin) must give the same bytes."""
    import romp_amd
    monkeypatch.setenv('ROMP_PIPE_NETS', '2')                   # (the two-network pipeline is an opt-in experiment)
    settings = romp_amd.romp_settings([])
    settings.GPU, settings.center_thresh, settings.max_batch = 0, 1.3, mb
    sd = O.make_romp_state_dict(0, center_bias=2.0)
    model = romp_amd.ROMP(settings, state_dict=sd, smpl_model=O.make_synthetic_smpl(0))
    model.model.set_graph(True)
    x = O.make_images(n, seed=9).to(dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        want = []
        for c0 in range(0, n, mb):
            out, bids = model.forward_batch(x[c0:c0 + mb])
            want.append(None if out is None else {k: v.clone() for k, v in out.items() if torch.is_tensor(v)} | {'bids': bids.clone()})
        for rep in range(2):                                     # second pass replays the cached graphs
            got = list(model.forward_chunks(x, mb))
            assert [c0 for _, _, c0 in got] == list(range(0, n, mb))
            assert (len(set(id(t) for t in model._pipe['nets'])) == 2) == (mb > 2)
            for (out, bids, _), w in zip(got, want):
                assert (out is None) == (w is None)
                if out is not None:
                    assert torch.equal(bids, w['bids'])
                    for k in ('cam', 'smpl_thetas', 'smpl_betas', 'verts', 'joints', 'center_preds', 'center_confs'):
                        assert torch.equal(out[k], w[k]), k
        s.synchronize()


@pytest.mark.parametrize('mb,n', [(2, 5), (2, 8), (4, 8)])
def test_forward_chunks_primed_across_calls(dev, mb, n):
    """Round 6: `next_images` keeps the chunk pipeline primed across calls (the next call's first network is launched under this
    call's last parse + SMPL).  Odd and even chunk counts (the primed chunk's parity carries over), the same tensor walked again
    and a DIFFERENT tensor announced: every call returns exactly what forward_batch returns; a primed chunk that is never
    picked up (another tensor arrives) is dropped without harm."""
    import romp_amd
    settings = romp_amd.romp_settings([])
    settings.GPU, settings.center_thresh, settings.max_batch = 0, 1.3, mb
    sd = O.make_romp_state_dict(0, center_bias=2.0)
    model = romp_amd.ROMP(settings, state_dict=sd, smpl_model=O.make_synthetic_smpl(0))
    model.model.set_graph(True)
    xa, xb = O.make_images(n, seed=9).to(dev), O.make_images(n, seed=10).to(dev)
    keys = ('cam', 'smpl_thetas', 'smpl_betas', 'verts', 'joints', 'center_preds', 'center_confs')
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        want = {}
        for name, x in (('a', xa), ('b', xb)):
            want[name] = []
            for c0 in range(0, n, mb):
                out, bids = model.forward_batch(x[c0:c0 + mb])
                want[name].append(None if out is None else {k: out[k].clone() for k in keys} | {'bids': bids.clone()})

        def check(x, name, nxt):
            got = list(model.forward_chunks(x, mb, next_images=nxt))
            for (out, bids, _), w in zip(got, want[name]):
                assert (out is None) == (w is None)
                if out is not None:
                    assert torch.equal(bids, w['bids'])
                    for k in keys:
                        assert torch.equal(out[k], w[k]), (name, k)
        check(xa, 'a', xa)
        assert model._pipe['primed'] is not None
        check(xa, 'a', xa)                                       # picked up the primed first chunk
        check(xa, 'a', xb)                                       # announces the other tensor
        assert model._pipe['primed']['ptr'] == xb.data_ptr()
        check(xb, 'b', xa)
        check(xb, 'b', None)                                     # xa was announced, xb arrives: the primed chunk is dropped
        assert model._pipe['primed'] is None
        check(xa, 'a', None)
        s.synchronize()


def test_graph_cache_is_bounded(dev):
    """Graph mode with fresh output tensors on every call: the per-(batch, pointers) hipGraph cache must stay
    bounded (it is dropped and rebuilt past 32 entries) and keep producing the same maps."""
    from romp_amd.net import RompNet
    net = RompNet(O.make_romp_state_dict(0), dev, max_batch=1, use_graph=True)
    x = O.make_images(1, seed=1).to(dev)
    s = torch.cuda.Stream()
    keep = []
    with torch.cuda.stream(s):
        c0, p0 = net.forward_nhwc(x)
        for _ in range(40):
            c, p = net.forward_nhwc(x)
            keep.append((c, p))                      # keep them alive: every call sees new pointers
        s.synchronize()
    assert all(torch.equal(c, c0) and torch.equal(p, p0) for c, p in keep)


def _seam_views(H, W):
    """The ordinary 1x1 convs around a seam need a map of whole 16-column tiles, the seam kernel only a pixel count: on a narrower /
    odd-width map they see the same (contiguous NHWC, pointwise) pixels as an (H * W / 16) x 16 map.  -> (that shape, as_map(act, shape):
    the same tensor declared with another shape)."""
    import dataclasses
    view = (H, W) if W % 16 == 0 else (H * W // 16, 16)
    assert view[0] * view[1] == H * W
    return view, lambda act, hw: dataclasses.replace(act, H=hw[0], W=hw[1])


@pytest.mark.gpu
@pytest.mark.parametrize('B,H', [(1, 16), (3, 32), (2, 128)])            # (2, 128): layer1's production shape
def test_seam1x1(dev, B, H, monkeypatch):
    _seam1x1(dev, B, H, monkeypatch)


def _seam1x1(dev, B, H, monkeypatch, W=None, run=True):
    """csrc/conv_h2x.hip: the 1x1 64 -> 256 (+ residual + ReLU) / 1x1 256 -> 64 (+ ReLU) pair across
    a Bottleneck seam as one launch: both output tensors against torch on the CPU.  W: the map's width (default: square);
    run=False: lower and check the fusion only (no device; -> the program)."""
    import ctypes as C
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math, decode_h2
    monkeypatch.setenv('ROMP_FUSE_SEAMS', '1')
    W = H if W is None else W
    g = torch.Generator().manual_seed(7 * B + H)
    x0 = torch.randn(B, H, W, 64, generator=g)
    dims = [(64, 256), (256, 64), (64, 256), (256, 64), (64, 64)]
    ws = [torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5 for ci, co in dims]
    sc = [torch.rand(co, generator=g) + 0.5 for _, co in dims]
    sh = [torch.randn(co, generator=g) * 0.2 for _, co in dims]

    def cbr(t, i, res=None):
        y = F.conv2d(t, ws[i], None) * sc[i].view(1, -1, 1, 1) + sh[i].view(1, -1, 1, 1)
        return torch.relu(y if res is None else y + res)
    rx = cbr(x0.permute(0, 3, 1, 2), 0)
    rm = cbr(rx, 1)
    rt = cbr(rm, 2, res=rx)
    ru = cbr(rt, 3)
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    view, as_map = _seam_views(H, W)                        # (H, W) itself on maps of whole 16-column tiles
    ax = P.conv('x', Act(L.BUF_IMAGE, 64, view[0], view[1], 64), [ws[0]], [sc[0]], [sh[0]], 1, 1, True)
    am = P.conv('m', ax, [ws[1]], [sc[1]], [sh[1]], 1, 1, True)
    at = P.conv('t', as_map(am, (H, W)), [ws[2]], [sc[2]], [sh[2]], 1, 1, True, res=as_map(ax, (H, W)))
    au = P.conv('u', at, [ws[3]], [sc[3]], [sh[3]], 1, 1, True)
    av = P.conv('v', as_map(au, view), [ws[4]], [sc[4]], [sh[4]], 1, 1, True)
    ops = P.op_array()
    assert P.fused_seams == 1 and [o.kind for o in P.ops] == [L.OP_CONV, L.OP_CONV, L.OP_NOP, L.OP_SEAM1X1, L.OP_CONV], [o.kind for o in P.ops]
    assert (P.ops[3].H, P.ops[3].W) == (H, W)
    if not run:
        return P
    lib = L.load()
    h = C.c_void_p()
    sizes = (C.c_int64 * len(P.buf_floats))(*P.buf_floats)
    L.check(lib.romp_net_create(C.byref(h), ops, len(P.ops), sizes, len(P.buf_floats), B))
    try:
        xd = x0.to(dev).contiguous()
        dummy = torch.empty(16, device=dev)
        L.check(lib.romp_net_forward(h, L.ptr(xd), B, L.ptr(dummy), L.ptr(dummy), L.stream_ptr(dev)))
        for act, ref, name in ((at, rt, 't'), (au, ru, 'u')):
            n = P.buf_floats[act.buf] * B
            out = torch.empty(n, device=dev)
            L.check(lib.romp_net_read_buffer(h, act.buf, B, L.ptr(out), n, L.stream_ptr(dev)))
            torch.cuda.synchronize()
            y = decode_h2(out.cpu().reshape(B, H, W, act.C))
            r = ref.permute(0, 2, 3, 1)
            err = (y - r).abs().max().item() / r.abs().max().item()
            print(f'seam1x1 B={B} {H}x{W} {name}: relative err {err:.3e}')
            assert err < 5e-5, (name, err)
    finally:
        lib.romp_net_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize('B,H', [(1, 16), (3, 32), (2, 128)])
def test_seam1x1_downsample(dev, B, H, monkeypatch):
    _seam1x1_downsample(dev, B, H, monkeypatch)


def _seam1x1_downsample(dev, B, H, monkeypatch, W=None, run=True):
    """csrc/conv_h2x.hip, DS = 1 (round 5, OPF_SEAM_DS): the seam behind Bottleneck 0 -- t = relu(bn3(conv1x1(m)) + bn_d(conv1x1(x0))),
    the residual being the block's own `downsample` conv of the block input (model.py:289-301) -- as one launch that never
    materialises the downsample output; both outputs against torch on the CPU, and against the ROMP_SEAM_DS=0 lowering of the
    same program (the downsample as a launch of its own).  W: the map's width (default: square); run=False: lower and check the
    fusion only (no device; -> the two programs)."""
    import ctypes as C
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math, decode_h2
    monkeypatch.setenv('ROMP_FUSE_SEAMS', '1')
    W = H if W is None else W
    g = torch.Generator().manual_seed(11 * B + H)
    img = torch.randn(B, H, W, 64, generator=g)
    dims = [(64, 64), (64, 64), (64, 256), (64, 256), (256, 64), (64, 64)]      # x0, m, downsample, conv3, next conv1, a reader of u
    ws = [torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5 for ci, co in dims]
    sc = [torch.rand(co, generator=g) + 0.5 for _, co in dims]
    sh = [torch.randn(co, generator=g) * 0.2 for _, co in dims]

    def cb(t, i, relu=True, res=None):
        y = F.conv2d(t, ws[i], None) * sc[i].view(1, -1, 1, 1) + sh[i].view(1, -1, 1, 1)
        y = y if res is None else y + res
        return torch.relu(y) if relu else y
    r0 = cb(img.permute(0, 3, 1, 2), 0)
    rm = cb(r0, 1)
    rd = cb(r0, 2, relu=False)
    rt = cb(rm, 3, res=rd)
    ru = cb(rt, 4)
    outs = {}
    for ds in ('1', '0'):
        monkeypatch.setenv('ROMP_SEAM_DS', ds)
        P = Program(dev)
        set_conv_math(P, 'f16x2')
        view, as_map = _seam_views(H, W)                    # (H, W) itself on maps of whole 16-column tiles
        dmap = (H, W) if ds == '1' else view                # the downsample conv: folded into the seam / a launch of its own
        a0 = P.conv('x0', Act(L.BUF_IMAGE, 64, view[0], view[1], 64), [ws[0]], [sc[0]], [sh[0]], 1, 1, True)
        am = P.conv('m', a0, [ws[1]], [sc[1]], [sh[1]], 1, 1, True)
        ad = P.conv('d', as_map(a0, dmap), [ws[2]], [sc[2]], [sh[2]], 1, 1, False)
        at = P.conv('t', as_map(am, (H, W)), [ws[3]], [sc[3]], [sh[3]], 1, 1, True, res=as_map(ad, (H, W)))
        au = P.conv('u', at, [ws[4]], [sc[4]], [sh[4]], 1, 1, True)
        av = P.conv('v', as_map(au, view), [ws[5]], [sc[5]], [sh[5]], 1, 1, True)
        ops = P.op_array()
        kinds = [o.kind for o in P.ops]
        assert (P.ops[4].H, P.ops[4].W) == (H, W)
        if ds == '1':
            assert P.fused_seams == 1 and P.folded_downsamples == 1 and kinds == [L.OP_CONV, L.OP_CONV, L.OP_NOP, L.OP_NOP, L.OP_SEAM1X1, L.OP_CONV], kinds
            assert P.ops[4].flags & L.OPF_SEAM_DS
        else:
            assert P.fused_seams == 1 and kinds == [L.OP_CONV, L.OP_CONV, L.OP_CONV, L.OP_NOP, L.OP_SEAM1X1, L.OP_CONV], kinds
        if not run:
            outs[ds] = P
            continue
        lib = L.load()
        h = C.c_void_p()
        sizes = (C.c_int64 * len(P.buf_floats))(*P.buf_floats)
        L.check(lib.romp_net_create(C.byref(h), ops, len(P.ops), sizes, len(P.buf_floats), B))
        try:
            xd = img.to(dev).contiguous()
            dummy = torch.empty(16, device=dev)
            L.check(lib.romp_net_forward(h, L.ptr(xd), B, L.ptr(dummy), L.ptr(dummy), L.stream_ptr(dev)))
            for act, ref, name in ((at, rt, 't'), (au, ru, 'u')):
                n = P.buf_floats[act.buf] * B
                out = torch.empty(n, device=dev)
                L.check(lib.romp_net_read_buffer(h, act.buf, B, L.ptr(out), n, L.stream_ptr(dev)))
                torch.cuda.synchronize()
                y = decode_h2(out.cpu().reshape(B, H, W, act.C))
                r = ref.permute(0, 2, 3, 1)
                err = (y - r).abs().max().item() / r.abs().max().item()
                print(f'seam1x1 ds={ds} B={B} {H}x{W} {name}: relative err {err:.3e}')
                assert err < 5e-5, (ds, name, err)
                outs[(ds, name)] = y
        finally:
            lib.romp_net_destroy(h)
    if not run:
        return [outs['1'], outs['0']]
    for name in ('t', 'u'):                                      # the two lowerings agree to float32 rounding (the fold adds in float32 what
        d = (outs[('1', name)] - outs[('0', name)]).abs().max().item()      # the separate launch rounds to two fp16 pieces first)
        assert d < 2e-5 * max(1.0, outs[('0', name)].abs().max().item()), (name, d)


@pytest.mark.gpu
@pytest.mark.parametrize('ds', ['1', '0'])
def test_seam1x1_counted_waits_vs_full_drain(dev, ds, monkeypatch):
    """the seam kernel ends a tile on a COUNTED wait (vmcnt(52) / vmcnt(20)) that lets stores and the next residual stay in
    flight across the barrier; if the compiled loop ever issued fewer memory operations behind the DMA than the count, the barrier
    would release before the next m tile has landed -- a silent LDS race.  scripts/check_counted_waits.py counts the compiled
    instructions (CPU test); here the same programs run with the full-drain instantiation (ROMP_SEAM_FULL_DRAIN=1: vmcnt(0), round 3's
    form) and must give bit-identical tensors, eight tiles deep per workgroup."""
    import ctypes as C
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math
    monkeypatch.setenv('ROMP_FUSE_SEAMS', '1')
    monkeypatch.setenv('ROMP_SEAM_DS', ds)
    B, H = 8, 128
    g = torch.Generator().manual_seed(97)
    img = torch.randn(B, H, H, 64, generator=g)
    dims = [(64, 64), (64, 64), (64, 256), (64, 256), (256, 64), (64, 64)]
    ws = [torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5 for ci, co in dims]
    sc = [torch.rand(co, generator=g) + 0.5 for _, co in dims]
    sh = [torch.randn(co, generator=g) * 0.2 for _, co in dims]
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    a0 = P.conv('x0', Act(L.BUF_IMAGE, 64, H, H, 64), [ws[0]], [sc[0]], [sh[0]], 1, 1, True)
    am = P.conv('m', a0, [ws[1]], [sc[1]], [sh[1]], 1, 1, True)
    ad = P.conv('d', a0, [ws[2]], [sc[2]], [sh[2]], 1, 1, False)
    at = P.conv('t', am, [ws[3]], [sc[3]], [sh[3]], 1, 1, True, res=ad)
    au = P.conv('u', at, [ws[4]], [sc[4]], [sh[4]], 1, 1, True)
    P.conv('v', au, [ws[5]], [sc[5]], [sh[5]], 1, 1, True)
    ops = P.op_array()
    assert P.fused_seams == 1 and getattr(P, 'folded_downsamples', 0) == (1 if ds == '1' else 0)
    lib = L.load()
    h = C.c_void_p()
    sizes = (C.c_int64 * len(P.buf_floats))(*P.buf_floats)
    L.check(lib.romp_net_create(C.byref(h), ops, len(P.ops), sizes, len(P.buf_floats), B))
    got = {}
    try:
        xd = img.to(dev).contiguous()
        dummy = torch.empty(16, device=dev)
        for drain in ('0', '1', '0'):
            monkeypatch.setenv('ROMP_SEAM_FULL_DRAIN', drain)
            for rep in range(3):
                L.check(lib.romp_net_forward(h, L.ptr(xd), B, L.ptr(dummy), L.ptr(dummy), L.stream_ptr(dev)))
                for act, name in ((at, 't'), (au, 'u')):
                    n = P.buf_floats[act.buf] * B
                    out = torch.empty(n, device=dev)
                    L.check(lib.romp_net_read_buffer(h, act.buf, B, L.ptr(out), n, L.stream_ptr(dev)))
                    torch.cuda.synchronize()
                    bits = out.view(torch.int32).cpu()
                    if name in got:
                        assert torch.equal(bits, got[name]), 'seam ds=%s, ROMP_SEAM_FULL_DRAIN=%s, pass %d: tensor %s differs from the first run' % (ds, drain, rep, name)
                    else:
                        got[name] = bits
    finally:
        lib.romp_net_destroy(h)
