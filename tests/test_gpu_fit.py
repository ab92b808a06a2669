"""Fitting to 2-D keypoints on the GPU (run with -m gpu): romp_fit_reproject and romp_fit_adam (csrc/fit.hip) and
romp_amd.fitting on top of them, against the float64 CPU restatements of tests/test_fit.py.

Tolerance: the rule of tests/test_gpu_smpl_grad.py.  error = max |delta| / max |float64 reference| per tensor; every case
also evaluates the restatement in float32 on the CPU and requires  err_HIP <= 8 * max(err_CPU_f32, FLOOR).  The sums here have
at most 71 terms, so the float32 CPU error can be exactly 0; FLOOR = 4 * 2^-24 is a handful of float32 roundings, and
nothing a wrong sign or a missing term could hide under.  Every figure is printed before it is asserted (pytest -s).

Four waves share a workgroup of fit_reproject_kernel (one wave per person), so N = 1, 3, 5 are a lone person, a partial
workgroup, and a workgroup plus one."""
import ctypes
import types

import numpy as np
import pytest
import torch

from test_fit import adam_loop_torch, fit_loop_torch, project_torch, reproject_torch
from test_smpl_grad import model_for, smpl_torch

pytestmark = pytest.mark.gpu
FLOOR = 4 * 2.0 ** -24
J = 71
RESIDUAL = 0.05                                                  # the noise put on the targets, per coordinate


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


_LAYERS = {}


def layer(dev, n_betas=10):
    from romp_amd.smpl import SMPL
    if n_betas not in _LAYERS:
        model = model_for(n_betas)
        _LAYERS[n_betas] = (model, SMPL(model, model_type='smpl' if n_betas == 10 else 'smpla').to(dev))
    return _LAYERS[n_betas]


def scaled(x, ref):
    return float((x.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def within(tag, name, hip, f32, ref):
    """The rule of the module docstring for one tensor; prints the figures, returns whether it holds."""
    assert hip.shape == ref.shape and hip.dtype == torch.float32 and bool(torch.isfinite(hip).all()), (tag, name)
    e_hip, e_f32 = scaled(hip, ref), scaled(f32, ref)
    print(f'{tag} {name}: max|ref| {float(ref.abs().max()):.3g} err_hip {e_hip:.3e} err_cpu_f32 {e_f32:.3e} '
          f'bound {8 * max(e_f32, FLOOR):.3e}')
    return e_hip <= 8 * max(e_f32, FLOOR)


def case(N, K, camera, seed, inds=None):
    """Seeded float32 joints (N,71,3), cam (N,3), targets (N,K,2) = the projection of the picked joints plus noise of
    RESIDUAL per coordinate, conf (N,K) in (0.2, 1].  Perspective: the depth of every joint, p.z, lies in [0.5, 8]."""
    g = torch.Generator().manual_seed(seed)
    joints = 0.4 * torch.randn(N, J, 3, generator=g)
    if camera == 'weak':
        cam = torch.cat([0.5 + torch.rand(N, 1, generator=g), 0.2 * torch.randn(N, 2, generator=g)], 1)
    else:
        joints[:, :, 2] = joints[:, :, 2].clamp(-1.2, 1.2)
        cam = torch.cat([0.3 * torch.randn(N, 2, generator=g), 1.7 + 5.1 * torch.rand(N, 1, generator=g)], 1)
        cam[0, 2] = 1.7                                                             # the near end: p.z from 0.5
        joints[0, 0, 2] = -1.2
        z = joints[:, :, 2] + cam[:, None, 2]
        assert float(z.min()) >= 0.5 - 1e-6 and float(z.max()) <= 8
    X = joints[:, :K] if inds is None else joints[:, torch.as_tensor(inds)]
    kp = (project_torch(X, cam, camera) + RESIDUAL * torch.randn(N, K, 2, generator=g).double()).float()
    conf = 0.2 + 0.8 * torch.rand(N, K, generator=g)
    return joints, cam, kp, conf


def cpu_eval(joints, cam, kp, conf, inds, sigma, camera, dtype):
    j, c = joints.to(dtype).clone().requires_grad_(True), cam.to(dtype).clone().requires_grad_(True)
    loss = reproject_torch(j, c, kp, conf, inds, sigma, camera, dtype)
    loss.sum().backward()                                        # loss[n] depends on person n alone
    return loss.detach().double(), j.grad.double(), c.grad.double()


def hip_eval(dev, joints, cam, kp, conf, inds, sigma, camera, history_rows=0, row=0):
    """The C entry on buffers filled with NaN, so that an element it does not write shows."""
    from romp_amd import fitting as F
    N = joints.shape[0]
    nan = lambda *s: torch.full(s, float('nan'), device=dev, dtype=torch.float32)
    loss, gj, gc = nan(N), nan(N, joints.shape[1], 3), nan(N, 3)
    hist = nan(history_rows, N) if history_rows else None
    inds_c = F._inds(inds, kp.shape[1])
    F._reproject(joints.to(dev).contiguous(), cam.to(dev).contiguous(), kp.to(dev).contiguous(), None if conf is None else conf.to(dev).contiguous(),
                 inds_c, F.CAMERAS[camera], 443.4, 256., sigma, loss, gj, gc, hist, row)
    torch.cuda.synchronize()
    return (loss, gj, gc) if hist is None else (loss, gj, gc, hist)


def check(dev, N, K, camera, sigma, seed, inds=None, with_conf=True):
    joints, cam, kp, conf = case(N, K, camera, seed, inds)
    conf = conf if with_conf else None
    ref = cpu_eval(joints, cam, kp, conf, inds, sigma, camera, torch.float64)
    f32 = cpu_eval(joints, cam, kp, conf, inds, sigma, camera, torch.float32)
    got = hip_eval(dev, joints, cam, kp, conf, inds, sigma, camera)
    tag = f'N={N} K={K} {camera} sigma={sigma:.3g}'
    ok = [within(tag, name, h, f, r) for name, h, f, r in zip(('loss', 'grad_joints', 'grad_cam'), got, f32, ref)]
    picked = list(range(K)) if inds is None else list(inds)
    rest = [j for j in range(J) if j not in picked]
    assert bool((got[1][:, rest] == 0).all()), 'a joint that was not picked has a gradient'
    assert all(ok)


# ------------------------------------------------------------------------------------------------ loss and gradients
@pytest.mark.parametrize('sigma', [0., 0.1 * RESIDUAL * 2 ** 0.5])     # plain squares; Geman-McClure at a tenth of the typical residual
@pytest.mark.parametrize('camera', ['weak', 'perspective'])
@pytest.mark.parametrize('K', [1, 24, 65, 71])                         # one lane; part of a wave; one lane of the second round; every joint
@pytest.mark.parametrize('N', [1, 3, 5])
def test_loss_and_gradients(dev, N, K, camera, sigma):
    check(dev, N, K, camera, sigma, seed=100 * N + K)


@pytest.mark.parametrize('camera', ['weak', 'perspective'])
@pytest.mark.parametrize('K', [24, 71])
def test_permuted_joint_inds(dev, K, camera):
    inds = torch.randperm(J, generator=torch.Generator().manual_seed(K))[:K].tolist()
    assert inds != sorted(inds)
    check(dev, 5, K, camera, 0.007, seed=7, inds=inds)


@pytest.mark.parametrize('camera', ['weak', 'perspective'])
def test_null_conf_stands_for_ones(dev, camera):
    check(dev, 3, 65, camera, 0., seed=8, with_conf=False)
    joints, cam, kp, _ = case(3, 65, camera, 8)
    a = hip_eval(dev, joints, cam, kp, None, None, 0., camera)
    b = hip_eval(dev, joints, cam, kp, torch.ones(3, 65), None, 0., camera)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ edge cases
@pytest.mark.parametrize('camera', ['weak', 'perspective'])
def test_invisible_keypoints(dev, camera):
    """Person 1 has every conf 0: loss 0 and all gradients 0, every element written.  Person 0 has a NaN target at a conf-0
    keypoint, a -2 target and a conf-0 keypoint: all three drop out, the rest is the float64 figure."""
    joints, cam, kp, conf = case(3, 65, camera, 9)
    conf[1] = 0
    kp[0, 3] = float('nan')
    conf[0, 3] = 0
    kp[0, 64, 1] = -2.
    conf[0, 10] = 0
    kp[2, 5, 0] = float('nan')                                    # a NaN target alone fails `> -1.99`: invisible too
    ref = cpu_eval(joints, cam, torch.nan_to_num(kp, nan=-2.), conf, None, 0., camera, torch.float64)
    f32 = cpu_eval(joints, cam, torch.nan_to_num(kp, nan=-2.), conf, None, 0., camera, torch.float32)
    got = hip_eval(dev, joints, cam, kp, conf, None, 0., camera)
    for t in got:
        assert bool(torch.isfinite(t).all())
    assert float(got[0][1]) == 0 and bool((got[1][1] == 0).all()) and bool((got[2][1] == 0).all())
    assert bool((got[1][0, [3, 10, 64]] == 0).all()) and bool((got[1][2, 5] == 0).all())
    assert bool((got[1][0, [2, 4, 63]] != 0).any(1).all())
    assert all([within(f'invisible {camera}', n, h, f, r) for n, h, f, r in zip(('loss', 'grad_joints', 'grad_cam'), got, f32, ref)])


@pytest.mark.parametrize('camera', ['weak', 'perspective'])
@pytest.mark.parametrize('sigma', [0., 0.01])
def test_a_perfect_fit_has_no_loss_and_no_gradient(dev, camera, sigma):
    """Targets that are the device's own projection bits: joints and camera on a coarse binary grid, so that the float32
    projection by the project's own kernels is exact and equals the kernel's float64 one."""
    g = torch.Generator().manual_seed(10)
    joints = torch.randint(-64, 65, (3, J, 3), generator=g).float() / 64
    if camera == 'weak':
        cam = torch.tensor([[0.5, 0.25, -0.125], [1.0, 0., 0.5], [2.0, -0.5, 0.25]])
        kp = project_torch(joints, cam, camera).float()
        assert torch.equal(kp.double(), project_torch(joints, cam, camera))
        got = hip_eval(dev, joints, cam, kp, None, None, sigma, camera)
        assert all(bool((t == 0).all()) for t in got)
    else:                                                        # 443.4 / 256 is no binary fraction: the float64 projection, rounded
        cam = torch.tensor([[0.5, 0.25, 4.0], [1.0, 0., 3.0], [-0.5, 0.25, 6.0]])
        kp = project_torch(joints, cam, camera).float()
        got = hip_eval(dev, joints, cam, kp, None, None, sigma, camera)
        # residuals are one float32 rounding of a coordinate of size <= 1: e <= 2 (2^-24)^2 per keypoint
        assert float(got[0].max()) <= 2 * (2.0 ** -24) ** 2 and float(got[1].abs().max()) <= 2 * 2.0 ** -24 and float(got[2].abs().max()) <= 2 * 2.0 ** -24


def test_two_calls_give_equal_bits_and_the_history_row(dev):
    joints, cam, kp, conf = case(5, 65, 'perspective', 11)
    a = hip_eval(dev, joints, cam, kp, conf, None, 0.007, 'perspective', history_rows=3, row=2)
    b = hip_eval(dev, joints, cam, kp, conf, None, 0.007, 'perspective', history_rows=3, row=2)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    assert torch.equal(a[3][2], a[0]) and bool(torch.isnan(a[3][:2]).all())   # the row asked for, and nothing else


def test_a_side_stream_gives_the_default_streams_bits(dev):
    joints, cam, kp, conf = case(5, 71, 'weak', 12)
    want = hip_eval(dev, joints, cam, kp, conf, None, 0., 'weak')
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        got = hip_eval(dev, joints, cam, kp, conf, None, 0., 'weak')
    s.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(want, got))


# ------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize('camera,root_align', [('weak', False), ('perspective', True)])
def test_reprojection_loss_through_the_layer(dev, camera, root_align):
    from romp_amd.fitting import reprojection_loss
    model, smpl = layer(dev)
    N, K = 3, 24
    g = torch.Generator().manual_seed(13)
    betas, poses = torch.randn(N, 10, generator=g), 0.4 * torch.randn(N, 72, generator=g)
    cam = torch.tensor([[0.9, 0.05, -0.03], [0.7, -0.1, 0.08], [1.2, 0.2, 0.1]]) if camera == 'weak' else \
        torch.tensor([[0.1, -0.2, 3.0], [-0.3, 0.1, 5.0], [0.2, 0.3, 2.5]])
    inds = torch.randperm(J, generator=g)[:K].tolist()
    _, jt = smpl_torch(model, betas, poses, root_align, torch.float64)
    kp = (project_torch(jt[:, inds], cam, camera) + RESIDUAL * torch.randn(N, K, 2, generator=g).double()).float()
    conf = 0.2 + 0.8 * torch.rand(N, K, generator=g)
    weight = torch.tensor([1.0, 0.5, 2.0])                       # the incoming gradient differs per person

    def cpu(dtype):
        b, p, c = (t.to(dtype).clone().requires_grad_(True) for t in (betas, poses, cam))
        _, j = smpl_torch(model, b, p, root_align, dtype)
        loss = reproject_torch(j, c, kp, conf, inds, 0.01, camera, dtype)
        (loss * weight.to(dtype)).sum().backward()
        return loss.detach().double(), b.grad.double(), p.grad.double(), c.grad.double()

    ref, f32 = cpu(torch.float64), cpu(torch.float32)
    b, p, c = (t.to(dev).requires_grad_(True) for t in (betas, poses, cam))
    _, j, _ = smpl(b, p, root_align=root_align)
    loss = reprojection_loss(j, c, kp.to(dev), conf.to(dev), inds, sigma=0.01, camera=camera)
    assert loss.shape == (N,) and loss.grad_fn is not None
    (loss * weight.to(dev)).sum().backward()
    torch.cuda.synchronize()
    got = (loss.detach(), b.grad, p.grad, c.grad)
    assert all([within(f'autograd {camera}', n, h, f, r) for n, h, f, r in zip(('loss', 'betas.grad', 'poses.grad', 'cam.grad'), got, f32, ref)])


# ------------------------------------------------------------------------------------------------ romp_fit_adam
@pytest.mark.parametrize('priors', [False, True])
def test_adam_two_segments_five_steps(dev, priors):
    """(3,10) and (3,72) in one launch per step; supplied gradients +-(0.1 + |randn|), none near zero, so Adam's g / sqrt(v)
    cannot flip on rounding noise.  With priors: the narrow tensor has weights and no reference (zeros), the wide one both."""
    from romp_amd import lib as L
    h = L.load()
    g = torch.Generator().manual_seed(14)
    shapes = [(3, 10), (3, 72)]
    params = [torch.randn(s, generator=g) for s in shapes]
    grads = [[(0.1 + torch.randn(s, generator=g).abs()) * (torch.randint(0, 2, s, generator=g) * 2 - 1).float() for s in shapes]
             for _ in range(5)]
    refs = [None, torch.randn(shapes[1], generator=g)] if priors else [None, None]
    ws = [0.05 + 0.2 * torch.rand(10, generator=g), torch.cat([torch.zeros(3), 0.05 + 0.2 * torch.rand(69, generator=g)])] if priors \
        else [None, None]
    want = adam_loop_torch(params, grads, refs, ws, 0.02, torch.float64)
    f32 = adam_loop_torch(params, grads, refs, ws, 0.02, torch.float32)
    d = lambda t: None if t is None else t.to(dev).contiguous()
    p_d, r_d, w_d = [d(t) for t in params], [d(t) for t in refs], [d(t) for t in ws]
    m_d, v_d = [torch.zeros_like(t) for t in p_d], [torch.zeros_like(t) for t in p_d]
    g_d = [torch.empty_like(t) for t in p_d]
    segs = (L.FitSegment * 2)(*[L.FitSegment(p_d[i].data_ptr(), g_d[i].data_ptr(), m_d[i].data_ptr(), v_d[i].data_ptr(),
                                             None if r_d[i] is None else r_d[i].data_ptr(), None if w_d[i] is None else w_d[i].data_ptr(),
                                             shapes[i][0], shapes[i][1]) for i in range(2)])
    for step, gs in enumerate(grads):
        for i in range(2):
            g_d[i].copy_(gs[i])
        L.check(h.romp_fit_adam(segs, 2, 0.02, 0.9, 0.999, 1e-8, step + 1, L.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert all([within(f'adam priors={priors}', f'segment {i}', p_d[i], f32[i], want[i]) for i in range(2)])
    assert all(bool((p_d[i].cpu() != params[i]).all()) for i in range(2))          # every element took its steps


# ------------------------------------------------------------------------------------------------ KeypointFitter
def fit_case(model, camera, root_align, N=2, seed=40):
    g = torch.Generator().manual_seed(seed)
    b0, p0 = 0.5 * torch.randn(N, 10, generator=g), 0.2 * torch.randn(N, 72, generator=g)
    bt, pt = b0 + 0.3 * torch.randn(N, 10, generator=g), p0 + 0.1 * torch.randn(N, 72, generator=g)
    c0 = torch.tensor([[0.9, 0.05, -0.03], [0.7, -0.1, 0.08]]) if camera == 'weak' else torch.tensor([[0.1, -0.2, 3.0], [-0.3, 0.1, 5.0]])
    _, jt = smpl_torch(model, bt, pt, root_align, torch.float64)
    kp = project_torch(jt, c0 * 1.05, camera).float()
    conf = 0.2 + 0.8 * torch.rand(N, J, generator=g)
    conf[0, 5] = 0
    return b0, p0, c0, kp, conf


@pytest.mark.parametrize('camera,root_align', [('weak', False), ('perspective', True)])
def test_three_steps_equal_the_float64_loop(dev, camera, root_align):
    """Three steps at N = 2 against three steps of the float64 CPU loop (smpl_torch + reproject_torch + torch.optim.Adam with
    the priors added by hand), parameter by parameter; the yardstick is the same loop in float32."""
    from romp_amd.fitting import KeypointFitter
    model, smpl = layer(dev)
    b0, p0, c0, kp, conf = fit_case(model, camera, root_align)
    args = dict(steps=3, lr=0.02, sigma=0.05, w_betas=1e-3, w_pose=2e-3)
    want = fit_loop_torch(model, b0, p0, c0, kp, conf, None, camera=camera, root_align=root_align, dtype=torch.float64, **args)
    f32 = fit_loop_torch(model, b0, p0, c0, kp, conf, None, camera=camera, root_align=root_align, dtype=torch.float32, **args)
    got = KeypointFitter(smpl, camera=camera, root_align=root_align, **args).fit(b0, p0, c0, kp, conf)
    torch.cuda.synchronize()
    assert got['loss_history'].shape == (4, 2) and got['verts'].shape == (2, 6890, 3) and got['joints'].shape == (2, J, 3)
    ok = [within(f'fitter {camera}', k, got[k], f32[k], want[k]) for k in ('betas', 'poses', 'cam', 'loss_history')]
    for k, start in (('betas', b0), ('poses', p0), ('cam', c0)):
        assert float((got[k].cpu() - start).abs().max()) > 0.02    # it moved: three steps of lr 0.02
    v, j, _ = smpl(got['betas'], got['poses'], root_align=root_align)
    assert torch.equal(v, got['verts']) and torch.equal(j, got['joints'])      # the outputs belong to the returned parameters
    assert all(ok)


@pytest.mark.parametrize('camera,root_align,cpu_fall', [('weak', False, (22.8, 16.5)), ('perspective', True, (15.1, 15.0))])
def test_a_fit_that_converges(dev, camera, root_align, cpu_fall):
    """Targets: the projected joints of seeded beta*, theta* = 0.3 randn, cam*, computed by the device forward; start from
    zeros with the camera off by 10 %; the recipe's defaults (30 steps, lr 0.02, priors 1e-4).  The float64 CPU loop
    (fit_loop_torch) under this recipe falls, first loss / last loss per person, 22.8x and 16.5x with the weak camera and
    15.1x and 15.0x with the perspective one; the device must reach a third of that fall."""
    from romp_amd.fitting import KeypointFitter, reprojection_loss
    model, smpl = layer(dev)
    g = torch.Generator().manual_seed(5)
    bt, pt = torch.randn(2, 10, generator=g).to(dev), (0.3 * torch.randn(2, 72, generator=g)).to(dev)
    ct = (torch.tensor([[0.9, 0.05, -0.03], [0.7, -0.1, 0.08]]) if camera == 'weak' else torch.tensor([[0.1, -0.2, 3.0], [-0.3, 0.1, 5.0]])).to(dev)
    _, jt, _ = smpl(bt, pt, root_align=root_align)
    kp = project_torch(jt.cpu(), ct.cpu(), camera, torch.float32).to(dev)
    fitter = KeypointFitter(smpl, camera=camera, root_align=root_align)
    assert fitter.steps == 30 and fitter.lr == 0.02
    zeros_b, zeros_p, c0 = torch.zeros(2, 10, device=dev), torch.zeros(2, 72, device=dev), ct * 1.1
    res = fitter.fit(zeros_b, zeros_p, c0, kp)
    hist = res['loss_history']
    assert hist.shape == (31, 2) and hist.is_cuda and bool(torch.isfinite(hist).all())
    _, j0, _ = smpl(zeros_b, zeros_p, root_align=root_align)
    first = reprojection_loss(j0, c0, kp, camera=camera)
    assert torch.equal(hist[0], first)
    fall = (hist[0] / hist[-1]).cpu().tolist()
    print(f'fit {camera}: loss {hist[0].cpu().tolist()} -> {hist[-1].cpu().tolist()}, fall {fall} (float64 CPU loop: {cpu_fall})')
    assert all(f >= c / 3 for f, c in zip(fall, cpu_fall))


# ------------------------------------------------------------------------------------------------ refine_outputs
PAD = [20., 20., 0., 0., 600., 640.]                             # a 600 x 640 frame padded to 640 x 640


def stand_in(dev, kind):
    """What refine_outputs reads of a ROMP / BEV object -- smpl_parser (the real parser classes on the synthetic body
    models), settings.root_align, tdevice -- without building a network."""
    from romp_amd.bev import SMPLA_parser
    from romp_amd.post_parser import SMPL_parser
    parser = SMPL_parser(model_for(10)) if kind == 'romp' else SMPLA_parser(model_for(11), model_for(10))
    return types.SimpleNamespace(smpl_parser=parser.to(dev), settings=types.SimpleNamespace(root_align=False), tdevice=dev)


def synthetic_outputs(dev, model, kind, N=3):
    from romp_amd import lib as L
    from romp_amd.post_parser import body_mesh_projection2image
    g = torch.Generator().manual_seed(15)
    thetas = (0.3 * torch.randn(N, 72, generator=g)).to(dev)
    if kind == 'romp':
        betas = torch.randn(N, 10, generator=g).to(dev)
        cam = torch.tensor([[0.9, 0.05, -0.03], [0.7, -0.1, 0.08], [0.5, 0.3, 0.2]], device=dev)
        out = model.smpl_parser({'smpl_betas': betas, 'smpl_thetas': thetas, 'cam': cam})
        out.update(body_mesh_projection2image(out['joints'], cam, input2org_offsets=PAD))
        return out
    betas = torch.randn(N, 11, generator=g)
    betas[:, 10] = torch.tensor([0.1, 0.9, 0.3])                 # the second person is an infant: the SMIL layer
    betas = betas.to(dev)
    trans = torch.tensor([[0.1, -0.2, 3.0], [-0.3, 0.1, 5.0], [0.4, 0.2, 4.0]], device=dev)
    verts, joints, _ = model.smpl_parser(betas, thetas)
    org = torch.empty(N, J, 3, device=dev)
    L.check(L.load().romp_bev_project_verts(L.ptr(joints.contiguous()), N, J, L.ptr(trans), (ctypes.c_float * 6)(*PAD), L.ptr(org),
                                            L.stream_ptr(dev)))
    pj = org[:, :, :2].contiguous()
    return {'smpl_betas': betas, 'smpl_thetas': thetas, 'cam': torch.zeros(N, 3, device=dev), 'cam_trans': trans, 'verts': verts,
            'joints': joints, 'pj2d': pj, 'pj2d_org': pj}


@pytest.mark.parametrize('kind', ['romp', 'bev'])
def test_refine_outputs(dev, kind):
    from oracle import body_kernels_ref as R
    from romp_amd.fitting import refine_outputs
    from romp_amd.post_parser import body_mesh_projection2image
    model = stand_in(dev, kind)
    out = synthetic_outputs(dev, model, kind)
    cam_key = 'cam' if kind == 'romp' else 'cam_trans'
    steps, lr = 10, 0.01
    # (a) its own projection as the keypoints: the loss before is float32 rounding and nothing moves further than Adam can
    same = refine_outputs(model, out, out['pj2d_org'], pad_info=PAD, steps=steps, lr=lr)
    torch.cuda.synchronize()
    # a coordinate goes through about six float32 operations at magnitudes <= 2 on its way to pixels and back: <= 16 ulp of 1
    floor = 2 * (16 * 2.0 ** -23) ** 2
    print(f'{kind}: loss on its own projection {same["fit_loss"].cpu().tolist()} (floor {floor:.2e})')
    assert same['fit_loss'].shape == (3, 2) and float(same['fit_loss'][:, 0].max()) <= floor
    for k in ('smpl_betas', 'smpl_thetas', cam_key):
        assert float((same[k] - out[k]).abs().max()) <= steps * lr, k
    # (b) keypoints shifted by 8 px: the loss falls, and the returned projection is the projection of the returned parameters
    shifted = out['pj2d_org'] + 8.
    conf = torch.ones(3, J, device=dev)
    conf[:, 60:] = 0.5
    res = refine_outputs(model, {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}, shifted.cpu().numpy(),
                         conf=conf, pad_info=PAD, steps=steps, lr=lr)
    torch.cuda.synchronize()
    loss = res['fit_loss'].cpu()
    print(f'{kind}: loss with the keypoints shifted by 8 px {loss.tolist()}')
    assert bool((loss[:, 1] < loss[:, 0]).all()) and float(loss[:, 0].min()) > 1e-4        # 8 px of 640: (2 * 8 / 640)^2 * 2 = 1.25e-3
    for k in ('smpl_betas', 'smpl_thetas', cam_key):
        assert float((res[k] - out[k]).abs().max()) > 0, k
    if kind == 'romp':
        verts, joints, _ = model.smpl_parser.smpl_model(res['smpl_betas'], res['smpl_thetas'])
        assert torch.equal(verts, res['verts']) and torch.equal(joints, res['joints'])
        proj = body_mesh_projection2image(res['joints'], res['cam'], input2org_offsets=PAD)
        assert torch.equal(proj['pj2d_org'], res['pj2d_org']) and torch.equal(proj['pj2d'], res['pj2d'])
    else:
        verts, joints, _ = model.smpl_parser(res['smpl_betas'], res['smpl_thetas'])
        assert torch.equal(verts, res['verts']) and torch.equal(joints, res['joints'])
        assert float(res['smpl_betas'][1, 10]) == float(out['smpl_betas'][1, 10])      # the infant's age column is not fitted
        want = R.bev_project_verts(res['joints'].cpu().numpy(), res['cam_trans'].cpu().numpy(), PAD)[:, :, :2]
        assert res['pj2d'] is res['pj2d_org'] and np.abs(res['pj2d_org'].cpu().numpy() - want).max() <= 640 * 8 * 2.0 ** -23
        assert same['cam'] is out['cam']                             # BEV's normalised cam is not fitted
