"""Fitting to 2-D keypoints, CPU part (include/romp_hip_fit.h, csrc/fit.hip, romp_amd/fitting.py): the exported symbols,
their argument checks (they return before any HIP call), and the torch restatements that tests/test_gpu_fit.py measures the
device against:  `reproject_torch`, the loss of romp_fit_reproject, pinned here in float64 to the oracle's two projections and
to the reference's visibility mask;  `adam_loop_torch`, torch.optim.Adam with the prior's gradient added by hand;
`fit_loop_torch`, the loop of KeypointFitter built from `smpl_torch`, `reproject_torch` and torch.optim.Adam."""
import ctypes
import os
import re

import numpy as np
import torch

from oracle import body_kernels_ref as R
from oracle import romp_oracle as O
from test_smpl_grad import smpl_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatements
def project_torch(X, cam, camera='weak', dtype=torch.float64, focal=443.4, half=256.):
    """The two cameras of romp_fit_reproject: X (N,K,3), cam (N,3) -> (N,K,2).  focal and half as the floats the C entry takes."""
    X, cam = X.to(dtype), cam.to(dtype)
    if camera == 'weak':
        return X[:, :, :2] * cam[:, None, 0:1] + cam[:, None, 1:]
    f, h = float(np.float32(focal)), float(np.float32(half))
    p = X + cam[:, None]
    return p[:, :, :2] / (p[:, :, 2:3] + 1e-6) * f / h


def reproject_torch(joints, cam, kp2d, conf=None, inds=None, sigma=0., camera='weak', dtype=torch.float64, focal=443.4, half=256.):
    """The loss of romp_fit_reproject, formula by formula (include/romp_hip_fit.h), differentiable in joints and cam.
    joints (N,J,3), cam (N,3), kp2d (N,K,2), conf (N,K) or None, inds: K joint indices or None -> loss (N,)."""
    joints, kp2d = joints.to(dtype), kp2d.to(dtype)
    K = kp2d.shape[1]
    X = joints[:, :K] if inds is None else joints[:, torch.as_tensor(inds, dtype=torch.long)]
    uv = project_torch(X, cam, camera, dtype, focal, half)
    w = torch.ones(kp2d.shape[:2], dtype=dtype) if conf is None else conf.to(dtype)
    vis = (w > 0) & (kp2d[:, :, 0] > -1.99) & (kp2d[:, :, 1] > -1.99)
    r = torch.where(vis[:, :, None], uv - kp2d, torch.zeros((), dtype=dtype))      # nothing of an invisible keypoint gets in
    e = (r * r).sum(-1)
    s = float(np.float32(sigma))
    rho = e if s <= 0 else (s * s) * e / (s * s + e)
    term = torch.where(vis, w * w * rho, torch.zeros((), dtype=dtype))
    return term.sum(1) / (vis.to(dtype).sum(1) + 1e-4)


def adam_loop_torch(params, grads_per_step, prior_refs, prior_ws, lr, dtype, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam over `params` (a list of tensors) with supplied data gradients grads_per_step[step][i] and the prior
    gradient 2 w[c] (p - ref) added by hand (ref None = zeros, w None = no prior).  -> the parameters after the last step."""
    ps = [p.to(dtype).clone().requires_grad_(True) for p in params]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps)
    for grads in grads_per_step:
        for p, g, ref, w in zip(ps, grads, prior_refs, prior_ws):
            g = g.to(dtype).clone()
            if w is not None:
                g = g + 2 * w.to(dtype)[None] * (p.detach() - (0 if ref is None else ref.to(dtype)))
            p.grad = g
        opt.step()
    return [p.detach() for p in ps]


def prior_weights(w, cols, free=0):
    out = torch.full((cols,), float(w), dtype=torch.float32)
    out[:free] = 0
    return out


def fit_loop_torch(model, betas0, poses0, cam0, kp2d, conf=None, inds=None, steps=30, lr=0.02, sigma=0., camera='weak', w_betas=1e-4,
                   w_pose=1e-4, root_align=False, dtype=torch.float64):
    """KeypointFitter.fit on the CPU: smpl_torch -> reproject_torch -> autograd -> torch.optim.Adam, the L2 priors added to the
    gradients by hand as romp_fit_adam adds them.  -> dict(betas, poses, cam, loss_history (steps + 1, N))."""
    b, p, c = (t.to(dtype).clone().requires_grad_(True) for t in (betas0, poses0, cam0))
    ref = poses0.to(dtype).clone()
    wb, wp = prior_weights(w_betas, b.shape[1]).to(dtype), prior_weights(w_pose, 72, free=3).to(dtype)
    opt = torch.optim.Adam([b, p, c], lr=lr)
    hist = []
    for s in range(steps + 1):
        opt.zero_grad()
        _, joints = smpl_torch(model, b, p, root_align, dtype)
        loss = reproject_torch(joints, c, kp2d, conf, inds, sigma, camera, dtype)
        hist.append(loss.detach().clone())
        if s == steps:
            break
        loss.sum().backward()
        b.grad += 2 * wb[None] * b.detach()
        p.grad += 2 * wp[None] * (p.detach() - ref)
        opt.step()
    return {'betas': b.detach(), 'poses': p.detach(), 'cam': c.detach(), 'loss_history': torch.stack(hist)}


def grid(shape, g, step, lim):
    """Seeded multiples of `step` in (-lim, lim): products and sums of a few of them are exact in float32, so an oracle that
    rounds to float32 on the way loses nothing."""
    return (torch.randint(-int(lim / step), int(lim / step) + 1, shape, generator=g).double() * step)


# ------------------------------------------------------------------------------------------------ pinned to the oracle
def test_weak_mode_equals_the_oracles_orthographic_projection():
    g = torch.Generator().manual_seed(1)
    N, J, K = 3, 71, 24
    joints, cam, kp = grid((N, J, 3), g, 1 / 256, 2), grid((N, 3), g, 1 / 16, 2), grid((N, K, 2), g, 1 / 256, 1)
    pj = O.batch_orth_proj(joints.numpy().astype(np.float32), cam.numpy())[:, :K].astype(np.float64)
    want = ((pj - kp.numpy()) ** 2).sum(-1).sum(-1) / (K + 1e-4)
    got = reproject_torch(joints, cam, kp, None, None, 0., 'weak', torch.float64).numpy()
    print('weak: max |delta|', np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    inds = torch.randperm(J, generator=g)[:K]
    pj = O.batch_orth_proj(joints.numpy().astype(np.float32), cam.numpy())[:, inds.numpy()].astype(np.float64)
    want = ((pj - kp.numpy()) ** 2).sum(-1).sum(-1) / (K + 1e-4)
    got = reproject_torch(joints, cam, kp, None, inds.tolist(), 0., 'weak', torch.float64).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_perspective_mode_equals_the_oracles_bev_projection():
    g = torch.Generator().manual_seed(2)
    N, J, K = 3, 71, 71
    joints = (torch.randn(N, J, 3, generator=g) * 0.4).float().double()             # float32 numbers: the oracle takes its inputs as float32
    trans = torch.cat([torch.randn(N, 2, generator=g) * 0.3, 0.5 + 7.5 * torch.rand(N, 1, generator=g)], 1).float().double()
    kp = (torch.randn(N, K, 2, generator=g) * 0.5).float().double()
    unit = [0., 0., 0., 0., 2., 2.]                               # to_org with max(h, w) = 2 and no offset: k + 1
    pj = R.bev_project_verts(joints.numpy(), trans.numpy(), unit, dtype=np.float64)[:, :, :2] - 1.0
    want = ((pj - kp.numpy()) ** 2).sum(-1).sum(-1) / (K + 1e-4)
    got = reproject_torch(joints, trans, kp, None, None, 0., 'perspective', torch.float64, focal=443.4, half=256.).numpy()
    print('perspective: max |delta|', np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_a_target_of_minus_two_drops_out_like_the_references_vis_mask():
    g = torch.Generator().manual_seed(3)
    N, J, K = 2, 71, 24
    joints, cam, kp = grid((N, J, 3), g, 1 / 256, 2), grid((N, 3), g, 1 / 16, 2), grid((N, K, 2), g, 1 / 256, 1)
    kp[0, 3] = -2.                                               # both coordinates, the data loader's mark
    kp[0, 7, 1] = -2.                                            # one coordinate is enough (keypoints_loss.py:24)
    kp[1, :] = -2.                                               # a person without any keypoint
    kp[0, 9] = -1.98                                             # just inside
    real = kp.numpy()
    vis_mask = ((real > -1.99).sum(-1) == real.shape[-1]).astype(np.float64)          # keypoints_loss.py:24
    pj = O.batch_orth_proj(joints.numpy().astype(np.float32), cam.numpy())[:, :K].astype(np.float64)
    want = (((pj - real) ** 2).sum(-1) * vis_mask).sum(-1) / (vis_mask.sum(-1) + 1e-4)  # :38 with the squared distance
    got = reproject_torch(joints, cam, kp, None, None, 0., 'weak', torch.float64).numpy()
    assert vis_mask[0].sum() == K - 2 and vis_mask[1].sum() == 0
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max() and got[1] == 0
    nan = kp.clone()
    nan[0, 3] = float('nan')
    conf = torch.ones(N, K, dtype=torch.float64)
    conf[0, 3] = 0
    again = reproject_torch(joints, cam, nan, conf, None, 0., 'weak', torch.float64).numpy()
    assert np.array_equal(again, got)                            # conf 0 hides it the same way, NaN and all


def test_robust_term_and_confidence():
    """One keypoint by hand: conf^2 sigma^2 e / (sigma^2 + e) / (1 + 1e-4)."""
    joints = torch.tensor([[[0.5, -0.25, 3.0]]], dtype=torch.float64)
    cam = torch.tensor([[2.0, 0.125, 0.25]], dtype=torch.float64)
    kp = torch.tensor([[[1.0, 0.0]]], dtype=torch.float64)        # u, v = 1.125, -0.25 -> e = 0.125^2 + 0.25^2
    e = 0.125 ** 2 + 0.25 ** 2
    got = reproject_torch(joints, cam, kp, torch.tensor([[0.5]]), None, 0.5, 'weak', torch.float64)
    assert abs(float(got) - 0.25 * (0.25 * e / (0.25 + e)) / (1 + 1e-4)) <= 1e-15


# ------------------------------------------------------------------------------------------------ the C seam
def test_fit_symbols_exported():
    from romp_amd import lib
    header = open(os.path.join(ROOT, 'include', 'romp_hip_fit.h')).read()
    declared = re.findall(r'^\s*(?:int|void)\s+(\w+)\s*\(', header, re.M)
    assert declared == lib.FIT_EXPORTS == ['romp_fit_reproject', 'romp_fit_adam']
    others = (lib.EXPORTS + lib.VIEW_EXPORTS + lib.MAP_EXPORTS + lib.TEXTURE_EXPORTS + lib.EVAL_EXPORTS + lib.RH_EXPORTS +
              lib.CANVAS_EXPORTS + lib.SMPL_GRAD_EXPORTS)
    assert not set(declared) & set(others)
    h = lib.load()
    assert h.romp_abi_version() == 7 == lib.ABI_VERSION
    assert len(h.romp_fit_reproject.argtypes) == 18 and len(h.romp_fit_adam.argtypes) == 8
    for n in declared:
        assert getattr(h, n).restype is ctypes.c_int, n
    assert ctypes.sizeof(lib.FitSegment) == 56                   # six pointers and two int32


def test_fit_segment_layout_matches_the_header():
    """The header compiles as C, and the ctypes mirror has the C struct's size and offsets."""
    import subprocess
    import tempfile
    from romp_amd.lib import FitSegment
    prog = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "romp_hip_fit.h"
    int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(romp_fit_segment), offsetof(romp_fit_segment, grad),
        offsetof(romp_fit_segment, v), offsetof(romp_fit_segment, prior_ref), offsetof(romp_fit_segment, prior_w),
        offsetof(romp_fit_segment, rows), offsetof(romp_fit_segment, cols)); return 0; }
    '''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, 't.c')
        open(c, 'w').write(prog)
        exe = os.path.join(td, 't')
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    assert vals == [ctypes.sizeof(FitSegment), FitSegment.grad.offset, FitSegment.v.offset, FitSegment.prior_ref.offset,
                    FitSegment.prior_w.offset, FitSegment.rows.offset, FitSegment.cols.offset]


def _host_pointer():
    buf = (ctypes.c_float * 1024)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_reproject_rejects_bad_arguments_before_any_device_call():
    from romp_amd import lib
    h = lib.load()
    keep, p = _host_pointer()                                    # never dereferenced: every call below fails its checks first
    I = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def call(joints=p, N=1, J=4, cam=p, targets=p, conf=None, K=2, inds=None, mode=0, loss=p, gj=p, gc=p, hist=None, row=0):
        return h.romp_fit_reproject(joints, N, J, cam, targets, conf, K, inds, mode, 443.4, 256., 0., loss, gj, gc, hist, row, None)

    for bad in (dict(joints=None), dict(cam=None), dict(targets=None), dict(loss=None), dict(gj=None), dict(gc=None),
                dict(N=-1), dict(K=0), dict(K=5), dict(J=257, K=1), dict(inds=I(0, 0)), dict(inds=I(0, 4)), dict(inds=I(-1, 2)),
                dict(mode=2), dict(row=-1)):
        assert call(**bad) == -1 and b'romp_fit_reproject' in h.romp_last_error(), bad
    assert call(N=0) == 0                                        # nothing to do, nothing launched
    assert call(N=0, inds=I(3, 1)) == 0
    assert call(N=0, inds=I(3, 3)) == -1                         # the index check does not depend on N


def test_adam_rejects_bad_arguments_before_any_device_call():
    from romp_amd import lib
    h = lib.load()
    keep, p = _host_pointer()
    a = p.value
    seg = lambda **k: lib.FitSegment(**dict(dict(param=a, grad=a, m=a, v=a, prior_ref=None, prior_w=None, rows=1, cols=3), **k))
    arr = lambda *s: (lib.FitSegment * len(s))(*s)
    call = lambda segs, n, step=1: h.romp_fit_adam(segs, n, 0.02, 0.9, 0.999, 1e-8, step, None)
    assert call(None, 1) == -1 and b'romp_fit_adam' in h.romp_last_error()
    assert call(arr(seg()), 0) == -1
    assert call(arr(*[seg()] * 9), 9) == -1
    assert call(arr(seg()), 1, step=0) == -1 and b'step' in h.romp_last_error()
    for bad in (dict(param=None), dict(grad=None), dict(m=None), dict(v=None), dict(rows=-1), dict(cols=0)):
        assert call(arr(seg(), seg(**bad)), 2) == -1 and b'segment 1' in h.romp_last_error(), bad
    assert call(arr(seg(rows=0), seg(rows=0, cols=72)), 2) == 0  # no element: nothing launched


def test_fitting_module_stands_without_the_oracle():
    src = open(os.path.join(ROOT, 'romp_amd', 'fitting.py')).read()
    assert 'oracle' not in src
    import romp_amd.fitting as F
    assert {'reprojection_loss', 'KeypointFitter', 'refine_outputs'} <= set(dir(F))
    imports = re.findall(r'^\s*(?:from|import)\s+([\w.]+)', src, re.M)
    assert set(imports) <= {'ctypes', 'numpy', 'torch', '.', '.post_parser'}, imports


def test_fitter_needs_the_device():
    """No CPU fallback: a layer that was not moved to the device raises, as the layer itself does."""
    import pytest
    from romp_amd.fitting import KeypointFitter, reprojection_loss
    from romp_amd.lib import RompHipError
    from romp_amd.smpl import SMPL
    from romp_amd.synthetic import make_smpl_model
    with pytest.raises(RompHipError):
        KeypointFitter(SMPL(make_smpl_model()), steps=1).fit(torch.zeros(1, 10), torch.zeros(1, 72), torch.ones(1, 3), torch.zeros(1, 24, 2))
    with pytest.raises(RompHipError):
        reprojection_loss(torch.zeros(1, 71, 3), torch.ones(1, 3), torch.zeros(1, 24, 2))
