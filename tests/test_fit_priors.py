"""SMPLify's pose priors and 3-D joint targets for the device fitter, CPU part (include/romp_hip_fit_priors.h,
csrc/fit_priors.hip, romp_amd/fitting.py): the exported symbols, their argument checks (they return before any HIP call),
`PosePrior`, and the torch restatements that tests/test_gpu_fit_priors.py measures the device against:
  `gmm_prior_torch`   MaxMixturePrior.merged_log_likelihood (prior_loss.py:232-247) on columns 3..3+D-1 of a 72-column pose;
  `angle_prior_torch` angle_prior (prior_loss.py:106-111), its indices moved to the 72-column pose;
  `joints3d_torch`    the loss of romp_fit_joints3d: calc_mpjpe's mask and align_by_parts (keypoints_loss.py:64-82), the squared
                      distance, confidences, robustifier and normaliser of the 2-D term;
  `fit_prior_loop_torch`  the loop of KeypointFitter with every term, built from these, `smpl_torch` and torch.optim.Adam.
All are pinned here in float64 by cases computed by hand."""
import ctypes
import math
import os
import pickle
import re

import numpy as np
import pytest
import torch

from test_fit import prior_weights, reproject_torch
from test_smpl_grad import smpl_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLE_COLUMNS, ANGLE_SIGNS = [55, 58, 12, 15], [1., -1., -1., -1.]       # prior_loss.py:111, plus the three global columns


# ------------------------------------------------------------------------------------------------ the restatements
def gmm_q_torch(poses, means, precisions, offsets, dtype=torch.float64):
    """q[n, m] = 0.5 d^T P_m d + offsets[m] with d = poses[n, 3:3+D] - means[m]: prior_loss.py:233-240, where offsets is
    -log(nll_weights).  poses (N,72), means (M,D), precisions (M,D,D), offsets (M) -> (N,M)."""
    means, precisions, offsets = means.to(dtype), precisions.to(dtype), offsets.to(dtype)
    D = means.shape[1]
    d = poses.to(dtype)[:, None, 3:3 + D] - means[None]                                  # :234
    pd = torch.einsum('mij,bmj->bmi', precisions, d)                                     # :236
    return 0.5 * (pd * d).sum(-1) + offsets[None]                                        # :238, :240


def gmm_prior_torch(poses, means, precisions, offsets, dtype=torch.float64):
    """-> (loss (N,), best (N,)): the minimum over the components (prior_loss.py:246) and the lowest index that attains it."""
    q = gmm_q_torch(poses, means, precisions, offsets, dtype)
    best = (q.detach() == q.detach().min(1, keepdim=True).values).to(torch.uint8).argmax(1)   # the first maximal value
    return q.gather(1, best[:, None])[:, 0], best


def gmm_margin(q):
    """How far each person's best q is ahead of the runner-up, over max(1, |q_best|).  One component: infinity."""
    if q.shape[1] < 2:
        return torch.full((q.shape[0],), float('inf'), dtype=torch.float64)
    two = torch.sort(q.detach().double(), 1).values[:, :2]
    return (two[:, 1] - two[:, 0]) / two[:, 0].abs().clamp(min=1.)


def angle_prior_torch(poses, dtype=torch.float64):
    """sum exp(s theta)^2 over left elbow, right elbow, left knee, right knee (prior_loss.py:111).  poses (N,72) -> (N,)."""
    p = poses.to(dtype)
    return (torch.exp(p[:, ANGLE_COLUMNS] * torch.tensor(ANGLE_SIGNS, dtype=dtype)) ** 2).sum(-1)


def joints3d_torch(joints, targets, conf=None, inds=None, align=None, sigma=0., trans=None, dtype=torch.float64):
    """The loss of romp_fit_joints3d, formula by formula (include/romp_hip_fit_priors.h), differentiable in joints and trans.
    joints (N,J,3), targets (N,K,3), conf (N,K) or None, inds: K joint indices or None, align: indices into the K keypoints or
    None, trans (N,3) or None -> loss (N,)."""
    joints, T = joints.to(dtype), targets.to(dtype)
    K = T.shape[1]
    zero = torch.zeros((), dtype=dtype)
    P = joints[:, :K] if inds is None else joints[:, torch.as_tensor(inds, dtype=torch.long)]
    if trans is not None:
        P = P + trans.to(dtype)[:, None]
    w = torch.ones(T.shape[:2], dtype=dtype) if conf is None else conf.to(dtype)
    vis = (w > 0) & (T[:, :, 0] != -2.) & ~torch.isnan(T).any(-1)                        # keypoints_loss.py:71, and conf, and NaN
    T = torch.where(vis[:, :, None], T, zero)                                            # nothing of an invisible keypoint gets in
    if align is not None and len(align):
        A = torch.as_tensor(list(align), dtype=torch.long)
        vis = vis & vis[:, A].all(1, keepdim=True)             # unlike the reference: a hidden alignment keypoint switches the person off
        P = P - P[:, A].mean(1, keepdim=True)                                            # align_by_parts, :67-68
        T = T - T[:, A].mean(1, keepdim=True)
    r = torch.where(vis[:, :, None], P - T, zero)
    e = (r * r).sum(-1)
    s = float(np.float32(sigma))
    rho = e if s <= 0 else (s * s) * e / (s * s + e)
    term = torch.where(vis, w * w * rho, zero)
    return term.sum(1) / (vis.to(dtype).sum(1) + 1e-4)


def fit_prior_loop_torch(model, betas0, poses0, cam0, kp2d=None, conf=None, joints3d=None, conf3d=None, prior=None, steps=30, lr=0.02,
                         sigma=0., camera='weak', w_betas=1e-4, w_pose=1e-4, root_align=False, w_gmm=0., w_angle=0., w_3d=1.,
                         sigma_3d=0., align=None, dtype=torch.float64):
    """KeypointFitter.fit with every term on the CPU: smpl_torch -> reproject_torch + w_3d joints3d_torch + w_gmm gmm_prior_torch +
    w_angle angle_prior_torch -> autograd -> torch.optim.Adam, the L2 priors added to the gradients by hand as romp_fit_adam
    adds them.  prior: (means, precisions, offsets) or None.  3-D targets are camera-space points with the perspective camera
    (trans = cam).  -> dict(betas, poses, cam, loss_history, loss3d_history, prior_history, margin: the smallest gmm_margin met)."""
    b, p, c = (t.to(dtype).clone().requires_grad_(True) for t in (betas0, poses0, cam0))
    ref = poses0.to(dtype).clone()
    wb, wp = prior_weights(w_betas, b.shape[1]).to(dtype), prior_weights(w_pose, 72, free=3).to(dtype)
    opt = torch.optim.Adam([b, p, c], lr=lr)
    h2, h3, hp, margin = [], [], [], float('inf')
    for s in range(steps + 1):
        opt.zero_grad()
        _, joints = smpl_torch(model, b, p, root_align, dtype)
        zeros = torch.zeros(b.shape[0], dtype=dtype)
        l2 = reproject_torch(joints, c, kp2d, conf, None, sigma, camera, dtype) if kp2d is not None else zeros
        l3 = joints3d_torch(joints, joints3d, conf3d, None, align, sigma_3d, c if camera == 'perspective' else None, dtype) \
            if joints3d is not None else zeros
        gmm = zeros
        if prior is not None and w_gmm > 0:
            gmm, _ = gmm_prior_torch(p, prior[0], prior[1], prior[2], dtype)
            margin = min(margin, float(gmm_margin(gmm_q_torch(p, prior[0], prior[1], prior[2], torch.float64)).min()))
        ang = angle_prior_torch(p, dtype)
        h2.append(l2.detach().clone()), h3.append(l3.detach().clone()), hp.append(torch.stack([gmm.detach(), ang.detach()], 1))
        if s == steps:
            break
        total = (l2 + w_3d * l3 + w_gmm * gmm + w_angle * ang).sum()
        if total.requires_grad:
            total.backward()
        for t in (b, p, c):
            t.grad = torch.zeros_like(t) if t.grad is None else t.grad
        b.grad += 2 * wb[None] * b.detach()
        p.grad += 2 * wp[None] * (p.detach() - ref)
        opt.step()
    return {'betas': b.detach(), 'poses': p.detach(), 'cam': c.detach(), 'loss_history': torch.stack(h2), 'loss3d_history': torch.stack(h3),
            'prior_history': torch.stack(hp), 'margin': margin}


def mixture(M, D, seed, spread=1.0):
    """A seeded mixture as the device reads it: means (M,D) = spread * randn, precisions A A^T / D + I (condition number <= 100,
    asserted), offsets in (0, 2): float32 tensors."""
    g = torch.Generator().manual_seed(seed)
    means = spread * torch.randn(M, D, generator=g)
    A = torch.randn(M, D, D, generator=g)
    prec = A @ A.transpose(1, 2) / D + torch.eye(D)
    prec = 0.5 * (prec + prec.transpose(1, 2))
    assert float(torch.linalg.cond(prec.double()).max()) <= 100
    return means, prec.contiguous(), 2 * torch.rand(M, generator=g)


# ------------------------------------------------------------------------------------------------ pinned by hand
def test_one_component_with_identity_precision_is_half_the_squared_distance_plus_the_offset():
    poses = torch.zeros(2, 72, dtype=torch.float64)
    poses[0, 3:6] = torch.tensor([1., 2., -2.])
    poses[1, 3:6] = torch.tensor([0.5, 0., 0.])
    poses[:, :3] = 7.                                            # the global orientation is not the prior's business
    poses[:, 6:] = 9.                                            # nor the columns past D
    means = torch.tensor([[0., 1., 0.]], dtype=torch.float64)    # d = (1, 1, -2) and (0.5, -1, 0)
    loss, best = gmm_prior_torch(poses, means, torch.eye(3, dtype=torch.float64)[None], torch.tensor([0.25], dtype=torch.float64))
    assert loss.tolist() == [0.5 * 6 + 0.25, 0.5 * 1.25 + 0.25] and best.tolist() == [0, 0]


def test_the_minimum_takes_the_lowest_index_at_a_tie_and_a_full_precision():
    poses = torch.zeros(1, 72, dtype=torch.float64)
    poses[0, 3:5] = torch.tensor([1., 2.])
    P = torch.tensor([[2., 1.], [1., 3.]], dtype=torch.float64)  # d^T P d = 2 + 2 * 2 + 12 = 18 at d = (1, 2)
    means = torch.zeros(3, 2, dtype=torch.float64)
    means[0] = torch.tensor([1., 2.])                            # d = 0: q = offset
    loss, best = gmm_prior_torch(poses, means, torch.stack([P, P, P]), torch.tensor([9.5, 0.5, 0.5], dtype=torch.float64))
    assert loss.tolist() == [9.5] and best.tolist() == [0]       # 9.5 = 9 + 0.5 = 9 + 0.5: three equal, the first wins
    loss, best = gmm_prior_torch(poses, means, torch.stack([P, P, P]), torch.tensor([10., 0.5, 0.5], dtype=torch.float64))
    assert loss.tolist() == [9.5] and best.tolist() == [1]


def test_one_angle_is_exp_of_twice_the_signed_angle():
    for col, sign in zip(ANGLE_COLUMNS, ANGLE_SIGNS):
        poses = torch.zeros(1, 72, dtype=torch.float64)
        poses[0, col] = 0.75
        want = math.exp(2 * sign * 0.75) + 3.0                   # the other three are exp(0)
        assert abs(float(angle_prior_torch(poses)) - want) <= 1e-15 * want
    poses = torch.zeros(1, 72, dtype=torch.float64)
    poses[0, 3:] = 100.                                          # everything else is ignored
    poses[0, ANGLE_COLUMNS] = 0.
    assert float(angle_prior_torch(poses)) == 4.0


def test_angle_columns_are_the_references_indices_plus_three():
    """angle_prior reads pose[:, [55-3, 58-3, 12-3, 15-3]] of the 69-column body pose (prior_loss.py:111)."""
    g = torch.Generator().manual_seed(1)
    poses = torch.randn(3, 72, generator=g, dtype=torch.float64)
    body = poses[:, 3:]
    want = (torch.exp(body[:, [55 - 3, 58 - 3, 12 - 3, 15 - 3]] * torch.tensor([1., -1., -1, -1.], dtype=torch.float64)) ** 2).sum(dim=-1)
    assert torch.equal(angle_prior_torch(poses), want)


def test_one_3d_keypoint_with_confidence_and_geman_mcclure():
    """conf^2 sigma^2 e / (sigma^2 + e) / (1 + 1e-4) with r = (0.5, -0.25, 3) + (0.5, 0.25, -1) - (0.5, 0.5, 1) = (0.5, -0.5, 1)."""
    joints = torch.tensor([[[0.5, -0.25, 3.0]]], dtype=torch.float64)
    trans = torch.tensor([[0.5, 0.25, -1.0]], dtype=torch.float64)
    target = torch.tensor([[[0.5, 0.5, 1.0]]], dtype=torch.float64)
    e = 0.25 + 0.25 + 1.0
    got = joints3d_torch(joints, target, torch.tensor([[0.5]]), None, None, 0.5, trans)
    assert abs(float(got) - 0.25 * (0.25 * e / (0.25 + e)) / (1 + 1e-4)) <= 1e-15
    got = joints3d_torch(joints, target, None, None, None, 0., trans)
    assert abs(float(got) - e / (1 + 1e-4)) <= 1e-15
    for hidden in (dict(conf=torch.tensor([[0.]])), dict(targets=torch.tensor([[[-2., 0.5, 1.]]], dtype=torch.float64)),
                   dict(targets=torch.tensor([[[0.5, float('nan'), 1.]]], dtype=torch.float64))):
        args = dict(dict(targets=target, conf=None), **hidden)
        assert float(joints3d_torch(joints, args['targets'], args['conf'], None, None, 0., trans)) == 0.


def test_alignment_on_two_keypoints():
    """Three keypoints, aligned on the first two.  By hand: predictions (0,0,0), (2,0,0), (1,3,0) have the alignment mean
    (1,0,0) -> (-1,0,0), (1,0,0), (0,3,0); targets (1,1,1), (1,1,3), (1,2,2) have (1,1,2) -> (0,0,-1), (0,0,1), (0,1,0);
    residuals (-1,0,1), (1,0,-1), (0,2,0): e = 2, 2, 4, loss = 8 / (3 + 1e-4).  A translation changes nothing: the joint
    gradients sum to zero, and the aligned set's share of them is minus the gradient of the third keypoint."""
    joints = torch.tensor([[[0., 0., 0.], [2., 0., 0.], [1., 3., 0.]]], dtype=torch.float64, requires_grad=True)
    targets = torch.tensor([[[1., 1., 1.], [1., 1., 3.], [1., 2., 2.]]], dtype=torch.float64)
    trans = torch.tensor([[5., -3., 2.]], dtype=torch.float64, requires_grad=True)
    loss = joints3d_torch(joints, targets, None, None, [0, 1], 0., trans)
    assert abs(float(loss.detach()) - 8 / (3 + 1e-4)) <= 1e-15
    loss.sum().backward()
    n = 3 + 1e-4
    g = torch.tensor([[-2., 0., 2.], [2., 0., -2.], [0., 4., 0.]], dtype=torch.float64) / n       # 2 r_k / n
    want = g.clone()
    want[:2] -= g.sum(0) / 2                                     # g_j - [j in A] (1 / |A|) sum_k g_k
    assert float((joints.grad[0] - want).abs().max()) <= 1e-15
    assert float((joints.grad[0, :2].sum(0) - (g[:2].sum(0) - g.sum(0))).abs().max()) <= 1e-15   # the aligned set's share
    assert float(joints.grad[0].sum(0).abs().max()) <= 1e-15 and float(trans.grad.abs().max()) == 0.
    hidden = targets.clone()
    hidden[0, 1, 0] = -2.                                        # an alignment keypoint without a target: the person is off
    assert float(joints3d_torch(joints.detach(), hidden, None, None, [0, 1], 0., trans.detach())) == 0.
    hidden = targets.clone()
    hidden[0, 2, 0] = -2.                                        # another keypoint: only that one drops out
    assert abs(float(joints3d_torch(joints.detach(), hidden, None, None, [0, 1], 0., trans.detach())) - 4 / (2 + 1e-4)) <= 1e-15


def test_permuted_joint_inds_pick_the_joints():
    g = torch.Generator().manual_seed(2)
    joints, targets = torch.randn(2, 10, 3, generator=g, dtype=torch.float64), torch.randn(2, 3, 3, generator=g, dtype=torch.float64)
    got = joints3d_torch(joints, targets, None, [7, 2, 4], None, 0., None)
    want = ((joints[:, [7, 2, 4]] - targets) ** 2).sum(-1).sum(-1) / (3 + 1e-4)
    assert float((got - want).abs().max()) <= 1e-15


# ------------------------------------------------------------------------------------------------ PosePrior
def synthetic_gmm(M=8, D=69, seed=3):
    """A seeded mixture in the layout of SMPLify's gmm_08.pkl: float64 means (M,D), covars (M,D,D), weights (M,)."""
    rng = np.random.RandomState(seed)
    A = rng.randn(M, D, D)
    covars = 0.05 * (A @ A.transpose(0, 2, 1) / D + np.eye(D)) * (1 + 0.1 * rng.rand(M))[:, None, None]
    weights = rng.rand(M) + 0.1
    return {'means': 0.3 * rng.randn(M, D), 'covars': covars, 'weights': weights / weights.sum()}


def test_pose_prior_is_the_references_construction():
    """prior_loss.py:202-214 transcribed into numpy float64; PosePrior stores the same numbers rounded to float32 (its
    precisions are made symmetric first, which moves a float64 inverse by roundings of float64 only)."""
    from romp_amd.fitting import PosePrior
    gmm = synthetic_gmm()
    precisions = np.stack([np.linalg.inv(cov) for cov in gmm['covars']])                             # :202-203
    sqrdets = np.array([(np.sqrt(np.linalg.det(c))) for c in gmm['covars']])                          # :208-209
    const = (2 * np.pi) ** (69 / 2.)                                                                  # :210
    nll_weights = np.asarray(gmm['weights'] / (const * (sqrdets / sqrdets.min())))                    # :212
    prior = PosePrior(gmm['means'], gmm['covars'], gmm['weights'])
    assert prior.means.dtype == prior.precisions.dtype == prior.offsets.dtype == torch.float32
    assert prior.means.shape == (8, 69) and prior.precisions.shape == (8, 69, 69) and prior.offsets.shape == (8,)
    assert prior.precisions.is_contiguous() and torch.equal(prior.precisions, prior.precisions.transpose(1, 2))
    ulp = 2.0 ** -23
    assert np.array_equal(prior.means.numpy(), gmm['means'].astype(np.float32))
    assert np.abs(prior.precisions.numpy() - precisions).max() <= ulp * np.abs(precisions).max()
    assert np.abs(prior.offsets.numpy() + np.log(nll_weights)).max() <= ulp * np.abs(np.log(nll_weights)).max()
    # and the likelihood built from them is merged_log_likelihood's (:234-247)
    poses = torch.from_numpy(0.3 * np.random.RandomState(4).randn(5, 72))
    d = poses[:, None, 3:] - torch.from_numpy(gmm['means'])[None]
    want = (0.5 * (torch.einsum('mij,bmj->bmi', torch.from_numpy(precisions), d) * d).sum(-1) - torch.log(torch.from_numpy(nll_weights))[None]).min(1).values
    got, _ = gmm_prior_torch(poses, prior.means, prior.precisions, prior.offsets)
    assert float((got - want).abs().max()) <= 64 * ulp * float(want.abs().max())       # float32 storage of 69 x 69 terms


def test_pose_prior_from_file_and_sliced(tmp_path):
    from romp_amd.fitting import PosePrior
    gmm = synthetic_gmm(M=3, seed=5)
    want = PosePrior(gmm['means'], gmm['covars'], gmm['weights'])
    with open(str(tmp_path / 'gmm_03.pkl'), 'wb') as f:
        pickle.dump(gmm, f, protocol=2)                          # the protocol of SMPLify's own file
    np.savez(str(tmp_path / 'gmm_03.npz'), **gmm)
    for name in ('gmm_03.pkl', 'gmm_03.npz'):
        got = PosePrior.from_file(str(tmp_path / name))
        assert all(torch.equal(getattr(got, k), getattr(want, k)) for k in ('means', 'precisions', 'offsets')), name
    cut = want.sliced(63)
    assert torch.equal(cut.means, want.means[:, :63]) and torch.equal(cut.precisions, want.precisions[:, :63, :63])
    assert torch.equal(cut.offsets, want.offsets) and cut.precisions.is_contiguous() and cut.means.is_contiguous()
    with pytest.raises(ValueError):
        PosePrior(gmm['means'], gmm['covars'][:, :5], gmm['weights'])


# ------------------------------------------------------------------------------------------------ the C seam
def test_fit_prior_symbols_exported():
    from romp_amd import lib
    header = open(os.path.join(ROOT, 'include', 'romp_hip_fit_priors.h')).read()
    declared = re.findall(r'^\s*(?:int|void)\s+(\w+)\s*\(', header, re.M)
    assert declared == lib.FIT_PRIOR_EXPORTS == ['romp_fit_pose_prior', 'romp_fit_joints3d']
    others = (lib.EXPORTS + lib.VIEW_EXPORTS + lib.MAP_EXPORTS + lib.TEXTURE_EXPORTS + lib.EVAL_EXPORTS + lib.RH_EXPORTS +
              lib.CANVAS_EXPORTS + lib.SMPL_GRAD_EXPORTS + lib.FIT_EXPORTS)
    assert not set(declared) & set(others)
    assert lib.FIT_EXPORTS == ['romp_fit_reproject', 'romp_fit_adam']
    h = lib.load()
    assert h.romp_abi_version() == 7 == lib.ABI_VERSION
    assert len(h.romp_fit_pose_prior.argtypes) == 16 and len(h.romp_fit_joints3d.argtypes) == 19
    for n in declared:
        assert getattr(h, n).restype is ctypes.c_int, n
    assert 'symmetric' in header.lower() and 'ROMP_FIT_MAX_GAUSSIANS 16' in header


def test_the_header_compiles_as_c():
    import subprocess
    import tempfile
    prog = '#include "romp_hip_fit_priors.h"\nint main(void) { return ROMP_FIT_MAX_GAUSSIANS == 16 && ROMP_FIT_MAX_POSE_DIM == 69 ? 0 : 1; }\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, 't.c')
        open(c, 'w').write(prog)
        subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), c, '-o', os.path.join(td, 't')])
        subprocess.check_call([os.path.join(td, 't')])


def _host_pointer():
    buf = (ctypes.c_float * 1024)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_pose_prior_rejects_bad_arguments_before_any_device_call():
    from romp_amd import lib
    h = lib.load()
    keep, p = _host_pointer()                                    # never dereferenced: every call below fails its checks first

    def call(poses=p, N=1, means=p, prec=p, offs=p, M=8, D=69, loss=p, best=None, gp=p, acc=0, hist=None, row=0):
        return h.romp_fit_pose_prior(poses, N, means, prec, offs, M, D, 1., 1., loss, best, gp, acc, hist, row, None)

    for bad in (dict(poses=None), dict(loss=None), dict(gp=None), dict(N=-1), dict(D=0), dict(D=70), dict(M=-1), dict(M=17),
                dict(prec=None), dict(offs=None), dict(row=-1), dict(M=0, D=0), dict(means=None, D=70)):
        assert call(**bad) == -1 and b'romp_fit_pose_prior' in h.romp_last_error(), bad
    assert call(N=0) == 0                                        # nothing to do, nothing launched
    assert call(N=0, M=0, means=None, prec=None, offs=None) == 0 and call(N=0, means=None, prec=None, offs=None) == 0
    assert call(N=0, D=1, M=16, acc=1) == 0
    assert call(N=0, D=70) == -1                                 # the range checks do not depend on N


def test_joints3d_rejects_bad_arguments_before_any_device_call():
    from romp_amd import lib
    h = lib.load()
    keep, p = _host_pointer()
    I = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def call(joints=p, N=1, J=4, trans=None, targets=p, conf=None, K=2, inds=None, align=None, n_align=0, loss=p, gj=p, gt=None,
             acc=0, hist=None, row=0):
        return h.romp_fit_joints3d(joints, N, J, trans, targets, conf, K, inds, align, n_align, 0., 1., loss, gj, gt, acc, hist, row, None)

    for bad in (dict(joints=None), dict(targets=None), dict(loss=None), dict(gj=None), dict(gt=p), dict(trans=p), dict(N=-1),
                dict(K=0), dict(K=5), dict(J=257, K=1), dict(inds=I(0, 0)), dict(inds=I(0, 4)), dict(inds=I(-1, 2)),
                dict(align=I(0), n_align=-1), dict(align=I(0, 1, 1), n_align=3), dict(n_align=1), dict(align=I(0, 0), n_align=2),
                dict(align=I(2), n_align=1), dict(align=I(-1), n_align=1), dict(row=-1)):
        assert call(**bad) == -1 and b'romp_fit_joints3d' in h.romp_last_error(), bad
    assert call(N=0) == 0                                        # nothing to do, nothing launched
    assert call(N=0, trans=p, gt=p, inds=I(3, 1), align=I(1, 0), n_align=2, acc=1) == 0
    assert call(N=0, inds=I(3, 3)) == -1 and call(N=0, align=I(1, 1), n_align=2) == -1   # the index checks do not depend on N


def test_the_new_terms_need_the_device():
    """No CPU fallback, as for the reprojection loss."""
    from romp_amd.fitting import PosePrior, joints3d_loss, pose_prior_loss
    from romp_amd.lib import RompHipError
    gmm = synthetic_gmm(M=2, seed=6)
    with pytest.raises(RompHipError):
        pose_prior_loss(torch.zeros(1, 72), PosePrior(gmm['means'], gmm['covars'], gmm['weights']))
    with pytest.raises(RompHipError):
        joints3d_loss(torch.zeros(1, 71, 3), torch.zeros(1, 24, 3))


def test_fitter_arguments():
    from romp_amd.fitting import KeypointFitter
    from romp_amd.smpl import SMPL
    from romp_amd.synthetic import make_smpl_model
    f = KeypointFitter(SMPL(make_smpl_model()))
    assert (f.pose_prior, f.w_gmm, f.w_angle, f.w_3d, f.sigma_3d, f.align_inds) == (None, 0., 0., 1., 0., None)
    with pytest.raises(ValueError):
        KeypointFitter(SMPL(make_smpl_model()), w_gmm=-1.)
