"""SMPLify's pose priors and 3-D joint targets on the GPU (run with -m gpu): romp_fit_pose_prior and romp_fit_joints3d
(csrc/fit_priors.hip) and romp_amd.fitting on top of them, against the float64 CPU restatements of tests/test_fit_priors.py.

Tolerance: the rule of tests/test_gpu_fit.py.  error = max |delta| / max |float64 reference| per tensor; every case also
evaluates the restatement in float32 on the CPU and requires  err_HIP <= 8 * max(err_CPU_f32, FLOOR),  FLOOR = 4 * 2^-24.
Every figure is printed before it is asserted (pytest -s).

Input conditions, asserted on the CPU in float64 before the device is touched: each person's best q is ahead of the runner-up
by at least 1e-3 * max(1, |q_best|), so that a float32 yardstick cannot pick another component; precisions are A A^T / D + I
with a condition number <= 100; |theta| <= pi.

fit_pose_prior_kernel gives a workgroup to each person (PERSONS_PER_WORKGROUP = 1), so N = 1, 2 are a lone workgroup and a
workgroup plus one; its eight waves take one mixture component each per round, so M = 1, 8, 16 are one wave, one full round
and two; a lane owns columns i and i + 64 of the D, so D = 1, 63, 64, 65, 69 are one lane, part of a wave, the last lane of
the first round, the first lane of the second round and the full body pose.  fit_joints3d_kernel gives a wave to each person,
four to a workgroup: N = 1, 3, 5 as in tests/test_gpu_fit.py."""
import itertools
import math

import pytest
import torch

from test_fit_priors import (ANGLE_COLUMNS, angle_prior_torch, fit_prior_loop_torch, gmm_margin, gmm_prior_torch, gmm_q_torch,
                             joints3d_torch, mixture)
from test_gpu_fit import FLOOR, J, PAD, fit_case, layer, stand_in, synthetic_outputs, within
from test_smpl_grad import smpl_torch

pytestmark = pytest.mark.gpu
PERSONS_PER_WORKGROUP = 1
PRIOR_N = sorted({1, PERSONS_PER_WORKGROUP + 1} | ({PERSONS_PER_WORKGROUP - 1} if PERSONS_PER_WORKGROUP >= 2 else set()))
MARGIN = 1e-3
W_GMM, W_ANGLE = 0.8, 0.37


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def nan_like(dev, *shape):
    return torch.full(shape, float('nan'), device=dev, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ the pose prior
def prior_case(N, M, D, seed):
    """-> poses (N,72) float32 with |theta| <= 3.14 < pi, and the mixture (means, precisions, offsets) or None for M = 0.  Person n
    sits 0.3 randn from the mean of component (3 n + 1) % M; the argmin margin is asserted."""
    g = torch.Generator().manual_seed(seed)
    poses = (0.8 * torch.randn(N, 72, generator=g)).clamp(-3.14, 3.14)
    if M == 0:
        return poses, None
    mix = mixture(M, D, seed + 1)
    for n in range(N):
        poses[n, 3:3 + D] = (mix[0][(3 * n + 1) % M] + 0.3 * torch.randn(D, generator=g)).clamp(-3.14, 3.14)
    assert float(poses.abs().max()) <= math.pi
    margin = gmm_margin(gmm_q_torch(poses, *mix))
    assert float(margin.min()) >= MARGIN, (N, M, D, seed, margin.tolist())
    return poses, mix


def cpu_prior(poses, mix, w_gmm, w_angle, dtype):
    p = poses.to(dtype).clone().requires_grad_(True)
    angle = angle_prior_torch(p, dtype)
    if mix is None:
        gmm, best = torch.zeros(p.shape[0], dtype=dtype), torch.full((p.shape[0],), -1)
    else:
        gmm, best = gmm_prior_torch(p, mix[0], mix[1], mix[2], dtype)
    (w_gmm * gmm + w_angle * angle).sum().backward()             # a row of the loss depends on its own person alone
    return torch.stack([gmm.detach(), angle.detach()], 1).double(), best, p.grad.double()


def hip_prior(dev, poses, mix, w_gmm, w_angle, accumulate=0, old=None, history_rows=0, row=0):
    """The C entry on buffers filled with NaN (best with -7), so that an element it does not write shows."""
    from romp_amd import fitting as F
    N = poses.shape[0]
    prior = None
    if mix is not None:
        prior = F.PosePrior.__new__(F.PosePrior)._set(mix[0], mix[1], mix[2], dev)
    loss, best = nan_like(dev, N, 2), torch.full((N,), -7, device=dev, dtype=torch.int32)
    gp = nan_like(dev, N, 72) if old is None else old.to(dev).clone()
    hist = nan_like(dev, history_rows, N, 2) if history_rows else None
    F._pose_prior(poses.to(dev).contiguous(), prior, w_gmm, w_angle, loss, best, gp, accumulate, hist, row)
    torch.cuda.synchronize()
    return (loss, best, gp) if hist is None else (loss, best, gp, hist)


def check_prior(dev, tag, poses, mix, w_gmm, w_angle):
    ref, f32 = cpu_prior(poses, mix, w_gmm, w_angle, torch.float64), cpu_prior(poses, mix, w_gmm, w_angle, torch.float32)
    loss, best, gp = hip_prior(dev, poses, mix, w_gmm, w_angle)
    print(f'{tag}: best {best.tolist()} (float64 {ref[1].tolist()})')
    ok = [within(tag, 'loss', loss, f32[0], ref[0]), within(tag, 'grad_poses', gp, f32[2], ref[2])]
    assert best.cpu().tolist() == ref[1].tolist()
    D = 0 if mix is None else mix[0].shape[1]
    quiet = [c for c in range(72) if not 3 <= c < 3 + D and c not in ANGLE_COLUMNS]
    assert bool((gp[:, quiet] == 0).all()), 'a column without a term has a gradient'
    assert all(ok)
    return loss, best, gp


@pytest.mark.parametrize('D', [1, 63, 64, 65, 69])
@pytest.mark.parametrize('M', [1, 8, 16])
@pytest.mark.parametrize('N', PRIOR_N)
def test_pose_prior_loss_best_and_gradient(dev, N, M, D):
    poses, mix = prior_case(N, M, D, seed=1000 * N + 10 * M + D)
    check_prior(dev, f'prior N={N} M={M} D={D}', poses, mix, W_GMM, W_ANGLE)


def test_mixture_off_and_angle_off(dev):
    poses, mix = prior_case(2, 8, 69, seed=21)
    loss, best, gp = check_prior(dev, 'prior M=0', poses, None, W_GMM, W_ANGLE)
    rest = [c for c in range(72) if c not in ANGLE_COLUMNS]
    assert bool((loss[:, 0] == 0).all()) and best.tolist() == [-1, -1] and bool((gp[:, rest] == 0).all())
    assert bool((gp[:, ANGLE_COLUMNS] != 0).all())
    loss, best, gp = check_prior(dev, 'prior w_angle=0', poses, mix, W_GMM, 0.)
    assert bool((loss[:, 1] > 0).all())                          # the loss is reported unweighted
    _, _, only_gmm = cpu_prior(poses, mix, W_GMM, 0., torch.float64)
    assert bool((only_gmm[:, :3] == 0).all()) and bool((gp[:, :3] == 0).all())


@pytest.mark.parametrize('M,a,b', [(8, 2, 5), (16, 3, 11), (16, 9, 12)])     # two waves; one wave in two rounds; two waves, second round
def test_a_tie_goes_to_the_lower_index(dev, M, a, b):
    g = torch.Generator().manual_seed(30 + a)
    means, prec, offs = mixture(M, 69, 31 + a)
    means[b], prec[b], offs[b] = means[a], prec[a], offs[a]
    poses = (0.5 * torch.randn(3, 72, generator=g))
    poses[:, 3:] = means[a][None] + 0.1 * torch.randn(3, 69, generator=g)
    q = gmm_q_torch(poses, means, prec, offs)
    assert torch.equal(q[:, a], q[:, b]) and bool((q.argsort(1)[:, :2].sort(1).values == torch.tensor([a, b])).all())
    loss, best, _ = hip_prior(dev, poses, (means, prec, offs), W_GMM, W_ANGLE)
    assert best.tolist() == [a] * 3
    assert float((loss[:, 0].cpu().double() - q[:, a]).abs().max()) <= 8 * FLOOR * float(q[:, a].abs().max())


def test_a_nan_pose_stays_with_its_person(dev):
    poses, mix = prior_case(3, 8, 69, seed=40)
    clean = hip_prior(dev, poses, mix, W_GMM, W_ANGLE)
    bad = poses.clone()
    bad[1, 10] = float('nan')
    bad[1, 55] = float('nan')
    got = hip_prior(dev, bad, mix, W_GMM, W_ANGLE)
    for x, y in zip(clean, got):
        assert torch.equal(x[[0, 2]], y[[0, 2]])
    assert bool(torch.isnan(got[0][1]).all()) and bool(torch.isnan(got[2][1, 3:]).any())


def test_pose_prior_accumulates(dev):
    poses, mix = prior_case(2, 8, 69, seed=50)
    plain = hip_prior(dev, poses, mix, W_GMM, W_ANGLE)
    on_zero = hip_prior(dev, poses, mix, W_GMM, W_ANGLE, accumulate=1, old=torch.zeros(2, 72))
    assert all(torch.equal(x, y) for x, y in zip(plain, on_zero))
    old = torch.randn(2, 72, generator=torch.Generator().manual_seed(51))
    got = hip_prior(dev, poses, mix, W_GMM, W_ANGLE, accumulate=1, old=old)
    ref, f32 = cpu_prior(poses, mix, W_GMM, W_ANGLE, torch.float64), cpu_prior(poses, mix, W_GMM, W_ANGLE, torch.float32)
    assert within('prior accumulate', 'grad_poses', got[2], old + f32[2].float(), old.double() + ref[2])
    assert torch.equal(got[2][:, :3].cpu(), old[:, :3])          # nothing acts on the global orientation
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])


def test_pose_prior_twice_on_a_side_stream_and_the_history_row(dev):
    poses, mix = prior_case(2, 16, 69, seed=60)
    a = hip_prior(dev, poses, mix, W_GMM, W_ANGLE, history_rows=3, row=2)
    b = hip_prior(dev, poses, mix, W_GMM, W_ANGLE, history_rows=3, row=2)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert torch.equal(a[3][2], a[0]) and bool(torch.isnan(a[3][:2]).all())       # the row asked for, and nothing else
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        c = hip_prior(dev, poses, mix, W_GMM, W_ANGLE)
    s.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a[:3], c))


# ------------------------------------------------------------------------------------------------ the 3-D term
RESIDUAL = 0.05                                                  # the noise put on the targets, per coordinate
SIGMA = 0.1 * RESIDUAL * 3 ** 0.5                                # Geman-McClure at a tenth of the typical residual
WEIGHT = 0.6


def j3d_case(N, K, seed, inds=None, with_trans=True):
    """Seeded float32 joints (N,71,3), trans (N,3) or None, targets (N,K,3) = the picked joints (+ trans) plus noise of RESIDUAL per
    coordinate, conf (N,K) in (0.2, 1]."""
    g = torch.Generator().manual_seed(seed)
    joints = 0.4 * torch.randn(N, J, 3, generator=g)
    trans = torch.cat([0.3 * torch.randn(N, 2, generator=g), 1.7 + 5.1 * torch.rand(N, 1, generator=g)], 1) if with_trans else None
    X = joints[:, :K] if inds is None else joints[:, torch.as_tensor(inds)]
    X = X if trans is None else X + trans[:, None]
    targets = X + RESIDUAL * torch.randn(N, K, 3, generator=g)
    conf = 0.2 + 0.8 * torch.rand(N, K, generator=g)
    return joints, trans, targets, conf


def cpu_j3d(joints, trans, targets, conf, inds, align, sigma, weight, dtype):
    j = joints.to(dtype).clone().requires_grad_(True)
    t = None if trans is None else trans.to(dtype).clone().requires_grad_(True)
    loss = joints3d_torch(j, targets, conf, inds, align, sigma, t, dtype)
    (weight * loss).sum().backward()                             # the gradients carry the weight, the loss does not
    return loss.detach().double(), j.grad.double(), None if t is None else t.grad.double()


def hip_j3d(dev, joints, trans, targets, conf, inds, align, sigma, weight, accumulate=0, old=None, history_rows=0, row=0):
    from romp_amd import fitting as F
    N = joints.shape[0]
    d = lambda t: None if t is None else t.to(dev).contiguous()
    loss = nan_like(dev, N)
    gj = nan_like(dev, N, joints.shape[1], 3) if old is None else old[0].to(dev).clone()
    gt = None if trans is None else (nan_like(dev, N, 3) if old is None else old[1].to(dev).clone())
    hist = nan_like(dev, history_rows, N) if history_rows else None
    F._joints3d(d(joints), d(trans), d(targets), d(conf), F._inds(inds, targets.shape[1]), F._align(align), sigma, weight, loss, gj,
                gt, accumulate, hist, row)
    torch.cuda.synchronize()
    return (loss, gj, gt) if hist is None else (loss, gj, gt, hist)


def holds(tag, name, hip, f32, ref):
    """`within`, and where the float64 reference is all zeros (one keypoint aligned on itself) the device's are exact zeros."""
    if float(ref.abs().max()) == 0:
        print(f'{tag} {name}: the reference is all zeros, max|hip| {float(hip.abs().max()):.3e}')
        return hip.shape == ref.shape and bool((hip == 0).all())
    return within(tag, name, hip, f32, ref)


def check_j3d(dev, tag, joints, trans, targets, conf, inds, align, sigma):
    ref = cpu_j3d(joints, trans, targets, conf, inds, align, sigma, WEIGHT, torch.float64)
    f32 = cpu_j3d(joints, trans, targets, conf, inds, align, sigma, WEIGHT, torch.float32)
    got = hip_j3d(dev, joints, trans, targets, conf, inds, align, sigma, WEIGHT)
    ok = [holds(tag, 'loss', got[0], f32[0], ref[0]), holds(tag, 'grad_joints', got[1], f32[1], ref[1])]
    K = targets.shape[1]
    picked = list(range(K)) if inds is None else list(inds)
    rest = [j for j in range(J) if j not in picked]
    assert bool((got[1][:, rest] == 0).all()), 'a joint that was not picked has a gradient'
    if trans is not None and align:
        assert bool((got[2] == 0).all()) and float(ref[2].abs().max()) <= 1e-12, 'grad_trans under alignment'
    elif trans is not None:
        ok.append(within(tag, 'grad_trans', got[2], f32[2], ref[2]))
    assert all(ok)
    return got


def align_set(K, n_align):
    return [None, [K // 2], [0, K - 1]][n_align]


J3D_CASES = [c for c in itertools.product([1, 3, 5], [1, 24, 65, 71], [False, True], [0, 1, 2], [0., SIGMA]) if c[3] <= c[1]]


@pytest.mark.parametrize('N,K,with_trans,n_align,sigma', J3D_CASES)
def test_joints3d_loss_and_gradients(dev, N, K, with_trans, n_align, sigma):
    joints, trans, targets, conf = j3d_case(N, K, seed=100 * N + K, with_trans=with_trans)
    check_j3d(dev, f'3d N={N} K={K} trans={with_trans} align={n_align} sigma={sigma:.3g}', joints, trans, targets, conf, None,
              align_set(K, n_align), sigma)


@pytest.mark.parametrize('n_align', [0, 2])
@pytest.mark.parametrize('K', [24, 71])
def test_joints3d_permuted_joint_inds(dev, K, n_align):
    inds = torch.randperm(J, generator=torch.Generator().manual_seed(K))[:K].tolist()
    assert inds != sorted(inds)
    joints, trans, targets, conf = j3d_case(5, K, seed=7, inds=inds)
    check_j3d(dev, f'3d permuted K={K} align={n_align}', joints, trans, targets, conf, inds, align_set(K, n_align), SIGMA)


def test_joints3d_null_conf_stands_for_ones(dev):
    joints, trans, targets, _ = j3d_case(3, 65, seed=8)
    a = check_j3d(dev, '3d conf=None', joints, trans, targets, None, None, [0, 64], 0.)
    b = hip_j3d(dev, joints, trans, targets, torch.ones(3, 65), None, [0, 64], 0., WEIGHT)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('n_align', [0, 2])
def test_joints3d_invisible_keypoints(dev, n_align):
    """Person 0 loses three keypoints, one by each rule (conf 0, x = -2, a NaN coordinate); person 1 has every conf 0;
    person 2 has a NaN in a joint whose keypoint is invisible, which must not get in."""
    joints, trans, targets, conf = j3d_case(3, 65, seed=9)
    conf[0, 10] = 0
    targets[0, 3, 0] = -2.
    targets[0, 40, 2] = float('nan')
    conf[1] = 0
    conf[2, 5] = 0
    joints[2, 5, 1] = float('nan')
    align = align_set(65, n_align)
    clean = joints.clone()
    clean[2, 5, 1] = 0.
    ref = cpu_j3d(clean, trans, targets, conf, None, align, 0., WEIGHT, torch.float64)
    f32 = cpu_j3d(clean, trans, targets, conf, None, align, 0., WEIGHT, torch.float32)
    got = hip_j3d(dev, joints, trans, targets, conf, None, align, 0., WEIGHT)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert float(got[0][1]) == 0 and bool((got[1][1] == 0).all()) and bool((got[2][1] == 0).all())
    assert bool((got[1][0, [3, 10, 40]] == 0).all()) and bool((got[1][2, 5] == 0).all())
    assert bool((got[1][0, [2, 4, 39]] != 0).any(1).all())
    ok = [within(f'3d invisible align={n_align}', n, h, f, r) for n, h, f, r in zip(('loss', 'grad_joints'), got, f32, ref)]
    if not n_align:
        ok.append(within('3d invisible', 'grad_trans', got[2], f32[2], ref[2]))
    assert all(ok)


@pytest.mark.parametrize('rule', ['conf', 'minus two', 'nan'])
def test_joints3d_an_invisible_alignment_keypoint_switches_the_person_off(dev, rule):
    joints, trans, targets, conf = j3d_case(3, 24, seed=10)
    if rule == 'conf':
        conf[1, 23] = 0
    elif rule == 'minus two':
        targets[1, 23, 0] = -2.
    else:
        targets[1, 23, 1] = float('nan')
    got = check_j3d(dev, f'3d hidden alignment keypoint ({rule})', joints, trans, targets, conf, None, [0, 23], SIGMA)
    assert float(got[0][1]) == 0 and bool((got[1][1] == 0).all()) and bool((got[2] == 0).all())
    assert float(got[0][0]) > 0 and float(got[0][2]) > 0 and bool((got[1][[0, 2]][:, :24] != 0).any(2).all())


@pytest.mark.parametrize('n_align', [0, 2])
def test_joints3d_accumulates(dev, n_align):
    joints, trans, targets, conf = j3d_case(5, 65, seed=11)
    align = align_set(65, n_align)
    plain = hip_j3d(dev, joints, trans, targets, conf, None, align, SIGMA, WEIGHT)
    on_zero = hip_j3d(dev, joints, trans, targets, conf, None, align, SIGMA, WEIGHT, accumulate=1, old=(torch.zeros(5, J, 3), torch.zeros(5, 3)))
    assert all(torch.equal(x, y) for x, y in zip(plain, on_zero))
    g = torch.Generator().manual_seed(12)
    old = (0.1 * torch.randn(5, J, 3, generator=g), 0.1 * torch.randn(5, 3, generator=g))
    got = hip_j3d(dev, joints, trans, targets, conf, None, align, SIGMA, WEIGHT, accumulate=1, old=old)
    ref = cpu_j3d(joints, trans, targets, conf, None, align, SIGMA, WEIGHT, torch.float64)
    f32 = cpu_j3d(joints, trans, targets, conf, None, align, SIGMA, WEIGHT, torch.float32)
    ok = [within(f'3d accumulate align={n_align}', 'grad_joints', got[1], old[0] + f32[1].float(), old[0].double() + ref[1]),
          within(f'3d accumulate align={n_align}', 'grad_trans', got[2], old[1] + f32[2].float(), old[1].double() + ref[2])]
    assert torch.equal(got[1][:, 65:].cpu(), old[0][:, 65:]) and torch.equal(got[0], plain[0])
    if n_align:
        assert torch.equal(got[2].cpu(), old[1])
    assert all(ok)


def test_joints3d_twice_on_a_side_stream_and_the_history_row(dev):
    joints, trans, targets, conf = j3d_case(5, 71, seed=13)
    a = hip_j3d(dev, joints, trans, targets, conf, None, [0, 70], SIGMA, WEIGHT, history_rows=3, row=1)
    b = hip_j3d(dev, joints, trans, targets, conf, None, [0, 70], SIGMA, WEIGHT, history_rows=3, row=1)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert torch.equal(a[3][1], a[0]) and bool(torch.isnan(a[3][[0, 2]]).all())
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        c = hip_j3d(dev, joints, trans, targets, conf, None, [0, 70], SIGMA, WEIGHT)
    s.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a[:3], c))


# ------------------------------------------------------------------------------------------------ autograd
def fit_mixture(seed=70):
    """Eight components over the full body pose, means 0.3 randn: the scale of the poses the fits below move through."""
    return mixture(8, 69, seed, spread=0.3)


def prior_object(dev, mix):
    from romp_amd.fitting import PosePrior
    return PosePrior.__new__(PosePrior)._set(mix[0], mix[1], mix[2], dev)


@pytest.mark.parametrize('with_trans,root_align,align', [(False, False, None), (True, True, [0, 8])])
def test_the_new_losses_through_the_layer(dev, with_trans, root_align, align):
    from romp_amd.fitting import joints3d_loss, pose_prior_loss
    model, smpl = layer(dev)
    N, K = 3, 24
    g = torch.Generator().manual_seed(14)
    betas, poses = torch.randn(N, 10, generator=g), 0.3 * torch.randn(N, 72, generator=g)
    trans = torch.tensor([[0.1, -0.2, 3.0], [-0.3, 0.1, 5.0], [0.2, 0.3, 2.5]]) if with_trans else None
    mix = fit_mixture()
    assert float(gmm_margin(gmm_q_torch(poses, *mix)).min()) >= MARGIN
    inds = torch.randperm(J, generator=g)[:K].tolist()
    _, jt = smpl_torch(model, betas, poses, root_align, torch.float64)
    targets = (jt[:, inds] + (0 if trans is None else trans[:, None].double()) + RESIDUAL * torch.randn(N, K, 3, generator=g).double()).float()
    conf = 0.2 + 0.8 * torch.rand(N, K, generator=g)
    weights = torch.tensor([[1.0, 0.5, 2.0], [0.02, 0.05, 0.01], [0.03, 0.01, 0.02]])      # per term and person

    def cpu(dtype):
        b, p = (t.to(dtype).clone().requires_grad_(True) for t in (betas, poses))
        t = None if trans is None else trans.to(dtype).clone().requires_grad_(True)
        _, j = smpl_torch(model, b, p, root_align, dtype)
        l3 = joints3d_torch(j, targets, conf, inds, align, SIGMA, t, dtype)
        gmm, _ = gmm_prior_torch(p, mix[0], mix[1], mix[2], dtype)
        ang = angle_prior_torch(p, dtype)
        (torch.stack([l3, gmm, ang]) * weights.to(dtype)).sum().backward()
        out = [l3.detach().double(), gmm.detach().double(), ang.detach().double(), b.grad.double(), p.grad.double()]
        return out + ([] if t is None else [t.grad.double()])

    ref, f32 = cpu(torch.float64), cpu(torch.float32)
    b, p = (t.to(dev).requires_grad_(True) for t in (betas, poses))
    t = None if trans is None else trans.to(dev).requires_grad_(True)
    _, j, _ = smpl(b, p, root_align=root_align)
    l3 = joints3d_loss(j, targets.to(dev), conf.to(dev), inds, align, sigma=SIGMA, trans=t)
    gmm, ang = pose_prior_loss(p, prior_object(dev, mix))
    assert l3.shape == gmm.shape == ang.shape == (N,) and l3.grad_fn is not None and gmm.grad_fn is not None and ang.grad_fn is not None
    (torch.stack([l3, gmm, ang]) * weights.to(dev)).sum().backward()
    torch.cuda.synchronize()
    got = [l3.detach(), gmm.detach(), ang.detach(), b.grad, p.grad] + ([] if t is None else [t.grad])
    names = ('loss3d', 'gmm', 'angle', 'betas.grad', 'poses.grad', 'trans.grad')
    if align and t is not None:
        assert bool((got[5] == 0).all()) and float(ref[5].abs().max()) <= 1e-12
        got, ref, f32 = got[:5], ref[:5], f32[:5]
    assert all([within(f'autograd trans={with_trans}', n, h, f, r) for n, h, f, r in zip(names, got, f32, ref)])
    none, ang2 = pose_prior_loss(p.detach(), None)               # without a mixture the first loss is zeros
    assert bool((none == 0).all()) and torch.equal(ang2, ang.detach())


# ------------------------------------------------------------------------------------------------ KeypointFitter
def targets3d_for(model, b0, p0, c0, camera, root_align, seed):
    """3-D targets near the start: its joints (camera-space points with the perspective camera) plus noise; one hidden."""
    g = torch.Generator().manual_seed(seed)
    _, jt = smpl_torch(model, b0, p0, root_align, torch.float64)
    jt = jt + (c0[:, None].double() if camera == 'perspective' else 0)
    t3 = (jt + RESIDUAL * torch.randn(jt.shape, generator=g).double()).float()
    t3[1, 30, 0] = -2.
    return t3, 0.2 + 0.8 * torch.rand(jt.shape[:2], generator=g)


FIT_KEYS = ('betas', 'poses', 'cam', 'loss_history', 'loss3d_history', 'prior_history')


@pytest.mark.parametrize('camera,root_align', [('weak', False), ('perspective', True)])
def test_three_steps_with_every_term_equal_the_float64_loop(dev, camera, root_align):
    """Three steps at N = 2 with 2-D + 3-D + GMM + angle + L2 against the float64 CPU loop (fit_prior_loop_torch), parameter by
    parameter; the yardstick is the same loop in float32.  The argmin margin is asserted at every step of the float64 loop."""
    from romp_amd.fitting import KeypointFitter
    model, smpl = layer(dev)
    b0, p0, c0, kp, conf = fit_case(model, camera, root_align)
    t3, c3 = targets3d_for(model, b0, p0, c0, camera, root_align, 41)
    mix = fit_mixture()
    args = dict(steps=3, lr=0.02, sigma=0.05, w_betas=1e-3, w_pose=2e-3, w_gmm=0.01, w_angle=0.02, w_3d=0.7, sigma_3d=0.2)
    loop = lambda dtype: fit_prior_loop_torch(model, b0, p0, c0, kp, conf, t3, c3, mix, camera=camera, root_align=root_align,
                                              align=[0, 8], dtype=dtype, **args)
    want, f32 = loop(torch.float64), loop(torch.float32)
    print(f'fitter {camera}: smallest argmin margin over the float64 loop {want["margin"]:.3g}')
    assert want['margin'] >= MARGIN
    got = KeypointFitter(smpl, camera=camera, root_align=root_align, pose_prior=prior_object(dev, mix), align_inds=[0, 8], **args).fit(
        b0, p0, c0, kp, conf, joints3d=t3, conf3d=c3)
    torch.cuda.synchronize()
    assert got['loss_history'].shape == got['loss3d_history'].shape == (4, 2) and got['prior_history'].shape == (4, 2, 2)
    ok = [within(f'fitter all terms {camera}', k, got[k], f32[k], want[k]) for k in FIT_KEYS]
    for k, start in (('betas', b0), ('poses', p0), ('cam', c0)):
        assert float((got[k].cpu() - start).abs().max()) > 0.02
    v, j, _ = smpl(got['betas'], got['poses'], root_align=root_align)
    assert torch.equal(v, got['verts']) and torch.equal(j, got['joints'])
    assert all(ok)


@pytest.mark.parametrize('camera,root_align', [('weak', False), ('perspective', True)])
def test_three_steps_on_3d_targets_alone(dev, camera, root_align):
    """kp2d = None: no 2-D launch, loss_history is zeros; without alignment, so that the perspective camera moves too.  The weak
    camera has no term and stays where it started."""
    from romp_amd.fitting import KeypointFitter
    model, smpl = layer(dev)
    b0, p0, c0, _, _ = fit_case(model, camera, root_align)
    t3, c3 = targets3d_for(model, b0 + 0.3, p0 * 1.3, c0 * 1.02, camera, root_align, 42)
    args = dict(steps=3, lr=0.02, w_betas=1e-3, w_pose=2e-3, w_3d=1.5, sigma_3d=0.3)
    loop = lambda dtype: fit_prior_loop_torch(model, b0, p0, c0, None, None, t3, c3, None, camera=camera, root_align=root_align,
                                              dtype=dtype, **args)
    want, f32 = loop(torch.float64), loop(torch.float32)
    got = KeypointFitter(smpl, camera=camera, root_align=root_align, **args).fit(b0, p0, c0, None, joints3d=t3, conf3d=c3)
    torch.cuda.synchronize()
    assert 'prior_history' not in got and bool((got['loss_history'] == 0).all()) and got['loss_history'].shape == (4, 2)
    keys = ('betas', 'poses', 'loss3d_history') + (('cam',) if camera == 'perspective' else ())
    ok = [within(f'fitter 3-D only {camera}', k, got[k], f32[k], want[k]) for k in keys]
    if camera == 'weak':
        assert torch.equal(got['cam'].cpu(), c0)
    assert bool((got['loss3d_history'][-1] < got['loss3d_history'][0]).all()) and all(ok)


@pytest.mark.parametrize('camera,root_align', [('weak', False), ('perspective', True)])
def test_the_defaults_are_the_old_fitter(dev, camera, root_align):
    """With the new arguments at their defaults the fitter is the loop of its four old launches, bit for bit."""
    from romp_amd import fitting as F
    from romp_amd import lib as L
    model, smpl = layer(dev)
    b0, p0, c0, kp, conf = fit_case(model, camera, root_align)
    steps, lr, sigma, ra = 3, 0.02, 0.05, int(root_align)
    got = F.KeypointFitter(smpl, camera=camera, root_align=root_align, steps=steps, lr=lr, sigma=sigma).fit(b0, p0, c0, kp, conf)
    assert set(got) == {'betas', 'poses', 'cam', 'verts', 'joints', 'loss_history'}
    h, ctx, st = L.load(), smpl._context(), L.stream_ptr(dev)
    b, p, c, kp_d, conf_d = (t.to(dev).float().contiguous().clone() for t in (b0, p0, c0, kp, conf))
    ref = p.clone()
    f32 = dict(device=dev, dtype=torch.float32)
    verts, joints = torch.empty(2, 6890, 3, **f32), torch.empty(2, J, 3, **f32)
    loss, gj, gc, gb, gp = torch.empty(2, **f32), torch.empty(2, J, 3, **f32), torch.empty(2, 3, **f32), torch.empty_like(b), torch.empty_like(p)
    hist = torch.empty(steps + 1, 2, **f32)
    wb = torch.full((10,), 1e-4, **f32)
    wp = torch.cat([torch.zeros(3, **f32), torch.full((69,), 1e-4, **f32)])
    state = [torch.zeros_like(t) for t in (b, p, c, b, p, c)]
    segs = (L.FitSegment * 3)(L.FitSegment(b.data_ptr(), gb.data_ptr(), state[0].data_ptr(), state[3].data_ptr(), None, wb.data_ptr(), 2, 10),
                              L.FitSegment(p.data_ptr(), gp.data_ptr(), state[1].data_ptr(), state[4].data_ptr(), ref.data_ptr(), wp.data_ptr(), 2, 72),
                              L.FitSegment(c.data_ptr(), gc.data_ptr(), state[2].data_ptr(), state[5].data_ptr(), None, None, 2, 3))
    for s in range(steps + 1):
        L.check(h.smpl_forward(ctx, L.ptr(b), 10, L.ptr(p), 2, ra, L.ptr(verts), L.ptr(joints), st))
        L.check(h.romp_fit_reproject(L.ptr(joints), 2, J, L.ptr(c), L.ptr(kp_d), L.ptr(conf_d), J, None, F.CAMERAS[camera], 443.4, 256.,
                                     sigma, L.ptr(loss), L.ptr(gj), L.ptr(gc), L.ptr(hist), s, st))
        if s == steps:
            break
        L.check(h.smpl_backward(ctx, L.ptr(b), 10, L.ptr(p), 2, ra, None, L.ptr(gj), L.ptr(gb), L.ptr(gp), st))
        L.check(h.romp_fit_adam(segs, 3, lr, 0.9, 0.999, 1e-8, s + 1, st))
    torch.cuda.synchronize()
    for k, t in (('betas', b), ('poses', p), ('cam', c), ('verts', verts), ('joints', joints), ('loss_history', hist)):
        assert torch.equal(got[k], t), k


def prior_drive_mixture():
    means, prec, _ = mixture(1, 69, 80, spread=0.3)
    return means, prec, torch.tensor([0.5])


def test_a_fit_that_the_prior_drives(dev):
    """No keypoint is visible; a one-component prior sits at a seeded pose mu (0.3 randn), w_gmm = 1, the start is zeros; the
    recipe's defaults otherwise (30 steps, lr 0.02, L2 priors 1e-4).  The float64 CPU loop (fit_prior_loop_torch) under this
    recipe takes the mixture term of either person (they start alike) from 7.54 to 1.12 (the offset is 0.5): a fall of 6.42;
    the device must reach a third of that fall."""
    from romp_amd.fitting import KeypointFitter
    cpu_fall = (6.42, 6.42)
    model, smpl = layer(dev)
    mix = prior_drive_mixture()
    kp, conf = torch.zeros(2, J, 2), torch.zeros(2, J)
    res = KeypointFitter(smpl, pose_prior=prior_object(dev, mix), w_gmm=1.).fit(torch.zeros(2, 10), torch.zeros(2, 72),
                                                                               torch.tensor([[0.9, 0.05, -0.03], [0.7, -0.1, 0.08]]), kp, conf)
    hist = res['prior_history']
    assert hist.shape == (31, 2, 2) and hist.is_cuda and bool(torch.isfinite(hist).all()) and bool((res['loss_history'] == 0).all())
    fall = (hist[0, :, 0] - hist[-1, :, 0]).cpu().tolist()
    print(f'prior-driven fit: gmm {hist[0, :, 0].cpu().tolist()} -> {hist[-1, :, 0].cpu().tolist()}, fall {fall} (float64 CPU loop: {cpu_fall})')
    assert bool((hist[-1, :, 0] < hist[0, :, 0]).all()) and all(f >= c / 3 for f, c in zip(fall, cpu_fall))


# ------------------------------------------------------------------------------------------------ refine_outputs
@pytest.mark.parametrize('kind', ['romp', 'bev'])
def test_refine_outputs_with_prior_and_3d_targets(dev, kind):
    from romp_amd.fitting import refine_outputs
    model = stand_in(dev, kind)
    out = synthetic_outputs(dev, model, kind)
    steps = 4
    mix = fit_mixture()
    targets = out['joints'] + (out['cam_trans'][:, None] if kind == 'bev' else 0) + 0.02
    conf3d = torch.ones(3, J, device=dev)
    res = refine_outputs(model, out, out['pj2d_org'] + 8., pad_info=PAD, steps=steps, lr=0.01, joints3d=targets, conf3d=conf3d,
                         pose_prior=prior_object(dev, mix), w_gmm=0.01, w_angle=0.01, w_3d=0.5, align_inds=[0])
    torch.cuda.synchronize()
    assert res['prior_history'].shape == (steps + 1, 3, 2) and res['loss3d_history'].shape == (steps + 1, 3)
    assert res['fit_loss'].shape == (3, 2) and res['verts'].shape == (3, 6890, 3) and res['joints'].shape == (3, J, 3)
    assert res['smpl_thetas'].shape == (3, 72) and res['smpl_betas'].shape == out['smpl_betas'].shape
    for k in ('prior_history', 'loss3d_history', 'fit_loss'):
        assert bool(torch.isfinite(res[k]).all()), k
    assert bool((res['prior_history'][:, :, 1] > 0).all()) and bool((res['loss3d_history'] > 0).all())
    adults = [0, 1, 2] if kind == 'romp' else [0, 2]             # BEV: the second person is an infant, fitted without the mixture
    assert bool((res['prior_history'][:, adults, 0] != 0).all())
    if kind == 'bev':
        assert bool((res['prior_history'][:, 1, 0] == 0).all())
    only3d = refine_outputs(model, out, None, pad_info=PAD, steps=steps, lr=0.01, joints3d=targets)
    torch.cuda.synchronize()
    assert 'prior_history' not in only3d and bool((only3d['fit_loss'] == 0).all())
    assert only3d['loss3d_history'].shape == (steps + 1, 3) and bool(torch.isfinite(only3d['loss3d_history']).all())
