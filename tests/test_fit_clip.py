"""Temporal smoothness terms for the device fitter and the acceleration metric, CPU part (include/romp_hip_fit_clip.h,
csrc/fit_clip.hip, romp_amd/clip.py): the exported symbols, their argument checks (they return before any HIP call),
`clip_links`, and the torch / numpy restatements that tests/test_gpu_fit_clip.py measures the device against:
  `links_of`               the link rule: (prev, next) -> for every row the linked rows or -1;
  `temporal_torch`         Lvel and Lacc of one tensor, built term by term from the link rule; gradients come from autograd;
  `rotation_smooth_torch`  Lrot on `batch_rodrigues_torch` of tests/test_smpl_grad.py;
  `accel_np`               compute_accel / compute_error_accel (evaluation_matrix.py:424-465) restated for one chain in frame order;
  `fit_clip_loop_torch`    `fit_prior_loop_torch` of tests/test_fit_priors.py plus the new terms.
All are pinned here in float64 by cases computed by hand.  tests/make_golden_clip.py writes a fixture from the reference's
own functions where their module can be imported; it needs packages that are not part of this project's environment, so
`accel_np` is pinned by hand alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_fit import prior_weights, reproject_torch
from test_fit_priors import angle_prior_torch, fit_prior_loop_torch, gmm_prior_torch, joints3d_torch
from test_smpl_grad import batch_rodrigues_torch, model_for, smpl_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatements
def links_of(prev, nxt):
    """The link rule.  -> (pv, nx): lists; pv[n] = p iff prev[n] == p, 0 <= p < N, p != n and next[p] == n, else -1; nx[p] = n
    for that same link."""
    prev, nxt = [int(v) for v in prev], [int(v) for v in nxt]
    N = len(prev)
    pv, nx = [-1] * N, [-1] * N
    for n in range(N):
        p = prev[n]
        if 0 <= p < N and p != n and nxt[p] == n:
            pv[n], nx[p] = p, n
    return pv, nx


def rho_torch(e, sigma):
    s = float(np.float32(sigma))
    return e if s <= 0 else (s * s) * e / (s * s + e)


def temporal_torch(x, prev, nxt, col_w=None, sigma_vel=0., sigma_acc=0., dtype=torch.float64):
    """x (N, ...) read as (N, cols) -> (Lvel (N,), Lacc (N,)), differentiable in x: for every row the terms whose links exist,
    zero otherwise (include/romp_hip_fit_clip.h)."""
    N = x.shape[0]
    x = x.to(dtype).reshape(N, -1)
    w = torch.ones(x.shape[1], dtype=dtype) if col_w is None else col_w.to(dtype).reshape(-1)
    pv, nx = links_of(prev, nxt)
    zero = torch.zeros((), dtype=dtype)
    vel = [rho_torch((w * (x[n] - x[pv[n]]) ** 2).sum(), sigma_vel) if pv[n] >= 0 else zero for n in range(N)]
    acc = [rho_torch((w * (x[pv[n]] - 2 * x[n] + x[nx[n]]) ** 2).sum(), sigma_acc) if pv[n] >= 0 and nx[n] >= 0 else zero for n in range(N)]
    return (torch.stack(vel), torch.stack(acc)) if N else (torch.zeros(0, dtype=dtype), torch.zeros(0, dtype=dtype))


def rotation_smooth_torch(poses, prev, nxt, joint_w=None, sigma=0., dtype=torch.float64):
    """poses (N,72) -> Lrot (N,) = rho(sum_j joint_w[j] |R_j(n) - R_j(pv)|_F^2), zero without the link."""
    N = poses.shape[0]
    R = batch_rodrigues_torch(poses.to(dtype).reshape(-1, 3)).reshape(N, 24, 9)
    w = torch.ones(24, dtype=dtype) if joint_w is None else joint_w.to(dtype).reshape(-1)
    pv, _ = links_of(prev, nxt)
    zero = torch.zeros((), dtype=dtype)
    return torch.stack([rho_torch((w[:, None] * (R[n] - R[pv[n]]) ** 2).sum(), sigma) if pv[n] >= 0 else zero for n in range(N)])


def accel_np(joints, gt=None, vis=None):
    """One chain in frame order, joints (T,J,3): -> (values (T-2,), keep (T-2,) bool); entry i is centred on frame i + 1.
    Without gt compute_accel (evaluation_matrix.py:432-435), with gt compute_error_accel (:451-454); keep is its new_vis
    (:456-463), which the reference applies as normed[new_vis]."""
    joints = np.asarray(joints, np.float64)
    accel = joints[:-2] - 2 * joints[1:-1] + joints[2:]                                  # :432-433, :452
    if gt is not None:
        gt = np.asarray(gt, np.float64)
        accel = accel - (gt[:-2] - 2 * gt[1:-1] + gt[2:])                                # :451, :454
    normed = np.linalg.norm(accel, axis=2)                                               # :434, :454
    if vis is None:
        keep = np.ones(len(normed), dtype=bool)                                          # :457
    else:
        invis = np.logical_not(np.asarray(vis).astype(bool))                             # :459
        keep = np.logical_not(np.logical_or(invis, np.logical_or(np.roll(invis, -1), np.roll(invis, -2)))[:-2])   # :460-463
    return np.mean(normed, axis=1), keep                                                 # :435, :465


SMOOTH_COLUMNS = ('joints', 'cam', 'betas', 'rot')


def fit_clip_loop_torch(model, betas0, poses0, cam0, links, kp2d=None, conf=None, joints3d=None, conf3d=None, prior=None, steps=30,
                        lr=0.02, sigma=0., camera='weak', w_betas=1e-4, w_pose=1e-4, root_align=False, w_gmm=0., w_angle=0., w_3d=1.,
                        sigma_3d=0., align=None, w_smooth_pose=0., joint_w=None, w_smooth_joints=(0., 0.), smooth_joint_inds=None,
                        w_smooth_cam=(0., 0.), w_smooth_betas=0., sigma_smooth=0., dtype=torch.float64):
    """KeypointFitter.fit with links on the CPU: the loop of fit_prior_loop_torch with  w_smooth_joints . (Lvel, Lacc) of the 71
    joints (213 columns, three of weight one per joint of smooth_joint_inds), w_smooth_cam . (Lvel, Lacc) of the camera,
    w_smooth_betas Lvel of the betas and w_smooth_pose Lrot added to the objective.  -> the dict of fit_prior_loop_torch (without
    its margin) plus smooth_history (steps + 1, N, L): (vel, acc) for joints, cam, betas, then rot, each when its term is on."""
    prev, nxt = links
    b, p, c = (t.to(dtype).clone().requires_grad_(True) for t in (betas0, poses0, cam0))
    ref = poses0.to(dtype).clone()
    wb, wp = prior_weights(w_betas, b.shape[1]).to(dtype), prior_weights(w_pose, 72, free=3).to(dtype)
    col_w = None
    if smooth_joint_inds is not None:
        col_w = torch.zeros(71, 3, dtype=dtype)
        col_w[list(smooth_joint_inds)] = 1.
        col_w = col_w.reshape(213)
    on = {'joints': max(w_smooth_joints) > 0, 'cam': max(w_smooth_cam) > 0, 'betas': w_smooth_betas > 0, 'rot': w_smooth_pose > 0}
    opt = torch.optim.Adam([b, p, c], lr=lr)
    h2, h3, hp, hs = [], [], [], []
    for s in range(steps + 1):
        opt.zero_grad()
        _, joints = smpl_torch(model, b, p, root_align, dtype)
        zeros = torch.zeros(b.shape[0], dtype=dtype)
        l2 = reproject_torch(joints, c, kp2d, conf, None, sigma, camera, dtype) if kp2d is not None else zeros
        l3 = joints3d_torch(joints, joints3d, conf3d, None, align, sigma_3d, c if camera == 'perspective' else None, dtype) \
            if joints3d is not None else zeros
        gmm = gmm_prior_torch(p, prior[0], prior[1], prior[2], dtype)[0] if prior is not None and w_gmm > 0 else zeros
        ang = angle_prior_torch(p, dtype)
        total = l2 + w_3d * l3 + w_gmm * gmm + w_angle * ang
        cols = []
        if on['joints']:
            v, a = temporal_torch(joints, prev, nxt, col_w, sigma_smooth, sigma_smooth, dtype)
            total, cols = total + w_smooth_joints[0] * v + w_smooth_joints[1] * a, cols + [v, a]
        if on['cam']:
            v, a = temporal_torch(c, prev, nxt, None, sigma_smooth, sigma_smooth, dtype)
            total, cols = total + w_smooth_cam[0] * v + w_smooth_cam[1] * a, cols + [v, a]
        if on['betas']:
            v, a = temporal_torch(b, prev, nxt, None, sigma_smooth, sigma_smooth, dtype)
            total, cols = total + w_smooth_betas * v, cols + [v, a]
        if on['rot']:
            r = rotation_smooth_torch(p, prev, nxt, joint_w, sigma_smooth, dtype)
            total, cols = total + w_smooth_pose * r, cols + [r]
        h2.append(l2.detach().clone()), h3.append(l3.detach().clone()), hp.append(torch.stack([gmm.detach(), ang.detach()], 1))
        hs.append(torch.stack([t.detach() for t in cols], 1) if cols else torch.zeros(b.shape[0], 0, dtype=dtype))
        if s == steps:
            break
        if total.requires_grad:
            total.sum().backward()
        for t in (b, p, c):
            t.grad = torch.zeros_like(t) if t.grad is None else t.grad
        b.grad += 2 * wb[None] * b.detach()
        p.grad += 2 * wp[None] * (p.detach() - ref)
        opt.step()
    return {'betas': b.detach(), 'poses': p.detach(), 'cam': c.detach(), 'loss_history': torch.stack(h2), 'loss3d_history': torch.stack(h3),
            'prior_history': torch.stack(hp), 'smooth_history': torch.stack(hs)}


def chain(N):
    """(prev, next) of one chain 0 -> 1 -> ... -> N - 1 as int32 tensors."""
    prev = torch.arange(-1, N - 1, dtype=torch.int32)
    nxt = torch.arange(1, N + 1, dtype=torch.int32)
    if N:
        nxt[-1] = -1
    return prev, nxt


# ------------------------------------------------------------------------------------------------ pinned by hand
def test_the_link_rule():
    assert links_of([-1, 0, 1], [1, 2, -1]) == ([-1, 0, 1], [1, 2, -1])
    assert links_of([-1, 0, 1], [2, 2, -1]) == ([-1, -1, 1], [-1, 2, -1])          # next[0] != 1: no link 0 -> 1
    assert links_of([-1, 1, 1], [1, 2, -1]) == ([-1, -1, 1], [-1, 2, -1])          # prev[1] == 1: a row is not its own neighbour
    assert links_of([7, -5, 1], [1, 2, 9]) == ([-1, -1, 1], [-1, 2, -1])           # out of range: never an index
    assert links_of([], []) == ([], [])


def test_velocity_and_acceleration_of_three_rows_by_hand():
    """x = 0, 1, 3 in one column: v = -, 1, 2 and a_1 = 0 - 2 + 3 = 1.  The gradient of sum (Lvel + Lacc): row 0 gets
    -2 v_1 + 2 a_1 = 0, row 1 gets 2 v_1 - 2 v_2 - 4 a_1 = -6, row 2 gets 2 v_2 + 2 a_1 = 6."""
    x = torch.tensor([[0.], [1.], [3.]], dtype=torch.float64, requires_grad=True)
    prev, nxt = chain(3)
    vel, acc = temporal_torch(x, prev, nxt)
    assert vel.tolist() == [0., 1., 4.] and acc.tolist() == [0., 1., 0.]
    (vel + acc).sum().backward()
    assert x.grad[:, 0].tolist() == [0., -6., 6.]
    vel, acc = temporal_torch(x.detach(), prev, nxt, col_w=torch.tensor([2.]))
    assert vel.tolist() == [0., 2., 8.] and acc.tolist() == [0., 2., 0.]
    vel, acc = temporal_torch(x.detach(), prev, nxt, sigma_vel=2., sigma_acc=1.)     # 4 e / (4 + e); e / (1 + e)
    assert vel.tolist() == [0., 4. / 5., 16. / 8.] and acc.tolist() == [0., 0.5, 0.]
    vel, acc = temporal_torch(x.detach(), [-1, 0, 1], [2, 2, -1])                    # the link 0 -> 1 is inconsistent
    assert vel.tolist() == [0., 0., 4.] and acc.tolist() == [0., 0., 0.]
    two = torch.tensor([[0., 3.], [1., 1.]], dtype=torch.float64)                    # two columns: 1 + 4
    assert temporal_torch(two, *chain(2))[0].tolist() == [0., 5.]


def test_rotation_term_is_four_times_one_minus_cosine():
    """Row 0 is the zero pose (R = I exactly: rv / |rv + 1e-8| = 0), row 1 turns joint 3 by 0.5 about z and joint 7 by 0.25 about
    x: |R - I|_F^2 = 4 (1 - cos phi) each, up to the 1e-8 of the layer's formula."""
    poses = torch.zeros(2, 72, dtype=torch.float64)
    poses[1, 3 * 3 + 2], poses[1, 3 * 7] = 0.5, 0.25
    want = 4 * (1 - np.cos(0.5)) + 4 * (1 - np.cos(0.25))
    got = rotation_smooth_torch(poses, *chain(2))
    assert float(got[0]) == 0. and abs(float(got[1]) - want) <= 1e-7
    w = torch.ones(24, dtype=torch.float64)
    w[3], w[7] = 0.5, 0.
    assert abs(float(rotation_smooth_torch(poses, *chain(2), joint_w=w)[1]) - 2 * (1 - np.cos(0.5))) <= 1e-7
    e = 4 * (1 - np.cos(0.5)) + 4 * (1 - np.cos(0.25))
    assert abs(float(rotation_smooth_torch(poses, *chain(2), sigma=0.5)[1]) - 0.25 * e / (0.25 + e)) <= 1e-7
    flipped = torch.zeros(2, 72, dtype=torch.float64)                               # the same rotation named by both axis signs
    flipped[0, 3:6] = torch.tensor([0., 0., np.pi - 0.01])
    flipped[1, 3:6] = torch.tensor([0., 0., -(np.pi + 0.01)])
    assert float(rotation_smooth_torch(flipped, *chain(2))[1]) <= 1e-7


def test_accel_np_by_hand():
    """Three frames, two joints: joint 0 moves 0, 1, 4 along x (acceleration 2), joint 1 moves (0,0,0), (0,3,0), (0,6,4)
    (acceleration (0,0,4), norm 4): mean 3.  Against a ground truth that accelerates joint 0 by (2, 0, 0) too and joint 1 by
    (0, 3, 0): differences (0,0,0) and (0,-3,4), norms 0 and 5, mean 2.5."""
    J = np.array([[[0., 0, 0], [0, 0, 0]], [[1, 0, 0], [0, 3, 0]], [[4, 0, 0], [0, 6, 4]]])
    value, keep = accel_np(J)
    assert value.tolist() == [3.] and keep.tolist() == [True]
    G = np.array([[[5., 5, 5], [1, 1, 1]], [[5, 5, 5], [1, 1, 1]], [[7, 5, 5], [1, 4, 1]]])
    value, keep = accel_np(J, G)
    assert value.tolist() == [2.5] and keep.tolist() == [True]
    five = np.zeros((5, 1, 3))
    for hidden, want in ((0, [False, True, True]), (2, [False, False, False]), (4, [True, True, False]), (1, [False, False, True])):
        vis = np.ones(5, bool)
        vis[hidden] = False
        assert accel_np(five, five, vis)[1].tolist() == want, hidden


def test_the_clip_loop_with_the_terms_off_is_the_prior_loop():
    model = model_for(10)
    g = torch.Generator().manual_seed(3)
    b0, p0 = 0.5 * torch.randn(3, 10, generator=g), 0.2 * torch.randn(3, 72, generator=g)
    c0 = torch.tensor([[0.9, 0.05, -0.03], [0.7, -0.1, 0.08], [0.8, 0., 0.]])
    kp = 0.3 * torch.randn(3, 71, 2, generator=g)
    want = fit_prior_loop_torch(model, b0, p0, c0, kp, steps=2, w_angle=0.01)
    got = fit_clip_loop_torch(model, b0, p0, c0, chain(3), kp, steps=2, w_angle=0.01)
    for k in ('betas', 'poses', 'cam', 'loss_history', 'prior_history'):
        assert torch.equal(got[k], want[k]), k
    assert got['smooth_history'].shape == (3, 3, 0)


def test_one_step_of_the_clip_loop_by_hand():
    """3-D targets that are the start's own joints (no residual, no gradient), no L2 priors, the camera term alone on a chain of
    two rows with cam = (1, 0, 0) and (2, 0, 0): the gradient of |cam_1 - cam_0|^2 is -2 and +2 on the first column and zero
    elsewhere, and the first Adam step moves a parameter by lr g / (|g| + eps): by +lr and -lr."""
    model = model_for(10)
    b0, p0 = torch.zeros(2, 10), torch.zeros(2, 72)
    c0 = torch.tensor([[1., 0., 0.], [2., 0., 0.]])
    _, joints = smpl_torch(model, b0, p0, False, torch.float64)
    got = fit_clip_loop_torch(model, b0, p0, c0, chain(2), None, None, joints, steps=1, lr=0.125, w_betas=0., w_pose=0.,
                              w_smooth_cam=(1., 0.))
    want = torch.tensor([[1.125, 0., 0.], [1.875, 0., 0.]], dtype=torch.float64)
    assert float((got['cam'] - want).abs().max()) <= 1e-8
    assert float(got['betas'].abs().max()) == 0. and float(got['poses'].abs().max()) == 0.
    assert got['smooth_history'].shape == (2, 2, 2)
    assert got['smooth_history'][0].tolist() == [[0., 0.], [1., 0.]]
    assert abs(float(got['smooth_history'][1, 1, 0]) - 0.75 ** 2) <= 1e-8


# ------------------------------------------------------------------------------------------------ clip_links
def test_clip_links_by_hand():
    from romp_amd.clip import clip_links
    L = lambda t, f, **k: tuple(x.tolist() for x in clip_links(torch.tensor(t), torch.tensor(f), **k))
    # two tracks interleaved in frame-major order: rows 0, 2, 4 are track 7 and rows 1, 3, 5 track 3
    assert L([7, 3, 7, 3, 7, 3], [0, 0, 1, 1, 2, 2]) == ([-1, -1, 0, 1, 2, 3], [2, 3, 4, 5, -1, -1])
    # a singleton track between them
    assert L([7, 9, 7], [0, 0, 1]) == ([-1, -1, 0], [2, -1, -1])
    # a gap of two frames: cut with max_gap 1, linked with 2
    assert L([1, 1, 1], [0, 1, 3]) == ([-1, 0, -1], [1, -1, -1])
    assert L([1, 1, 1], [0, 1, 3], max_gap=2) == ([-1, 0, 1], [1, 2, -1])
    # a (track, frame) pair twice: rows 1 and 2 are never linked to each other; the chain runs 0 -> 1 and 2 -> 3
    assert L([1, 1, 1, 1], [0, 1, 1, 2]) == ([-1, 0, -1, 2], [1, -1, 3, -1])
    # shuffled rows: track 5 at frames 2, 0, 1 in rows 0, 2, 3; track 6 at frames 1, 0 in rows 1, 4
    assert L([5, 6, 5, 5, 6], [2, 1, 0, 1, 0]) == ([3, 4, -1, 2, -1], [-1, -1, 3, 0, 1])
    prev, nxt = clip_links(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    assert prev.shape == nxt.shape == (0,) and prev.dtype == nxt.dtype == torch.int32
    prev, nxt = clip_links([4], [0])
    assert prev.tolist() == [-1] and nxt.tolist() == [-1]
    with pytest.raises(ValueError):
        clip_links(torch.zeros(3), torch.zeros(2))


def test_clip_links_obey_the_link_rule_on_a_seeded_clip():
    from romp_amd.clip import clip_links
    g = torch.Generator().manual_seed(5)
    track, frame = torch.randint(0, 6, (60,), generator=g), torch.randint(0, 12, (60,), generator=g)
    prev, nxt = clip_links(track, frame, max_gap=2)
    pv, nx = links_of(prev, nxt)
    assert pv == prev.tolist() and nx == nxt.tolist()                 # every entry is a link: nothing stale
    for n, p in enumerate(pv):
        if p >= 0:
            assert int(track[p]) == int(track[n]) and 1 <= int(frame[n]) - int(frame[p]) <= 2


# ------------------------------------------------------------------------------------------------ the C seam
def test_fit_clip_symbols_exported():
    from romp_amd import lib
    header = open(os.path.join(ROOT, 'include', 'romp_hip_fit_clip.h')).read()
    declared = re.findall(r'^\s*(?:int|void)\s+(\w+)\s*\(', header, re.M)
    assert declared == lib.FIT_CLIP_EXPORTS == ['romp_fit_temporal', 'romp_clip_accel']
    others = (lib.EXPORTS + lib.VIEW_EXPORTS + lib.MAP_EXPORTS + lib.TEXTURE_EXPORTS + lib.EVAL_EXPORTS + lib.RH_EXPORTS +
              lib.CANVAS_EXPORTS + lib.SMPL_GRAD_EXPORTS + lib.FIT_EXPORTS + lib.FIT_PRIOR_EXPORTS + lib.TRACK_EXPORTS + lib.MOT_EXPORTS)
    assert not set(declared) & set(others)
    h = lib.load()
    assert h.romp_abi_version() == 7 == lib.ABI_VERSION
    assert len(h.romp_fit_temporal.argtypes) == 16 and len(h.romp_clip_accel.argtypes) == 12
    for n in declared:
        assert getattr(h, n).restype is ctypes.c_int, n
    assert 'ROMP_CLIP_MAX_SEGMENTS 4' in header and 'next[p] == n' in header
    assert 'fit_clip.hip' in __import__('romp_amd.build', fromlist=['SOURCES']).SOURCES


def test_the_header_compiles_as_c_and_the_segment_is_the_bindings():
    import subprocess
    import tempfile
    from romp_amd import lib
    prog = ('#include <stddef.h>\n#include <stdio.h>\n#include "romp_hip_fit_clip.h"\nint main(void) { printf("%d %d %d %d\\n", (int)sizeof(romp_clip_segment), '
            '(int)offsetof(romp_clip_segment, cols), (int)offsetof(romp_clip_segment, sigma_vel), (int)offsetof(romp_clip_segment, accumulate)); '
            'return ROMP_CLIP_MAX_SEGMENTS == 4 ? 0 : 1; }\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, 't.c')
        open(c, 'w').write(prog)
        subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), c, '-o', os.path.join(td, 't')])
        out = subprocess.check_output([os.path.join(td, 't')]).split()
    S = lib.ClipSegment
    assert [int(v) for v in out] == [ctypes.sizeof(S), S.cols.offset, S.sigma_vel.offset, S.accumulate.offset]


def _host_pointer():
    buf = (ctypes.c_float * 1024)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_fit_temporal_rejects_bad_arguments_before_any_device_call():
    from romp_amd import lib
    h = lib.load()
    keep, p = _host_pointer()                                    # never dereferenced: every call below fails its checks first
    P = p.value

    def seg(x=P, grad=P, col_w=None, cols=3, w_vel=1., w_acc=1.):
        return lib.ClipSegment(x, grad, col_w, cols, w_vel, w_acc, 0., 0., 0)

    def call(segs=(seg(),), n_seg=None, table=True, prev=p, nxt=p, N=1, poses=None, w_rot=1., gp=None, loss=p, hist=None, row=0):
        arr = (lib.ClipSegment * max(len(segs), 1))(*segs) if table else None
        return h.romp_fit_temporal(arr, len(segs) if n_seg is None else n_seg, prev, nxt, N, None, poses, None, w_rot, 0., gp, 0, loss,
                                   hist, row, None)

    for bad in (dict(table=False), dict(prev=None), dict(nxt=None), dict(loss=None), dict(n_seg=-1), dict(n_seg=5),
                dict(segs=(), n_seg=0), dict(segs=(seg(x=None),)), dict(segs=(seg(grad=None),)), dict(segs=(seg(), seg(cols=0))),
                dict(segs=(seg(w_vel=-1.),)), dict(segs=(seg(w_acc=-0.5),)), dict(segs=(seg(w_acc=float('nan')),)),
                dict(poses=p), dict(poses=p, gp=p, w_rot=-1.), dict(N=-1), dict(row=-1)):
        assert call(**bad) == -1 and b'romp_fit_temporal' in h.romp_last_error(), bad
    assert call(N=0) == 0                                        # nothing to do, nothing launched
    assert call(N=0, segs=(seg(),) * 4, poses=p, gp=p) == 0 and call(N=0, segs=(), n_seg=0, table=False, poses=p, gp=p) == 0
    assert call(N=0, segs=(seg(cols=0),)) == -1 and call(N=0, row=-1) == -1          # the checks do not depend on N


def test_clip_accel_rejects_bad_arguments_before_any_device_call():
    from romp_amd import lib
    h = lib.load()
    keep, p = _host_pointer()
    I = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def call(joints=p, N=1, J=4, gt=None, vis=None, K=2, inds=None, prev=p, nxt=p, value=p, valid=p):
        return h.romp_clip_accel(joints, N, J, gt, vis, K, inds, prev, nxt, value, valid, None)

    for bad in (dict(joints=None), dict(prev=None), dict(nxt=None), dict(value=None), dict(valid=None), dict(N=-1), dict(K=0), dict(K=5),
                dict(J=257, K=1), dict(inds=I(0, 0)), dict(inds=I(0, 4)), dict(inds=I(-1, 2))):
        assert call(**bad) == -1 and b'romp_clip_accel' in h.romp_last_error(), bad
    assert call(N=0) == 0 and call(N=0, gt=p, vis=p, inds=I(3, 1)) == 0
    assert call(N=0, inds=I(3, 3)) == -1


def test_the_clip_terms_need_the_device():
    """No CPU fallback, as for the other losses."""
    from romp_amd.clip import rotation_smoothness_loss, temporal_loss
    from romp_amd.evaluation import accel
    from romp_amd.lib import RompHipError
    with pytest.raises(RompHipError):
        temporal_loss(torch.zeros(3, 5), chain(3))
    with pytest.raises(RompHipError):
        rotation_smoothness_loss(torch.zeros(3, 72), chain(3))
    with pytest.raises(RompHipError):
        accel(torch.zeros(3, 14, 3), chain(3))
    with pytest.raises(ValueError):
        temporal_loss(torch.zeros(3, 5), chain(3), order=3)
    with pytest.raises(ValueError):
        temporal_loss(torch.zeros(3, 5), chain(2))


def test_fitter_smoothness_arguments():
    from romp_amd.fitting import KeypointFitter
    from romp_amd.smpl import SMPL
    from romp_amd.synthetic import make_smpl_model
    smpl = SMPL(make_smpl_model())
    f = KeypointFitter(smpl)
    assert (f.w_smooth_pose, f.w_smooth_joints, f.w_smooth_cam, f.w_smooth_betas, f.sigma_smooth, f.smooth_on) == \
        (0., (0., 0.), (0., 0.), 0., 0., False)
    f = KeypointFitter(smpl, w_smooth_joints=(0., 2.), w_smooth_cam=0.5)
    assert f.w_smooth_joints == (0., 2.) and f.w_smooth_cam == (0.5, 0.) and f.smooth_on
    for bad in (dict(w_smooth_pose=-1.), dict(w_smooth_joints=(1., -1.)), dict(w_smooth_cam=(-1., 0.)), dict(w_smooth_betas=-1.)):
        with pytest.raises(ValueError):
            KeypointFitter(smpl, **bad)
