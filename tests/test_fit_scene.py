"""Scene terms for the device fitter, CPU part (include/romp_hip_fit_scene.h, csrc/fit_scene.hip, romp_amd/scene.py): the exported
symbol, its argument checks (they return before any HIP call), `scene_groups`, `body_spheres`, and the float64 torch
restatements that tests/test_gpu_fit_scene.py measures the device against:
  `scenes_of`             the table rule: (offsets, members) -> the rows of every scene, in member order;
  `translation_torch`     a row's translation from its camera, by camera mode;
  `depth_order_torch`     the depth-order term, built pair by pair; gradients come from autograd;
  `collision_torch`       the sphere-proxy collision term between the persons of a scene;
  `fit_scene_loop_torch`  `fit_loop_torch` of tests/test_fit.py plus the two terms.
`depth_order_torch` is pinned by tests/golden/fit_scene.npz, which scripts/make_golden_fit_scene.py wrote from the reference's
own relative_depth_loss (values and gradients, both depth_loss_type values); `collision_torch` by a brute-force triple loop
written separately here and by torch.autograd.gradcheck."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from test_fit import fit_loop_torch, prior_weights, project_torch, reproject_torch
from test_smpl_grad import model_for, smpl_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'fit_scene.npz')


# ------------------------------------------------------------------------------------------------ the restatements
def scenes_of(offsets, members):
    """The table rule.  -> the list of scenes, each the list of its rows in member order: group g counts iff
    0 <= offsets[g] <= offsets[g + 1] <= N, an entry iff 0 <= member < N.  Empty groups are left out.  The tables of the tests
    name every row at most once (asserted), so a row's scene is the one that holds it."""
    offsets, members = [int(v) for v in offsets], [int(v) for v in members]
    N = len(members)
    assert len(offsets) == N + 1
    out, seen = [], set()
    for g in range(N):
        lo, hi = offsets[g], offsets[g + 1]
        if lo < 0 or lo > hi or hi > N:
            continue
        rows = [m for m in members[lo:hi] if 0 <= m < N]
        assert not seen & set(rows) and len(set(rows)) == len(rows)
        seen |= set(rows)
        if rows:
            out.append(rows)
    return out


def tables_of(scenes, N):
    """The (offsets, members) of a list of scenes, as int32 tensors; rows in no scene are padded with -1."""
    offsets, members = [0], []
    for rows in scenes:
        members += list(rows)
        offsets.append(len(members))
    offsets += [len(members)] * (N + 1 - len(offsets))
    members += [-1] * (N - len(members))
    return torch.tensor(offsets, dtype=torch.int32), torch.tensor(members, dtype=torch.int32)


def translation_torch(cam, camera, dtype=torch.float64):
    """perspective: t = cam; weak, cam = (s, c1, c2): t = 2 (c1 / s, c2 / s, 1 / s)."""
    cam = cam.to(dtype)
    if camera == 'perspective':
        return cam
    return 2 * torch.stack([cam[:, 1] / cam[:, 0], cam[:, 2] / cam[:, 0], 1 / cam[:, 0]], 1)


def softplus_torch(x):
    """max(x, 0) + log1p(exp(-|x|)), branch by branch so that autograd gives sigmoid(x) everywhere, 1/2 at zero included."""
    return torch.where(x >= 0, x + torch.log1p(torch.exp(-x.clamp(min=0))), torch.log1p(torch.exp(x.clamp(max=0))))


def depth_pairs_torch(z, ids, scenes, thresh, kind):
    """-> for every scene the list of its active pairs (row i, row j, term), i before j in member order."""
    out = []
    for rows in scenes:
        lab = [m for m in rows if int(ids[m]) >= 0]
        pairs = []
        for x in range(len(lab)):
            for y in range(x + 1, len(lab)):
                i, j = lab[x], lab[y]
                d, k = z[j] - z[i], int(ids[j]) - int(ids[i])
                if k == 0:
                    pairs.append((i, j, d * d))
                elif k < 0 and (kind == 'log' or bool(d - k * thresh > 0)):
                    pairs.append((i, j, softplus_torch(d)))
                elif k > 0 and (kind == 'log' or bool(d - k * thresh < 0)):
                    pairs.append((i, j, softplus_torch(-d)))
        out.append(pairs)
    return out


def depth_order_torch(z, ids, offsets, members, thresh=0.3, kind='piecewise', dtype=torch.float64):
    """z (N,) -> loss (N,), differentiable in z: loss[n] = (1 / 2A) * the sum of the active pairs of n's scene that contain n,
    A = the scene's number of active pairs; zeros where A == 0 (include/romp_hip_fit_scene.h)."""
    z = z.to(dtype)
    N = z.shape[0]
    loss = [torch.zeros((), dtype=dtype) for _ in range(N)]
    for pairs in depth_pairs_torch(z, ids, scenes_of(offsets, members), thresh, kind):
        for i, j, f in pairs:
            loss[i] = loss[i] + f / (2 * len(pairs))
            loss[j] = loss[j] + f / (2 * len(pairs))
    return torch.stack(loss) if N else torch.zeros(0, dtype=dtype)


def sphere_centres_torch(joints, cam, spheres, radius_scale, camera, dtype):
    """-> centres (N,S,3) and sigma^2 (N,S); spheres = (p, q, a, r) lists, a and r as the floats the C entry takes."""
    p, q, a, r = spheres
    J, t = joints.to(dtype), translation_torch(cam, camera, dtype)
    a = torch.tensor([float(np.float32(v)) for v in a], dtype=dtype)
    r = torch.tensor([float(np.float32(v)) for v in r], dtype=dtype)
    centres = (1 - a)[None, :, None] * J[:, list(p)] + a[None, :, None] * J[:, list(q)] + t[:, None]
    scale = torch.ones(J.shape[0], dtype=dtype) if radius_scale is None else radius_scale.to(dtype)
    sigma = r[None] / 3 * scale[:, None]
    return centres, sigma * sigma


def collision_torch(joints, cam, offsets, members, spheres, radius_scale=None, camera='perspective', dtype=torch.float64):
    """joints (N,J,3), cam (N,3) -> loss (N,), differentiable in both: loss[n] = 1/2 sum over the other rows m of n's scene
    and the sphere pairs (s, u) of exp(-|c_ns - c_mu|^2 / (sigma_ns^2 + sigma_mu^2))."""
    N = joints.shape[0]
    c, s2 = sphere_centres_torch(joints, cam, spheres, radius_scale, camera, dtype)
    loss = [torch.zeros((), dtype=dtype) for _ in range(N)]
    for rows in scenes_of(offsets, members):
        for n in rows:
            others = [m for m in rows if m != n]
            if others:
                d2 = ((c[n][None, :, None, :] - c[others][:, None, :, :]) ** 2).sum(-1)          # (M, S, S)
                loss[n] = 0.5 * torch.exp(-d2 / (s2[n][None, :, None] + s2[others][:, None, :])).sum()
    return torch.stack(loss) if N else torch.zeros(0, dtype=dtype)


def fit_scene_loop_torch(model, betas0, poses0, cam0, groups, kp2d, conf=None, depth_ids=None, steps=30, lr=0.02, sigma=0.,
                         camera='weak', w_betas=1e-4, w_pose=1e-4, root_align=False, w_depth_order=0., depth_loss_type='piecewise',
                         dist_thresh=0.3, w_collision=0., spheres=None, radius_scale=None, dtype=torch.float64):
    """KeypointFitter.fit with scene tables on the CPU: the loop of fit_loop_torch with  w_depth_order * depth_order_torch  on
    z = the third column of translation_torch(cam) and  w_collision * collision_torch  on the 71 joints added to the objective.
    -> the dict of fit_loop_torch plus scene_history (steps + 1, N, 2): (depth, collision), zeros for a term that is off."""
    offsets, members = groups
    b, p, c = (t.to(dtype).clone().requires_grad_(True) for t in (betas0, poses0, cam0))
    ref = poses0.to(dtype).clone()
    wb, wp = prior_weights(w_betas, b.shape[1]).to(dtype), prior_weights(w_pose, 72, free=3).to(dtype)
    thresh = float(np.float32(dist_thresh))
    opt = torch.optim.Adam([b, p, c], lr=lr)
    h2, hs = [], []
    for s in range(steps + 1):
        opt.zero_grad()
        _, joints = smpl_torch(model, b, p, root_align, dtype)
        zeros = torch.zeros(b.shape[0], dtype=dtype)
        l2 = reproject_torch(joints, c, kp2d, conf, None, sigma, camera, dtype)
        dep = depth_order_torch(translation_torch(c, camera, dtype)[:, 2], depth_ids, offsets, members, thresh, depth_loss_type, dtype) \
            if w_depth_order > 0 and depth_ids is not None else zeros
        col = collision_torch(joints, c, offsets, members, spheres, radius_scale, camera, dtype) if w_collision > 0 else zeros
        total = l2 + w_depth_order * dep + w_collision * col
        h2.append(l2.detach().clone()), hs.append(torch.stack([dep.detach(), col.detach()], 1))
        if s == steps:
            break
        total.sum().backward()
        b.grad += 2 * wb[None] * b.detach()
        p.grad += 2 * wp[None] * (p.detach() - ref)
        opt.step()
    return {'betas': b.detach(), 'poses': p.detach(), 'cam': c.detach(), 'loss_history': torch.stack(h2), 'scene_history': torch.stack(hs)}


# ------------------------------------------------------------------------------------------------ pinned by the reference
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('kind', ['Piecewise', 'Log'])
def test_depth_restatement_equals_the_reference(kind):
    """The two sums of the header: a scene's rows sum to the reference's mean over that image, and the sum over all rows
    divided by the number of scenes with an active pair is the reference's scalar; its gradient is the reference's."""
    from romp_amd.scene import scene_groups
    G = golden()
    z = torch.tensor(G['z'], requires_grad=True)
    ids, frames, thresh = torch.tensor(G['ids']), torch.tensor(G['frames']), float(G['thresh'])
    offsets, members = scene_groups(frames)
    loss = depth_order_torch(z, ids, offsets, members, thresh, kind.lower())
    per_image = torch.zeros(int(frames.max()) + 1, dtype=torch.float64).index_add(0, frames, loss.detach())
    assert float((per_image - torch.tensor(G['image_' + kind])).abs().max()) <= 1e-12
    active = int((per_image > 0).sum())
    assert active == int((torch.tensor(G['image_' + kind]) > 0).sum()) >= 5
    scalar = loss.sum() / active
    assert abs(float(scalar.detach()) - float(G['scalar_' + kind])) <= 1e-12
    scalar.backward()
    assert float((z.grad - torch.tensor(G['grad_' + kind])).abs().max()) <= 1e-12
    assert float(z.grad.abs().max()) > 0.01


def test_the_fixture_holds_the_cases_it_was_made_for():
    G = golden()
    ids, frames = G['ids'], G['frames']
    labelled = [int(((frames == f) & (ids >= 0)).sum()) for f in range(int(frames.max()) + 1)]
    assert labelled[:4] == [1, 2, 3, 6] and (ids == -1).sum() == 2
    assert len(set(ids[frames == 4])) == 1 and labelled[4] == 3                      # the all-equal scene
    assert G['image_Piecewise'][5] == 0 and G['image_Log'][5] > 0                   # no active pair under Piecewise only
    assert G['image_Piecewise'][1] > 0                                              # a violated pair
    six = frames[(frames == 6) | (frames == 7)]
    assert (six[:-1] != six[1:]).all() and len(six) == 8                            # interleaved row by row
    assert G['image_Piecewise'][0] == 0 and G['image_Piecewise'][8] == 0


def test_depth_order_by_hand():
    """Two rows, ids (0, 1): the second must lie deeper.  z = (5, 3): d = -2, k = 1, softplus(2), active (d - 0.3 < 0); each row
    gets half.  z = (3, 5): d = 2, beyond the margin: inactive under piecewise, softplus(-2) under log.  At the margin exactly
    (thresh 0.25, d = 0.25) the pair is inactive: the comparison is strict."""
    off, mem = tables_of([[0, 1]], 2)
    ids = torch.tensor([0, 1])
    sp = lambda x: math.log1p(math.exp(x))
    got = depth_order_torch(torch.tensor([5., 3.], dtype=torch.float64), ids, off, mem)
    assert got.tolist() == pytest.approx([sp(2.) / 2] * 2, abs=1e-15)
    assert depth_order_torch(torch.tensor([3., 5.], dtype=torch.float64), ids, off, mem).tolist() == [0., 0.]
    got = depth_order_torch(torch.tensor([3., 5.], dtype=torch.float64), ids, off, mem, kind='log')
    assert got.tolist() == pytest.approx([sp(-2.) / 2] * 2, abs=1e-15)
    assert depth_order_torch(torch.tensor([1., 1.25], dtype=torch.float64), ids, off, mem, thresh=0.25).tolist() == [0., 0.]
    assert depth_order_torch(torch.tensor([1., 1.125], dtype=torch.float64), ids, off, mem, thresh=0.25)[0] > 0
    same = depth_order_torch(torch.tensor([1., 1.5, 9.], dtype=torch.float64), torch.tensor([4, 4, -1]), *tables_of([[0, 1, 2]], 3))
    assert same.tolist() == [0.125, 0.125, 0.]                                      # one pair of equal layers: d^2 / 2 each
    z = torch.tensor([800., -800.], dtype=torch.float64, requires_grad=True)        # the overflow-safe softplus
    got = depth_order_torch(z, ids, off, mem)
    got.sum().backward()
    assert got.tolist() == [800., 800.] and z.grad.tolist() == [1., -1.]


def collision_brute_force(joints, cam, scenes, spheres, radius_scale, camera):
    """The energy of the header with python floats, one sphere pair at a time."""
    p, q, a, r = spheres
    N = len(joints)
    loss = [0.] * N
    for rows in scenes:
        for n in rows:
            for m in rows:
                if m == n:
                    continue
                for s in range(len(p)):
                    for u in range(len(p)):
                        cs, sig = [], []
                        for row, k in ((n, s), (m, u)):
                            if camera == 'perspective':
                                t = [float(v) for v in cam[row]]
                            else:
                                t = [2 * float(cam[row][1]) / float(cam[row][0]), 2 * float(cam[row][2]) / float(cam[row][0]), 2 / float(cam[row][0])]
                            al = float(np.float32(a[k]))
                            cs.append([(1 - al) * float(joints[row][p[k]][x]) + al * float(joints[row][q[k]][x]) + t[x] for x in range(3)])
                            sig.append(float(np.float32(r[k])) / 3 * (1. if radius_scale is None else float(radius_scale[row])))
                        d2 = sum((cs[0][x] - cs[1][x]) ** 2 for x in range(3))
                        loss[n] += 0.5 * math.exp(-d2 / (sig[0] ** 2 + sig[1] ** 2))
    return loss


SPHERES3 = ([0, 1, 4], [0, 2, 3], [0., 0.5, 1.], [0.3, 0.2, 0.25])


@pytest.mark.parametrize('camera', ['perspective', 'weak'])
def test_collision_restatement_equals_the_triple_loop(camera):
    g = torch.Generator().manual_seed(11)
    N, J = 6, 5
    joints = 0.2 * torch.randn(N, J, 3, generator=g, dtype=torch.float64)
    if camera == 'perspective':
        cam = torch.tensor([0., 0., 3.]) + 0.1 * torch.randn(N, 3, generator=g, dtype=torch.float64)
    else:
        cam = torch.cat([0.9 + 0.02 * torch.rand(N, 1, generator=g, dtype=torch.float64), 0.02 * torch.randn(N, 2, generator=g, dtype=torch.float64)], 1)
    scale = 0.5 + torch.rand(N, generator=g, dtype=torch.float64)
    scenes = [[0, 3], [1], [2, 4, 5]]
    off, mem = tables_of(scenes, N)
    for rs in (None, scale):
        got = collision_torch(joints, cam, off, mem, SPHERES3, rs, camera)
        want = collision_brute_force(joints.tolist(), cam.tolist(), scenes, SPHERES3, None if rs is None else rs.tolist(), camera)
        assert float((got - torch.tensor(want, dtype=torch.float64)).abs().max()) <= 1e-12 * max(want)
        assert got[1] == 0 and min(want[0], want[2]) > 1e-3          # alone in its scene: exactly zero; the others overlap
    assert abs(float(got[[0, 3]].sum()) - 2 * float(got[0])) <= 1e-12                # a pair shares its energy half and half


def test_collision_by_hand():
    """One sphere on joint 0 (r = 0.3: sigma = 0.1), two persons whose joint 0 lies at the origin: coincident centres give
    exp(0) = 1, half to each row; 0.2 apart: exp(-0.04 / 0.02) = exp(-2)."""
    one = ([0], [0], [0.], [0.3])
    joints = torch.zeros(2, 1, 3, dtype=torch.float64)
    off, mem = tables_of([[0, 1]], 2)
    assert collision_torch(joints, torch.zeros(2, 3, dtype=torch.float64), off, mem, one).tolist() == [0.5, 0.5]
    cam = torch.tensor([[0., 0., 3.], [0.2, 0., 3.]], dtype=torch.float64)
    s2 = (float(np.float32(0.3)) / 3) ** 2
    assert collision_torch(joints, cam, off, mem, one).tolist() == pytest.approx([0.5 * math.exp(-0.04 / (2 * s2))] * 2, rel=1e-14)
    none = tables_of([[0], [1]], 2)
    assert collision_torch(joints, cam, *none, one).tolist() == [0., 0.]


def test_collision_gradcheck():
    g = torch.Generator().manual_seed(12)
    joints = (0.2 * torch.randn(4, 5, 3, generator=g, dtype=torch.float64)).requires_grad_(True)
    off, mem = tables_of([[0, 2, 3]], 4)
    scale = 0.5 + torch.rand(4, generator=g, dtype=torch.float64)
    w = torch.rand(4, generator=g, dtype=torch.float64)
    for camera, cam in (('perspective', 0.1 * torch.randn(4, 3, generator=g, dtype=torch.float64)),
                        ('weak', torch.cat([0.9 + 0.05 * torch.rand(4, 1, generator=g, dtype=torch.float64),
                                            0.03 * torch.randn(4, 2, generator=g, dtype=torch.float64)], 1))):
        cam = cam.clone().requires_grad_(True)
        fn = lambda j, c: (w * collision_torch(j, c, off, mem, SPHERES3, scale, camera)).sum()
        assert float(fn(joints, cam).detach()) > 1e-2
        assert torch.autograd.gradcheck(fn, (joints, cam), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_the_scene_loop_with_the_terms_off_is_the_plain_loop():
    model = model_for(10)
    g = torch.Generator().manual_seed(3)
    b0, p0 = 0.5 * torch.randn(3, 10, generator=g), 0.2 * torch.randn(3, 72, generator=g)
    c0 = torch.tensor([[0.9, 0.05, -0.03], [0.7, -0.1, 0.08], [0.8, 0., 0.]])
    kp = 0.3 * torch.randn(3, 71, 2, generator=g)
    want = fit_loop_torch(model, b0, p0, c0, kp, steps=2)
    got = fit_scene_loop_torch(model, b0, p0, c0, tables_of([[0, 1, 2]], 3), kp, depth_ids=torch.tensor([0, 1, 2]), steps=2)
    for k in ('betas', 'poses', 'cam', 'loss_history'):
        assert torch.equal(got[k], want[k]), k
    assert got['scene_history'].shape == (3, 3, 2) and float(got['scene_history'].abs().max()) == 0.


def test_one_step_of_the_scene_loop_by_hand():
    """Keypoints that are the start's own projection (no residual, no gradient), no L2 priors, the depth term alone under
    'log' on two rows with ids (0, 1) at z = (5, 3): the gradient of softplus(z_0 - z_1) / 1 is +sigmoid(2) on z_0 and
    -sigmoid(2) on z_1, and the first Adam step moves a parameter by lr g / (|g| + eps): z_0 by -lr, z_1 by +lr."""
    model = model_for(10)
    b0, p0 = torch.zeros(2, 10), torch.zeros(2, 72)
    c0 = torch.tensor([[0.1, 0., 5.], [-0.1, 0., 3.]])
    _, joints = smpl_torch(model, b0, p0, True, torch.float64)
    kp = project_torch(joints, c0, 'perspective')
    got = fit_scene_loop_torch(model, b0, p0, c0, tables_of([[0, 1]], 2), kp, depth_ids=torch.tensor([0, 1]), steps=1, lr=0.125,
                               camera='perspective', root_align=True, w_betas=0., w_pose=0., w_depth_order=2., depth_loss_type='log')
    want = torch.tensor([[0.1, 0., 4.875], [-0.1, 0., 3.125]], dtype=torch.float64)
    assert float((got['cam'] - want).abs().max()) <= 1e-7
    assert float(got['betas'].abs().max()) == 0. and float(got['poses'].abs().max()) == 0.
    sp = math.log1p(math.exp(2.))
    assert got['scene_history'][0].reshape(-1).tolist() == pytest.approx([sp / 2, 0., sp / 2, 0.], abs=1e-12)
    assert float(got['scene_history'][1, :, 0].sum()) < sp


# ------------------------------------------------------------------------------------------------ scene_groups, body_spheres
def test_scene_groups_by_hand():
    from romp_amd.scene import scene_groups
    G = lambda ids: tuple(t.tolist() for t in scene_groups(torch.tensor(ids)))
    off, mem = scene_groups(torch.zeros(0, dtype=torch.int64))
    assert off.tolist() == [0] and mem.shape == (0,) and off.dtype == mem.dtype == torch.int32
    assert G([7]) == ([0, 1], [0])
    assert G([-1]) == ([0, 0], [-1])
    assert G([0, 0, 1, 1, 1]) == ([0, 2, 5, 5, 5, 5], [0, 1, 2, 3, 4])             # repeated frames, already in order
    assert G([4, 2, 4, 2, 9]) == ([0, 2, 4, 5, 5, 5], [1, 3, 0, 2, 4])             # unsorted and interleaved: by frame id
    assert G([3, -1, 3, -5, 0]) == ([0, 1, 3, 3, 3, 3], [4, 0, 2, -1, -1])         # negative ids: in no group
    assert G([-1, -1]) == ([0, 0, 0], [-1, -1])
    off, mem = scene_groups([2, 2])                                                # anything torch.as_tensor takes
    assert off.tolist() == [0, 2, 2] and mem.tolist() == [0, 1]


def test_scene_groups_obey_the_table_rule_on_seeded_ids():
    from romp_amd.scene import scene_groups
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(-2, 9, (60,), generator=g)
    off, mem = scene_groups(ids)
    assert off.shape == (61,) and mem.shape == (60,)
    scenes = scenes_of(off, mem)
    assert sorted(m for rows in scenes for m in rows) == [n for n in range(60) if ids[n] >= 0]
    frames = [int(ids[rows[0]]) for rows in scenes]
    assert frames == sorted(set(frames))
    for rows in scenes:
        assert rows == sorted(rows) and len({int(ids[m]) for m in rows}) == 1


def test_body_spheres_of_the_synthetic_models():
    from romp_amd.scene import BodySpheres, body_spheres
    from romp_amd.smpl import SMPL
    for nb in (10, 11):
        smpl = SMPL(model_for(nb), model_type='smpl' if nb == 10 else 'smpla')
        sp = body_spheres(smpl)
        assert isinstance(sp, BodySpheres) and len(sp) == 47 <= 64
        assert all(0 <= v < 24 for v in sp.p + sp.q) and sp.a == [0.] * 24 + [0.5] * 23
        assert all(math.isfinite(v) and 0.03 <= v <= 0.15 for v in sp.r)
        parents = smpl.parents.tolist()
        assert [(p, q) for p, q in zip(sp.p[24:], sp.q[24:])] == [(parents[j], j) for j in range(1, 24)]
        again = body_spheres(smpl)
        assert (again.p, again.q, again.a, again.r) == (sp.p, sp.q, sp.a, sp.r)
        assert len(sp.table()) == 47 and sp.table()[30].q == sp.q[30]
    with pytest.raises(ValueError):
        BodySpheres([0] * 65, [0] * 65, [0.] * 65, [0.1] * 65)
    with pytest.raises(ValueError):
        BodySpheres([0], [0, 1], [0.], [0.1])


# ------------------------------------------------------------------------------------------------ the C seam
def test_fit_scene_symbols_exported():
    from romp_amd import lib
    header = open(os.path.join(ROOT, 'include', 'romp_hip_fit_scene.h')).read()
    declared = re.findall(r'^\s*(?:int|void)\s+(\w+)\s*\(', header, re.M)
    assert declared == lib.FIT_SCENE_EXPORTS == ['romp_fit_scene']
    others = (lib.EXPORTS + lib.VIEW_EXPORTS + lib.MAP_EXPORTS + lib.TEXTURE_EXPORTS + lib.EVAL_EXPORTS + lib.RH_EXPORTS +
              lib.CANVAS_EXPORTS + lib.SMPL_GRAD_EXPORTS + lib.FIT_EXPORTS + lib.FIT_PRIOR_EXPORTS + lib.FIT_CLIP_EXPORTS +
              lib.TRACK_EXPORTS + lib.MOT_EXPORTS)
    assert not set(declared) & set(others)
    assert len(lib.EXPORTS) == 52
    h = lib.load()
    assert h.romp_abi_version() == 7 == lib.ABI_VERSION
    assert len(h.romp_fit_scene.argtypes) == 24 and h.romp_fit_scene.restype is ctypes.c_int
    assert 'ROMP_SCENE_MAX_SPHERES 64' in header and '0 <= offsets[g] <= offsets[g + 1] <= N' in header and '0 <= member < N' in header
    assert 'fit_scene.hip' in __import__('romp_amd.build', fromlist=['SOURCES']).SOURCES


def test_the_header_compiles_as_c_and_the_sphere_is_the_bindings():
    import subprocess
    import tempfile
    from romp_amd import lib
    prog = ('#include <stddef.h>\n#include <stdio.h>\n#include "romp_hip_fit_scene.h"\nint main(void) { printf("%d %d %d %d %d\\n", '
            '(int)sizeof(romp_scene_sphere), (int)offsetof(romp_scene_sphere, p), (int)offsetof(romp_scene_sphere, q), '
            '(int)offsetof(romp_scene_sphere, a), (int)offsetof(romp_scene_sphere, r)); '
            'return ROMP_SCENE_MAX_SPHERES == 64 && ROMP_SCENE_PIECEWISE == 0 && ROMP_SCENE_LOG == 1 ? 0 : 1; }\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, 't.c')
        open(c, 'w').write(prog)
        subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), c, '-o', os.path.join(td, 't')])
        out = subprocess.check_output([os.path.join(td, 't')]).split()
    S = lib.SceneSphere
    assert [int(v) for v in out] == [ctypes.sizeof(S), S.p.offset, S.q.offset, S.a.offset, S.r.offset]
    from romp_amd.scene import KINDS
    assert KINDS == {'piecewise': 0, 'log': 1}


def _host_pointer():
    buf = (ctypes.c_float * 1024)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_fit_scene_rejects_bad_arguments_before_any_device_call():
    from romp_amd import lib
    h = lib.load()
    keep, p = _host_pointer()                                    # never dereferenced: every call below fails its checks first
    nan, inf = float('nan'), float('inf')

    def table(*entries):
        return (lib.SceneSphere * max(len(entries), 1))(*[lib.SceneSphere(*e) for e in entries])

    good = table((0, 1, 0.5, 0.1), (3, 3, 0., 0.2))

    def call(joints=p, N=1, J=4, cam=p, mode=1, offsets=p, members=p, ids=p, w_depth=1., thresh=0.3, kind=0, spheres=good, S=2, scale=None,
             w_col=1., term_w=None, gj=p, gc=p, loss=p, hist=None, row=0):
        return h.romp_fit_scene(joints, N, J, cam, mode, offsets, members, ids, w_depth, thresh, kind, spheres, S, scale, w_col, term_w,
                                gj, 0, gc, 0, loss, hist, row, None)

    bad_cases = (dict(cam=None), dict(offsets=None), dict(members=None), dict(gc=None),                    # required pointers
                 dict(joints=None), dict(gj=None), dict(spheres=None),                                     # required with S > 0
                 dict(ids=None, S=0, spheres=None),                                                       # no term at all
                 dict(w_depth=-1.), dict(w_col=-0.5), dict(w_depth=nan), dict(w_col=nan), dict(thresh=-0.1), dict(thresh=nan),
                 dict(S=-1), dict(S=65),
                 dict(spheres=table((0, 4, 0.5, 0.1)), S=1), dict(spheres=table((-1, 0, 0.5, 0.1)), S=1),   # joint index outside 0..J-1
                 dict(spheres=table((0, 1, nan, 0.1)), S=1), dict(spheres=table((0, 1, inf, 0.1)), S=1),
                 dict(spheres=table((0, 1, 0.5, nan)), S=1), dict(spheres=table((0, 1, 0.5, inf)), S=1),
                 dict(spheres=table((0, 1, 0.5, 0.)), S=1), dict(spheres=table((0, 1, 0.5, -0.1)), S=1),
                 dict(spheres=table((0, 1, 0.5, 0.1), (0, 9, 0.5, 0.1)), S=2),                             # the second entry is checked too
                 dict(J=257), dict(J=0), dict(kind=2), dict(kind=-1), dict(mode=2), dict(mode=-1), dict(N=-1), dict(row=-1),
                 dict(w_depth=0., w_col=0., loss=None))
    for bad in bad_cases:
        assert call(**bad) == -1 and b'romp_fit_scene' in h.romp_last_error(), bad
    assert call(N=0) == 0                                        # nothing to do, nothing launched
    assert call(N=0, ids=None) == 0 and call(N=0, S=0, spheres=None, joints=None, gj=None) == 0
    assert call(N=0, w_depth=0., w_col=0.) == 0 and call(N=0, loss=None) == 0
    assert call(N=0, J=256, spheres=table((255, 0, 1., 0.1)), S=1) == 0
    assert call(N=0, row=-1) == -1 and call(N=0, spheres=table((0, 4, 0.5, 0.1)), S=1) == -1     # the checks do not depend on N


def test_the_scene_terms_need_the_device():
    """No CPU fallback, as for the other losses."""
    from romp_amd.lib import RompHipError
    from romp_amd.scene import BodySpheres, collision_loss, depth_order_loss, scene_groups
    groups = scene_groups(torch.tensor([0, 0, 1]))
    with pytest.raises(RompHipError):
        depth_order_loss(torch.ones(3), torch.tensor([0, 1, 0]), groups)
    with pytest.raises(RompHipError):
        depth_order_loss(torch.ones(3, 3), torch.tensor([0, 1, 0]), groups, camera='weak')
    with pytest.raises(RompHipError):
        collision_loss(torch.zeros(3, 71, 3), torch.ones(3, 3), groups, BodySpheres([0], [1], [0.5], [0.1]))
    with pytest.raises(ValueError):
        depth_order_loss(torch.ones(3), torch.tensor([0, 1, 0]), groups, kind='linear')
    with pytest.raises(ValueError):
        depth_order_loss(torch.ones(3), torch.tensor([0, 1]), groups)
    with pytest.raises(ValueError):
        depth_order_loss(torch.ones(3), torch.tensor([0, 1, 0]), scene_groups(torch.tensor([0, 0])))
    with pytest.raises(ValueError):
        collision_loss(torch.zeros(3, 71, 3), torch.ones(3, 3), groups, BodySpheres([], [], [], []))
    with pytest.raises(ValueError):
        collision_loss(torch.zeros(3, 71, 3), torch.ones(3, 3), groups, ([0], [1], [0.5], [0.1]))


def test_fitter_scene_arguments():
    from romp_amd.fitting import KeypointFitter
    from romp_amd.smpl import SMPL
    from romp_amd.synthetic import make_smpl_model
    smpl = SMPL(make_smpl_model())
    f = KeypointFitter(smpl)
    assert (f.w_depth_order, f.depth_loss_type, f.dist_thresh, f.w_collision, f.spheres, f.scene_on) == (0., 'piecewise', 0.3, 0., None, False)
    assert KeypointFitter(smpl, w_depth_order=0.5, depth_loss_type='Log').scene_on and KeypointFitter(smpl, w_collision=2.).scene_on
    for bad in (dict(w_depth_order=-1.), dict(w_collision=-1.), dict(dist_thresh=-0.1), dict(depth_loss_type='linear')):
        with pytest.raises(ValueError):
            KeypointFitter(smpl, **bad)
    import inspect
    fit = inspect.signature(KeypointFitter.fit).parameters
    assert [fit[k].default for k in ('scene', 'depth_ids', 'radius_scale')] == [None, None, None]
