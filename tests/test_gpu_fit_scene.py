"""Scene terms on the GPU (run with -m gpu): romp_fit_scene (csrc/fit_scene.hip), romp_amd.scene and the scene arguments of
KeypointFitter on top of it, against the float64 CPU restatements of tests/test_fit_scene.py.

Tolerance: the rule of tests/test_gpu_fit.py, unchanged.  error = max |delta| / max |float64 reference| per tensor; every case
also evaluates the restatement in float32 on the CPU and requires  err_HIP <= 8 * max(err_CPU_f32, FLOOR),  FLOOR = 4 * 2^-24.
Every figure is printed before it is asserted (pytest -s).  Output buffers start as NaN, so an unwritten element shows.
Every table entry of these cases is in range: the bounds tests of the kernel are judged by reading them (scene_group and
scene_member at the top of fit_scene.hip), as for the link tables of the clip terms.

fit_scene_kernel gives a workgroup of 256 threads to each row.  Depth: the threads stride over the P x P pair space of the
scene and over the row's P - 1 partners, so P = 1 (no pair), 2, 3, 24 (276 pairs: the second round of the workgroup) and 65
(the second round of a wave's partners) take every path.  Collision: a lane owns a sphere, so S = 1, 2, 46, 64 are one lane,
two, part of a wave and a full one; the partners are split over four waves, so scenes of 1, 2, 3 and 9 rows give no partner,
one wave busy, two, and the third round of every wave."""
import math

import numpy as np
import pytest
import torch

from test_fit import project_torch
from test_fit_scene import (collision_torch, depth_order_torch, fit_scene_loop_torch, scenes_of, tables_of, translation_torch)
from test_gpu_fit import FLOOR, J, PAD, layer, stand_in, synthetic_outputs, within
from test_smpl_grad import smpl_torch

pytestmark = pytest.mark.gpu
F32 = lambda v: float(np.float32(v))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def nan_like(dev, *shape):
    return torch.full(shape, float('nan'), device=dev, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ the two sides
def cpu_scene(c, dtype):
    """-> loss (N,2), grad_joints (N,J,3), grad_cam (N,3) in float64: the objective of the header built from depth_order_torch
    and collision_torch, its gradient by autograd.  c: a case dict (see `case`)."""
    joints, cam = c['joints'].to(dtype).clone().requires_grad_(True), c['cam'].to(dtype).clone().requires_grad_(True)
    N = cam.shape[0]
    tw = torch.ones(N, dtype=dtype) if c.get('term_w') is None else c['term_w'].to(dtype)
    zeros = torch.zeros(N, dtype=dtype)
    dep = depth_order_torch(translation_torch(cam, c['camera'], dtype)[:, 2], c['ids'], c['off'], c['mem'], F32(c['thresh']), c['kind'], dtype) \
        if c.get('ids') is not None else zeros
    col = collision_torch(joints, cam, c['off'], c['mem'], c['spheres'], c.get('scale'), c['camera'], dtype) if c.get('spheres') else zeros
    total = (tw * (F32(c['w_depth']) * dep + F32(c['w_col']) * col)).sum()
    if total.requires_grad:
        total.backward()
    gj = torch.zeros_like(joints) if joints.grad is None else joints.grad
    gc = torch.zeros_like(cam) if cam.grad is None else cam.grad
    return torch.stack([dep.detach(), col.detach()], 1).double(), gj.double(), gc.double()


def hip_scene(dev, c, old_gj=None, old_gc=None, history_rows=0, row=0, with_loss=True):
    """The C entry on buffers filled with NaN (or on `old` gradients with accumulate = 1).  -> loss, gj, gc, history."""
    from romp_amd import fitting as F
    from romp_amd.scene import KINDS, BodySpheres
    d = lambda t: None if t is None else t.to(dev).contiguous()
    N = c['cam'].shape[0]
    table = BodySpheres(*c['spheres']).table() if c.get('spheres') else None
    joints, cam = d(c['joints'].float()), d(c['cam'].float())
    gj = nan_like(dev, *joints.shape) if old_gj is None else old_gj.to(dev).clone()
    gc = nan_like(dev, N, 3) if old_gc is None else old_gc.to(dev).clone()
    loss = nan_like(dev, N, 2) if with_loss else None
    hist = nan_like(dev, history_rows, N, 2) if history_rows else None
    ids = None if c.get('ids') is None else d(c['ids'].to(torch.int32))
    F._fit_scene(joints if table is not None else None, cam, F.CAMERAS[c['camera']], (d(c['off']), d(c['mem'])), ids, c['w_depth'], c['thresh'],
                 KINDS[c['kind']], table, d(c.get('scale')), c['w_col'], d(c.get('term_w')), gj if table is not None else None,
                 int(old_gj is not None), gc, int(old_gc is not None), loss, hist, row)
    torch.cuda.synchronize()
    return loss, gj, gc, hist


def holds(tag, name, hip, f32, ref):
    """`within`, and where the reference is all zeros (no partner, no active pair) exact zeros instead of a ratio."""
    if float(ref.abs().max()) == 0.:
        print(f'{tag} {name}: the reference is exactly zero')
        return hip.shape == ref.shape and bool((hip == 0).all())
    return within(tag, name, hip, f32, ref)


def check(dev, tag, c):
    ref, f32 = cpu_scene(c, torch.float64), cpu_scene(c, torch.float32)
    loss, gj, gc, _ = hip_scene(dev, c)
    ok = [holds(tag, 'loss', loss, f32[0], ref[0]), holds(tag, 'grad_cam', gc, f32[2], ref[2])]
    if c.get('spheres'):
        ok.append(holds(tag, 'grad_joints', gj, f32[1], ref[1]))
    else:
        assert bool(torch.isnan(gj).all()), 'without spheres grad_joints is not touched'
    assert bool((loss.cpu()[ref[0] == 0] == 0).all())             # a term without a partner or an active pair is exactly zero
    assert all(ok)
    return loss, gj, gc, ref


def cams(N, camera, g, spread=0.1):
    """Cameras whose translations lie within a few `spread` of each other.  weak: s in [0.1, 2] when spread is None."""
    if camera == 'perspective':
        return torch.tensor([0.1, -0.2, 3.0]) + spread * torch.randn(N, 3, generator=g)
    if spread is None:
        return torch.cat([0.1 + 1.9 * torch.rand(N, 1, generator=g), 0.2 * torch.randn(N, 2, generator=g)], 1)
    return torch.cat([0.8 + 0.04 * spread * torch.randn(N, 1, generator=g), 0.4 * spread * torch.randn(N, 2, generator=g)], 1)


def case(scenes, N, camera, seed, depth=True, S=0, kind='piecewise', thresh=0.3, scale=False, wide=False):
    """A case dict: joints (N,71,3), cam (N,3), the tables of `scenes`, depth ids in -1..3 and a seeded sphere table."""
    g = torch.Generator().manual_seed(seed)
    off, mem = tables_of(scenes, N)
    c = dict(joints=0.1 * torch.randn(N, J, 3, generator=g), camera=camera, off=off, mem=mem, kind=kind, thresh=thresh, w_depth=0.7,
             w_col=1.3, cam=cams(N, camera, g, None if wide else 0.1))
    if depth:
        c['ids'] = torch.randint(-1, 4, (N,), generator=g)
    if S:
        p, q = torch.randint(0, J, (S,), generator=g).tolist(), torch.randint(0, J, (S,), generator=g).tolist()
        q[0] = p[0]                                                # p == q is allowed
        c['spheres'] = (p, q, [(0., 0.5, 1.)[s % 3] for s in range(S)], (0.2 + 0.2 * torch.rand(S, generator=g)).tolist())
    if scale:
        c['scale'] = 0.5 + torch.rand(N, generator=g)
    return c


# ------------------------------------------------------------------------------------------------ depth order
@pytest.mark.parametrize('camera', ['perspective', 'weak'])
@pytest.mark.parametrize('kind', ['piecewise', 'log'])
@pytest.mark.parametrize('P', [1, 2, 3, 24, 65])
def test_depth_order(dev, P, kind, camera):
    """A scene of P rows behind a scene of two, an empty group between them, and two rows in no scene; ids in -1..3, so some
    rows are unlabelled.  weak: s in [0.1, 2], z = 2 / s in [1, 20]; perspective: z = 3 +- 0.1, inside the margin."""
    N = P + 4
    scenes = [[0, 1], [], list(range(2, P + 2))]
    c = case(scenes, N, camera, 100 * P + 7, kind=kind, wide=camera == 'weak')
    c['ids'][0], c['ids'][1] = 1, 0
    if P >= 3:
        c['ids'][2], c['ids'][3], c['ids'][4] = 2, -1, 0             # a labelled, an unlabelled and a third row for certain
    loss, _, gc, ref = check(dev, f'depth P={P} {kind} {camera}', c)
    assert bool((loss[-2:] == 0).all()) and bool((gc[-2:] == 0).all())                # in no scene: nothing
    assert bool((loss.cpu()[c['ids'] < 0] == 0).all()) and bool((gc.cpu()[c['ids'] < 0] == 0).all())
    if P >= 3 or kind == 'log':
        assert float(ref[0][:, 0].max()) > 0


def test_depth_margins_hit_exactly(dev):
    """thresh = 0.25 and depths that are multiples of 0.25: d - k thresh == 0 is exact in float32 and float64 alike, and such a
    pair must be inactive.  Scene 0: ids (0, 1) at z (1, 1.25), the margin exactly: no active pair, A == 0, zeros.  Scene 1:
    the same a quarter closer: active.  Scene 2: ten rows on the grid, against the restatement.  Scene 3: right order, A == 0."""
    g = torch.Generator().manual_seed(31)
    scenes = [[0, 1], [2, 3], list(range(4, 14)), [14, 15, 16]]
    c = case(scenes, 17, 'perspective', 32, thresh=0.25)
    c['cam'][:, 2] = 0.25 * torch.randint(4, 12, (17,), generator=g).float()
    c['ids'] = torch.randint(0, 4, (17,), generator=g)
    c['cam'][0, 2], c['cam'][1, 2], c['cam'][2, 2], c['cam'][3, 2] = 1., 1.25, 1., 1.
    c['ids'][:4] = torch.tensor([0, 1, 0, 1])
    c['cam'][14:, 2], c['ids'][14:] = torch.tensor([1., 3., 5.]), torch.tensor([0, 1, 2])
    on_margin = sum(1 for i in range(4, 14) for j in range(i + 1, 14) if c['ids'][j] != c['ids'][i] and
                    float(c['cam'][j, 2] - c['cam'][i, 2]) == 0.25 * float(c['ids'][j] - c['ids'][i]))
    assert on_margin >= 2, on_margin                               # the grid scene holds such pairs too
    loss, _, gc, ref = check(dev, 'depth margins', c)
    assert bool((loss[[0, 1, 14, 15, 16]] == 0).all()) and bool((gc[[0, 1, 14, 15, 16]] == 0).all())
    assert float(loss[2, 0]) > 0 and float(ref[0][4:14, 0].min()) > 0


# ------------------------------------------------------------------------------------------------ collision
LAYOUT = [[0], [1, 2], [3, 4, 5], [], list(range(6, 15))]            # scenes of 1, 2, 3 and 9 rows; row 15 is in none


@pytest.mark.parametrize('camera', ['perspective', 'weak'])
@pytest.mark.parametrize('S', [1, 2, 46, 64])
def test_collision(dev, S, camera):
    c = case(LAYOUT, 16, camera, 200 + S, depth=False, S=S, scale=S in (2, 64))
    assert set(c['spheres'][2][:3]) <= {0., 0.5, 1.} and c['spheres'][0][0] == c['spheres'][1][0]
    loss, gj, gc, ref = check(dev, f'collision S={S} {camera}', c)
    assert bool((loss[[0, 15]] == 0).all()) and bool((gj[[0, 15]] == 0).all()) and bool((gc[[0, 15]] == 0).all())   # alone; in no scene
    assert float(ref[0][1:15, 1].min()) > 1e-6                       # every other row overlaps a partner
    used = set(c['spheres'][0]) | set(c['spheres'][1])
    rest = [j for j in range(J) if j not in used]
    assert bool((gj[:, rest] == 0).all()), 'a joint without a sphere has a gradient'


def test_collision_coincident_and_far(dev):
    """One sphere on joint 0.  Rows 0 and 1 are the same person twice: the term is exp(0) = 1, half to each, and the
    gradient exactly zero.  Rows 2 and 3 stand 50 m apart: exp(-2500 / 0.02) underflows to zero; everything stays finite."""
    joints = 0.1 * torch.randn(1, J, 3, generator=torch.Generator().manual_seed(41)).repeat(4, 1, 1)
    cam = torch.tensor([[0.1, -0.2, 3.], [0.1, -0.2, 3.], [0., 0., 3.], [0., 0., 53.]])
    off, mem = tables_of([[0, 1], [2, 3]], 4)
    c = dict(joints=joints, cam=cam, camera='perspective', off=off, mem=mem, kind='piecewise', thresh=0.3, w_depth=0., w_col=2.,
             spheres=([0], [0], [0.], [0.3]))
    loss, gj, gc, _ = hip_scene(dev, c)
    assert loss.cpu().tolist() == [[0., 0.5], [0., 0.5], [0., 0.], [0., 0.]]
    assert bool((gj == 0).all()) and bool((gc == 0).all())


# ------------------------------------------------------------------------------------------------ both terms
def both(camera, seed=300, **kw):
    return case(LAYOUT, 16, camera, seed, S=46, scale=True, **kw)


@pytest.mark.parametrize('camera', ['perspective', 'weak'])
def test_both_terms_accumulate_term_w_and_history(dev, camera):
    c = both(camera, kind='log')
    g = torch.Generator().manual_seed(301)
    c['term_w'] = 0.5 + torch.rand(16, generator=g)
    ref, f32 = cpu_scene(c, torch.float64), cpu_scene(c, torch.float32)
    loss, gj, gc, hist = hip_scene(dev, c, history_rows=3, row=2)
    tag = f'both {camera} term_w'
    assert all([holds(tag, 'loss', loss, f32[0], ref[0]), holds(tag, 'grad_joints', gj, f32[1], ref[1]), holds(tag, 'grad_cam', gc, f32[2], ref[2])])
    assert float(ref[0][:, 0].max()) > 0 and float(ref[0][:, 1].max()) > 0
    assert torch.equal(hist[2], loss) and bool(torch.isnan(hist[:2]).all())
    old_j, old_c = torch.randn(16, J, 3, generator=g), torch.randn(16, 3, generator=g)
    for acc_j, acc_c in ((1, 0), (0, 1), (1, 1)):
        _, aj, ac, _ = hip_scene(dev, c, old_j if acc_j else None, old_c if acc_c else None)
        want_j = (old_j.double() + gj.cpu().double()).float() if acc_j else gj.cpu()
        want_c = (old_c.double() + gc.cpu().double()).float() if acc_c else gc.cpu()
        # float(double(old) + g) with g the float64 gradient: within one rounding of adding the stored float32 gradient
        assert float((aj.cpu() - want_j).abs().max()) <= 2.0 ** -23 * float(want_j.abs().max()), (acc_j, acc_c)
        assert float((ac.cpu() - want_c).abs().max()) <= 2.0 ** -23 * float(want_c.abs().max()), (acc_j, acc_c)
    nl, nj, ncam, _ = hip_scene(dev, c, with_loss=False)             # the backward launch of the nodes: gradients alone
    assert nl is None and torch.equal(nj, gj) and torch.equal(ncam, gc)


def test_a_nan_stays_in_its_scene(dev):
    c = both('perspective', kind='log')
    c['ids'] = torch.randint(0, 4, (16,), generator=torch.Generator().manual_seed(302))
    clean = hip_scene(dev, c)
    c['cam'] = c['cam'].clone()
    c['cam'][4, 2] = float('nan')                                    # row 4 of the scene 3, 4, 5
    dirty = hip_scene(dev, c)
    rest = [n for n in range(16) if n not in (3, 4, 5)]
    for a, b in zip(clean[:3], dirty[:3]):
        assert torch.equal(a[rest], b[rest])
    assert bool(torch.isnan(dirty[0][[3, 4, 5]]).all()) and bool(torch.isnan(dirty[2][[3, 4, 5]]).any(1).all())
    assert bool(torch.isfinite(clean[0]).all())


def test_two_calls_give_equal_bits(dev):
    for camera in ('perspective', 'weak'):
        c = both(camera)
        a, b = hip_scene(dev, c), hip_scene(dev, c)
        for x, y in zip(a[:3], b[:3]):
            assert torch.equal(x, y) and bool(torch.isfinite(x).all())


# ------------------------------------------------------------------------------------------------ the autograd nodes
@pytest.mark.parametrize('camera', [None, 'perspective', 'weak'])
def test_depth_order_loss_node(dev, camera):
    from romp_amd.scene import depth_order_loss
    c = case(LAYOUT, 16, camera or 'perspective', 400, kind='log')
    g = torch.Generator().manual_seed(401)
    w = 0.5 + torch.rand(16, generator=g)
    thresh = F32(0.3)

    def cpu(dtype):
        x = (c['cam'][:, 2] if camera is None else c['cam']).to(dtype).clone().requires_grad_(True)
        z = x if camera is None else translation_torch(x, camera, dtype)[:, 2]
        loss = depth_order_torch(z, c['ids'], c['off'], c['mem'], thresh, 'log', dtype)
        (w.to(dtype) * loss).sum().backward()
        return loss.detach().double(), x.grad.double()

    ref, f32 = cpu(torch.float64), cpu(torch.float32)
    x = (c['cam'][:, 2] if camera is None else c['cam']).to(dev).clone().requires_grad_(True)
    loss = depth_order_loss(x, c['ids'].to(dev), (c['off'].to(dev), c['mem'].to(dev)), dist_thresh=0.3, kind='log', camera=camera)
    (w.to(dev) * loss).sum().backward()
    torch.cuda.synchronize()
    tag = f'depth_order_loss {camera}'
    assert all([within(tag, 'loss', loss.detach(), f32[0], ref[0]), within(tag, 'grad', x.grad, f32[1], ref[1])])


@pytest.mark.parametrize('camera', ['perspective', 'weak'])
def test_collision_loss_node(dev, camera):
    from romp_amd.scene import BodySpheres, collision_loss
    c = case(LAYOUT, 16, camera, 410, depth=False, S=46, scale=True)
    w = 0.5 + torch.rand(16, generator=torch.Generator().manual_seed(411))

    def cpu(dtype):
        j, cam = c['joints'].to(dtype).clone().requires_grad_(True), c['cam'].to(dtype).clone().requires_grad_(True)
        loss = collision_torch(j, cam, c['off'], c['mem'], c['spheres'], c['scale'], camera, dtype)
        (w.to(dtype) * loss).sum().backward()
        return loss.detach().double(), j.grad.double(), cam.grad.double()

    ref, f32 = cpu(torch.float64), cpu(torch.float32)
    j, cam = c['joints'].to(dev).requires_grad_(True), c['cam'].to(dev).requires_grad_(True)
    loss = collision_loss(j, cam, (c['off'].to(dev), c['mem'].to(dev)), BodySpheres(*c['spheres']), c['scale'].to(dev), camera)
    (w.to(dev) * loss).sum().backward()
    torch.cuda.synchronize()
    tag = f'collision_loss {camera}'
    assert all([within(tag, 'loss', loss.detach(), f32[0], ref[0]), within(tag, 'grad_joints', j.grad, f32[1], ref[1]),
                within(tag, 'grad_cam', cam.grad, f32[2], ref[2])])


# ------------------------------------------------------------------------------------------------ KeypointFitter with scenes
FRAMES = (1, 2, 3)                                                   # persons per frame


def scene_case(model, camera, root_align, seed):
    """3 frames x (1, 2, 3) persons in frame-major order.  The persons of a frame start within a few centimetres of each other
    (they overlap), with depth labels in the REVERSE of their start order (every labelled pair is violated); the keypoints
    are the projection of the start plus a little noise.  -> dict of float32 tensors."""
    from romp_amd.scene import scene_groups
    g = torch.Generator().manual_seed(seed)
    N = sum(FRAMES)
    frame = torch.tensor([f for f, n in enumerate(FRAMES) for _ in range(n)])
    b0, p0 = 0.5 * torch.randn(N, 10, generator=g), 0.2 * torch.randn(N, 72, generator=g)
    c0 = cams(N, camera, g, 0.03)
    z = translation_torch(c0, camera)[:, 2]
    ids = torch.zeros(N, dtype=torch.int64)
    for f in range(len(FRAMES)):
        rows = torch.nonzero(frame == f).squeeze(1)
        ids[rows[torch.argsort(z[rows], descending=True)]] = torch.arange(len(rows))       # the deepest row gets the front label
    _, jt = smpl_torch(model, b0, p0, root_align, torch.float64)
    kp = (project_torch(jt, c0, camera) + 0.005 * torch.randn(N, J, 2, generator=g).double()).float()
    conf = 0.2 + 0.8 * torch.rand(N, J, generator=g)
    return dict(b0=b0, p0=p0, c0=c0, kp=kp, conf=conf, ids=ids, groups=scene_groups(frame))


# the weights bring the two terms' gradients to the same order: the start's collision energy is about 1000, the depth term about 1
TERMS = {'depth': dict(w_depth_order=2.), 'collision': dict(w_collision=1e-4), 'both': dict(w_depth_order=2., w_collision=1e-4)}
FIT_KEYS = ('betas', 'poses', 'cam', 'loss_history', 'scene_history')


@pytest.mark.parametrize('terms', ['depth', 'collision', 'both'])
@pytest.mark.parametrize('camera,root_align', [('perspective', True), ('weak', False)])   # the BEV and the ROMP stand-in
def test_five_steps_with_scene_terms_equal_the_float64_loop(dev, camera, root_align, terms):
    from romp_amd.fitting import KeypointFitter
    from romp_amd.scene import body_spheres
    model, smpl = layer(dev)
    c = scene_case(model, camera, root_align, 500)
    sp = body_spheres(smpl)
    args = dict(steps=5, lr=0.01, sigma=0.05, w_betas=1e-3, w_pose=2e-3, depth_loss_type='piecewise', dist_thresh=0.3, **TERMS[terms])
    loop = lambda dtype: fit_scene_loop_torch(model, c['b0'], c['p0'], c['c0'], c['groups'], c['kp'], c['conf'], c['ids'], camera=camera,
                                              root_align=root_align, spheres=(sp.p, sp.q, sp.a, sp.r), dtype=dtype, **args)
    want, f32 = loop(torch.float64), loop(torch.float32)
    # the case is meaningful, by the float64 loop alone: a label is violated, two persons overlap, each term falls
    first, last = want['scene_history'][0].sum(0), want['scene_history'][-1].sum(0)
    print(f'scene fitter {camera} {terms}: float64 loop, (depth, collision) summed over the rows: first {first.tolist()} last {last.tolist()}')
    if 'w_depth_order' in args:
        assert float(first[0]) > 0 and float(last[0]) < float(first[0])
    if 'w_collision' in args:
        assert float(want['scene_history'][0, :, 1].max()) > 0.1 and float(last[1]) < float(first[1])
    got = KeypointFitter(smpl, camera=camera, root_align=root_align, **args).fit(c['b0'], c['p0'], c['c0'], c['kp'], c['conf'], scene=c['groups'],
                                                                                depth_ids=c['ids'])
    torch.cuda.synchronize()
    N = sum(FRAMES)
    assert got['loss_history'].shape == (6, N) and got['scene_history'].shape == (6, N, 2) and got['scene_history'].is_cuda
    ok = [holds(f'scene fitter {camera} {terms}', k, got[k], f32[k], want[k]) for k in FIT_KEYS]
    off = 1 if terms == 'depth' else 0 if terms == 'collision' else None
    if off is not None:
        assert bool((got['scene_history'][:, :, off] == 0).all())   # the term that is off
    assert bool((got['scene_history'][:, 0] == 0).all())             # the lone person of frame 0
    v, j, _ = smpl(got['betas'], got['poses'], root_align=root_align)
    assert torch.equal(v, got['verts']) and torch.equal(j, got['joints'])
    assert all(ok)


@pytest.mark.parametrize('camera,root_align', [('perspective', True), ('weak', False)])
def test_with_the_defaults_the_fitter_is_the_old_fitter(dev, camera, root_align):
    from romp_amd.fitting import KeypointFitter
    model, smpl = layer(dev)
    c = scene_case(model, camera, root_align, 510)
    old = KeypointFitter(smpl, camera=camera, root_align=root_align, steps=3).fit(c['b0'], c['p0'], c['c0'], c['kp'], c['conf'])
    for fitter, kw in ((KeypointFitter(smpl, camera=camera, root_align=root_align, steps=3, **TERMS['both']), dict(scene=None, depth_ids=c['ids'])),
                       (KeypointFitter(smpl, camera=camera, root_align=root_align, steps=3), dict(scene=c['groups'], depth_ids=c['ids'])),
                       (KeypointFitter(smpl, camera=camera, root_align=root_align, steps=3, w_depth_order=1.), dict(scene=c['groups']))):
        run = fitter.start(c['b0'], c['p0'], c['c0'], c['kp'], c['conf'], **kw)
        assert run.evaluate == run._evaluate_2d and run.update == run._update_2d      # the fast path, launch for launch
        new = fitter.fit(c['b0'], c['p0'], c['c0'], c['kp'], c['conf'], **kw)
        assert set(new) == set(old) == {'betas', 'poses', 'cam', 'verts', 'joints', 'loss_history'}
        for k in old:
            assert torch.equal(new[k], old[k]), k


# ------------------------------------------------------------------------------------------------ refine_scene
@pytest.mark.parametrize('kind', ['romp', 'bev'])
def test_refine_scene(dev, kind):
    """synthetic_outputs read as three persons of one image, moved to within a few centimetres of each other, with depth labels
    against their order.  ROMP: one fit of three rows.  BEV: the middle row is an infant on the SMIL layer; the adults are
    fitted with the infant as a fixed row and the infant against the fitted adults, so every row still has both terms.  The
    first row of scene_history is the terms of the start, which the nodes give directly."""
    from romp_amd.fitting import refine_outputs
    from romp_amd.scene import body_spheres, collision_loss, depth_order_loss, refine_scene, scene_groups
    model = stand_in(dev, kind)
    out = dict(synthetic_outputs(dev, model, kind))
    cam_key, camera = ('cam', 'weak') if kind == 'romp' else ('cam_trans', 'perspective')
    out[cam_key] = torch.tensor([[0.9, 0.05, -0.03], [0.89, 0.06, -0.02], [0.91, 0.04, -0.04]] if kind == 'romp' else
                                [[0.1, -0.2, 3.0], [0.12, -0.18, 3.05], [0.08, -0.22, 2.95]], device=dev)
    ids = torch.tensor([1, 0, 2])                                    # romp: z = 2 / s = 2.22, 2.25, 2.20; bev: 3.0, 3.05, 2.95
    frames = torch.zeros(3, dtype=torch.int64)
    start = refine_outputs(model, out, out['pj2d_org'], pad_info=PAD, steps=0)        # the projection of the moved persons
    shifted = start['pj2d_org'] + 8.
    args = dict(pad_info=PAD, steps=5, lr=0.01)
    plain = refine_outputs(model, out, shifted, **args)
    res = refine_scene(model, out, frames, shifted, depth_ids=ids, w_depth_order=2., w_collision=1e-4, **args)
    torch.cuda.synchronize()
    assert 'scene_history' not in plain and res['scene_history'].shape == (6, 3, 2) and res['fit_loss'].shape == (3, 2)
    hist = res['scene_history'].cpu()
    assert bool(torch.isfinite(hist).all()) and bool((hist[0] > 0).all())             # every row has both terms, the infant too
    groups = scene_groups(frames.to(dev))
    depth = depth_order_loss(out[cam_key], ids.to(dev), groups, camera=camera).cpu()
    rows = [0, 1, 2] if kind == 'romp' else [0, 2]                   # the infant's first row is taken against the FITTED adults
    assert float((hist[0, rows, 0] - depth[rows]).abs().max()) <= 1e-5 * float(depth.max())
    parser = model.smpl_parser
    joints = out['joints'].float()
    if kind == 'romp':
        col = collision_loss(joints, out[cam_key], groups, body_spheres(parser.smpl_model), camera=camera).cpu()
        assert float((hist[0, :, 1] - col).abs().max()) <= 1e-5 * float(col.max())
        verts, jn, _ = parser.smpl_model(res['smpl_betas'], res['smpl_thetas'])
        assert torch.equal(verts, res['verts']) and torch.equal(jn, res['joints'])
    else:                                                            # the adults' rows: their own layer's table, the infant fixed
        col = collision_loss(joints, out[cam_key], groups, body_spheres(parser.smpl_model), camera=camera).cpu()
        assert float((hist[0, [0, 2], 1] - col[[0, 2]]).abs().max()) <= 1e-5 * float(col.max())
        verts, jn, _ = parser(res['smpl_betas'], res['smpl_thetas'])
        assert torch.equal(verts, res['verts']) and torch.equal(jn, res['joints'])
    assert not torch.equal(res[cam_key], plain[cam_key])
    assert float(hist[-1, :, 0].sum()) < float(hist[0, :, 0].sum())                   # the depths moved towards their order
    off = refine_scene(model, out, frames, shifted, depth_ids=ids, **args)            # no weight: refine_outputs, bit for bit
    for k in ('smpl_betas', 'smpl_thetas', cam_key, 'verts', 'joints', 'fit_loss'):
        assert torch.equal(off[k], plain[k]), k
    assert 'scene_history' not in off
