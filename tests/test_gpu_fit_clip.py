"""Temporal smoothness terms and the acceleration metric on the GPU (run with -m gpu): romp_fit_temporal and romp_clip_accel
(csrc/fit_clip.hip), romp_amd.clip, the links of KeypointFitter and romp_amd.evaluation.accel on top of them, against the
float64 CPU restatements of tests/test_fit_clip.py.

Tolerance: the rule of tests/test_gpu_fit.py, unchanged.  error = max |delta| / max |float64 reference| per tensor; every case
also evaluates the restatement in float32 on the CPU and requires  err_HIP <= 8 * max(err_CPU_f32, FLOOR),  FLOOR = 4 * 2^-24.
Every figure is printed before it is asserted (pytest -s).  Output buffers start as NaN, so an unwritten element shows.

Input conditions, asserted on the CPU in float64 before the device is touched: |theta| <= pi; every link of a case that is
not meant to be static has e >= 1e-6 in every term; in the Geman-McClure cases e / sigma^2 lies in [0.1, 10] for every link,
so that both branches of rho matter.  `motion` builds such data: along every chain a row is its predecessor plus a step of
length 1.5 +- (0.5 .. 0.6), the sign alternating, in a random direction, so |v|^2 lies in [0.8, 4.5] and |a|^2 in [1, 10.3].

fit_temporal_kernel gives a wave to each (row, block), four to a workgroup: N x blocks = 3, 4, 5 are a lone partial workgroup,
a full one and one more.  A lane strides over the columns by 64: cols = 1, 3, 63, 64, 65, 213 are one lane, part of a wave,
the last lane short, a full wave, the second round and the joints segment of the fitter.  One chain of N = 1 has no link, 2 a
velocity term, 3 the first acceleration term, 5 the first row with the full five-term stencil."""
import math

import numpy as np
import pytest
import torch

from make_golden_clip import inputs as accel_inputs
from test_fit import project_torch
from test_fit_clip import (accel_np, chain, fit_clip_loop_torch, links_of, rotation_smooth_torch, temporal_torch)
from test_gpu_fit import FLOOR, J, PAD, layer, stand_in, synthetic_outputs, within
from test_smpl_grad import smpl_torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def nan_like(dev, *shape):
    return torch.full(shape, float('nan'), device=dev, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ link tables
def tables(name):
    """-> (prev, next) int32 tensors.  Every entry is in range: the bounds test of the kernel is checked by reading it."""
    if name == 'interleaved':                                    # two tracks of five frames, frame-major
        prev = [-1, -1] + list(range(8))
        nxt = list(range(2, 10)) + [-1, -1]
    elif name == 'shuffled':                                     # one chain through a seeded permutation of nine rows
        order = torch.randperm(9, generator=torch.Generator().manual_seed(21)).tolist()
        prev, nxt = [-1] * 9, [-1] * 9
        for a, b in zip(order[:-1], order[1:]):
            nxt[a], prev[b] = b, a
    elif name == 'singleton':                                    # row 2 stands alone between the rows of a chain of six
        rows = [0, 1, 3, 4, 5, 6]
        prev, nxt = [-1] * 7, [-1] * 7
        for a, b in zip(rows[:-1], rows[1:]):
            nxt[a], prev[b] = b, a
    elif name == 'cut':                                          # 0 -> 1 -> 2 -> 3 and 4 -> 5 -> 6 -> 7 -> 8
        prev, nxt = chain(9)
        prev, nxt = prev.tolist(), nxt.tolist()
        nxt[3], prev[4] = -1, -1
    elif name == 'next_disagrees':                               # next[3] names row 6, not 4: no link 3 -> 4, rows 4.. go on
        prev, nxt = chain(9)
        prev, nxt = prev.tolist(), nxt.tolist()
        nxt[3] = 6
    elif name == 'prev_is_self':                                 # prev[4] == 4: no link into row 4
        prev, nxt = chain(9)
        prev, nxt = prev.tolist(), nxt.tolist()
        prev[4] = 4
    else:
        raise KeyError(name)
    return torch.tensor(prev, dtype=torch.int32), torch.tensor(nxt, dtype=torch.int32)


TABLES = ['interleaved', 'shuffled', 'singleton', 'cut', 'next_disagrees', 'prev_is_self']


def chains_of(prev, nxt):
    """The chains of a table under the link rule, each as the list of its rows in order."""
    pv, nx = links_of(prev, nxt)
    out = []
    for n in range(len(pv)):
        if pv[n] < 0:
            rows = [n]
            while nx[rows[-1]] >= 0:
                rows.append(nx[rows[-1]])
            out.append(rows)
    return out


def motion(prev, nxt, cols, seed, scale=1.):
    """x (N, cols) float32 as the module docstring describes it, times `scale`."""
    g = torch.Generator().manual_seed(seed)
    N = prev.numel()
    x = torch.zeros(N, cols, dtype=torch.float64)
    for rows in chains_of(prev, nxt):
        x[rows[0]] = torch.randn(cols, generator=g, dtype=torch.float64)
        for k, (a, b) in enumerate(zip(rows[:-1], rows[1:])):
            u = torch.randn(cols, generator=g, dtype=torch.float64)
            m = 1.5 + (-1) ** k * (0.5 + 0.1 * float(torch.rand(1, generator=g)))
            x[b] = x[a] + m * u / u.norm()
    return (scale * x).float()


def pose_motion(prev, nxt, seed):
    """poses (N,72) float32, |theta| <= pi: a base of 0.5 randn per chain, steps of 0.2 randn per row."""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(prev.numel(), 72)
    for rows in chains_of(prev, nxt):
        p[rows[0]] = 0.5 * torch.randn(72, generator=g)
        for a, b in zip(rows[:-1], rows[1:]):
            p[b] = p[a] + 0.2 * torch.randn(72, generator=g)
    p = p.clamp(-1.8, 1.8)                                       # |theta| <= sqrt(3) 1.8 < pi
    assert float(p.reshape(-1, 3).norm(dim=1).max()) <= math.pi
    return p


def linked(prev, nxt):
    pv, nx = links_of(prev, nxt)
    vel = torch.tensor([p >= 0 for p in pv], dtype=torch.bool)
    acc = torch.tensor([p >= 0 and x >= 0 for p, x in zip(pv, nx)], dtype=torch.bool)
    return vel, acc


def sigma_for(e):
    """A width with e / sigma^2 in [0.1, 10] for every entry of e: the root of the geometric middle of its range; asserted."""
    if e.numel() == 0:
        return 1.
    s2 = math.sqrt(float(e.min()) * float(e.max()))
    s = float(np.float32(math.sqrt(s2)))
    assert float(e.min()) >= 1e-6 and float(e.min()) / (s * s) >= 0.1 and float(e.max()) / (s * s) <= 10, (float(e.min()), float(e.max()), s)
    return s


def segment(prev, nxt, cols, seed, robust, with_w=True, w_vel=0.7, w_acc=1.3, scale=1.):
    """One linear block as a dict: x, col_w in [0.5, 1.5] or None, the weights and, when robust, widths by `sigma_for`."""
    x = motion(prev, nxt, cols, seed, scale)
    g = torch.Generator().manual_seed(seed + 1000)
    col_w = 0.5 + torch.rand(cols, generator=g) if with_w else None
    vel, acc = linked(prev, nxt)
    ev, ea = temporal_torch(x, prev, nxt, col_w)
    assert (not bool(vel.any()) or float(ev[vel].min()) >= 1e-6) and (not bool(acc.any()) or float(ea[acc].min()) >= 1e-6)
    return dict(x=x, col_w=col_w, w_vel=w_vel, w_acc=w_acc, sigma_vel=sigma_for(ev[vel]) if robust else 0.,
                sigma_acc=sigma_for(ea[acc]) if robust else 0.)


def rotation(prev, nxt, seed, robust, with_w=True, w_rot=0.9):
    poses = pose_motion(prev, nxt, seed)
    g = torch.Generator().manual_seed(seed + 2000)
    joint_w = 0.5 + torch.rand(24, generator=g) if with_w else None
    vel, _ = linked(prev, nxt)
    e = rotation_smooth_torch(poses, prev, nxt, joint_w)
    assert not bool(vel.any()) or float(e[vel].min()) >= 1e-6
    return dict(poses=poses, joint_w=joint_w, w_rot=w_rot, sigma_rot=sigma_for(e[vel]) if robust else 0.)


# ------------------------------------------------------------------------------------------------ the two sides
def cpu_temporal(segs, rot, prev, nxt, dtype, term_w=None):
    """-> loss (N, L) float64, [gradient per segment], gradient of the poses or None: the objective of the header built from
    temporal_torch and rotation_smooth_torch, its gradient by autograd."""
    xs = [s['x'].to(dtype).clone().requires_grad_(True) for s in segs]
    N = prev.numel()
    tw = torch.ones(N, dtype=dtype) if term_w is None else term_w.to(dtype)
    cols, total = [], torch.zeros((), dtype=dtype)
    for s, x in zip(segs, xs):
        v, a = temporal_torch(x, prev, nxt, s['col_w'], s['sigma_vel'], s['sigma_acc'], dtype)
        total = total + (tw * (float(np.float32(s['w_vel'])) * v + float(np.float32(s['w_acc'])) * a)).sum()
        cols += [v, a]
    p = None
    if rot is not None:
        p = rot['poses'].to(dtype).clone().requires_grad_(True)
        r = rotation_smooth_torch(p, prev, nxt, rot['joint_w'], rot['sigma_rot'], dtype)
        total = total + (tw * float(np.float32(rot['w_rot'])) * r).sum()
        cols.append(r)
    if total.requires_grad:
        total.backward()
    grads = [torch.zeros_like(x) if x.grad is None else x.grad for x in xs]
    gp = None if p is None else (torch.zeros_like(p) if p.grad is None else p.grad)
    return torch.stack([c.detach() for c in cols], 1).double(), [g.double() for g in grads], None if gp is None else gp.double()


def hip_temporal(dev, segs, rot, prev, nxt, old=None, old_p=None, history_rows=0, row=0, term_w=None):
    """The C entry on buffers filled with NaN (or on `old` gradients with accumulate = 1).  -> loss, [grads], gp, history."""
    from romp_amd import fitting as F
    from romp_amd import lib as L
    N = prev.numel()
    d = lambda t: None if t is None else t.to(dev).contiguous()
    keep, table, grads = [], [], []
    for i, s in enumerate(segs):
        x, w = d(s['x']), d(s['col_w'])
        g = nan_like(dev, *x.shape) if old is None else old[i].to(dev).clone()
        keep += [x, w]
        grads.append(g)
        table.append(F._clip_segment(x, g, w, s['w_vel'], s['w_acc'], s['sigma_vel'], s['sigma_acc'], int(old is not None)))
    L_cols = 2 * len(segs) + (rot is not None)
    loss = nan_like(dev, N, L_cols)
    hist = nan_like(dev, history_rows, N, L_cols) if history_rows else None
    poses = joint_w = gp = None
    if rot is not None:
        poses, joint_w = d(rot['poses']), d(rot['joint_w'])
        gp = nan_like(dev, N, 72) if old_p is None else old_p.to(dev).clone()
    F._temporal((L.ClipSegment * len(table))(*table) if table else None, (d(prev), d(nxt)), N, loss, poses, joint_w,
                0. if rot is None else rot['w_rot'], 0. if rot is None else rot['sigma_rot'], gp, int(old_p is not None), hist, row, d(term_w))
    torch.cuda.synchronize()
    return loss, grads, gp, hist


def holds(tag, name, hip, f32, ref):
    """`within`, and where the reference is all zeros (no link, a static chain) exact zeros instead of a ratio."""
    if float(ref.abs().max()) == 0.:
        print(f'{tag} {name}: the reference is exactly zero')
        return hip.shape == ref.shape and bool((hip == 0).all())
    return within(tag, name, hip, f32, ref)


def check(dev, tag, segs, rot, prev, nxt):
    ref, f32 = cpu_temporal(segs, rot, prev, nxt, torch.float64), cpu_temporal(segs, rot, prev, nxt, torch.float32)
    loss, grads, gp, _ = hip_temporal(dev, segs, rot, prev, nxt)
    ok = [holds(tag, 'loss', loss, f32[0], ref[0])]
    ok += [holds(tag, f'grad[{i}]', grads[i], f32[1][i], ref[1][i]) for i in range(len(segs))]
    if rot is not None:
        ok.append(holds(tag, 'grad_poses', gp, f32[2], ref[2]))
    vel, acc = linked(prev, nxt)                                  # a term without its links is exactly zero
    for i in range(len(segs)):
        assert bool((loss[:, 2 * i].cpu()[~vel] == 0).all()) and bool((loss[:, 2 * i + 1].cpu()[~acc] == 0).all())
    if rot is not None:
        assert bool((loss[:, -1].cpu()[~vel] == 0).all())
    assert all(ok)
    return loss, grads, gp


def blocks(config, prev, nxt, seed, robust):
    if config == 'rot':
        return [], rotation(prev, nxt, seed, robust)
    if config == 'one':
        return [segment(prev, nxt, 65, seed, robust)], None
    return [segment(prev, nxt, c, seed + i, robust, with_w=bool(i % 2), scale=s) for i, (c, s) in enumerate(((213, 0.05), (3, 1.), (10, 0.3), (1, 2.)))], \
        rotation(prev, nxt, seed + 9, robust, with_w=False)


# ------------------------------------------------------------------------------------------------ losses and gradients
@pytest.mark.parametrize('robust', [False, True])
@pytest.mark.parametrize('config', ['rot', 'one', 'four+rot'])        # n_segments = 0 with rotations only, 1, and 4 with rotations
@pytest.mark.parametrize('N', [1, 2, 3, 4, 5])                         # waves: N, N and 5 N -- 3, 4 and 5 among them
def test_one_chain(dev, N, config, robust):
    prev, nxt = chain(N)
    segs, rot = blocks(config, prev, nxt, 100 * N + 7, robust)
    check(dev, f'chain N={N} {config} robust={robust}', segs, rot, prev, nxt)


@pytest.mark.parametrize('with_w', [False, True])
@pytest.mark.parametrize('cols', [1, 3, 63, 64, 65, 213])
def test_columns(dev, cols, with_w):
    prev, nxt = chain(5)
    seg = segment(prev, nxt, cols, 300 + cols, robust=True, with_w=with_w)
    check(dev, f'cols={cols} col_w={with_w}', [seg], None, prev, nxt)
    if not with_w:                                               # NULL stands for ones
        a = hip_temporal(dev, [seg], None, prev, nxt)
        b = hip_temporal(dev, [dict(seg, col_w=torch.ones(cols))], None, prev, nxt)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0])


@pytest.mark.parametrize('robust', [False, True])
@pytest.mark.parametrize('name', TABLES)
def test_tables(dev, name, robust):
    prev, nxt = tables(name)
    N = prev.numel()
    assert int(prev.min()) >= -1 and int(prev.max()) < N and int(nxt.min()) >= -1 and int(nxt.max()) < N
    segs = [segment(prev, nxt, 213, 400, robust, scale=0.05), segment(prev, nxt, 3, 401, robust, with_w=False)]
    rot = rotation(prev, nxt, 402, robust)
    loss, grads, gp = check(dev, f'table {name} robust={robust}', segs, rot, prev, nxt)
    if name == 'next_disagrees':                                 # rows 3 and 4 are not neighbours: what 3 gets is what a cut gives it
        cut = tables('cut')
        other = hip_temporal(dev, segs, rot, *cut)
        assert torch.equal(loss, other[0]) and all(torch.equal(a, b) for a, b in zip(grads, other[1])) and torch.equal(gp, other[2])
    if name == 'singleton':
        assert bool((loss[2] == 0).all()) and bool((grads[0][2] == 0).all()) and bool((gp[2] == 0).all())


def test_weights_switch_terms_off(dev):
    """w_vel = 0 leaves the acceleration gradient alone and the other way round; the losses are unweighted either way."""
    prev, nxt = chain(5)
    seg = segment(prev, nxt, 65, 500, robust=True)
    both = hip_temporal(dev, [seg], None, prev, nxt)
    for off in ('w_vel', 'w_acc'):
        s = dict(seg, **{off: 0.})
        loss, _, _ = check(dev, f'{off} = 0', [s], None, prev, nxt)
        assert torch.equal(loss, both[0])


def test_accumulate_onto_old_gradients_and_the_history_row(dev):
    prev, nxt = tables('interleaved')
    N = prev.numel()
    segs = [segment(prev, nxt, 65, 600, True), segment(prev, nxt, 3, 601, False)]
    rot = rotation(prev, nxt, 602, True)
    g = torch.Generator().manual_seed(603)
    old, old_p = [torch.randn(N, 65, generator=g), torch.randn(N, 3, generator=g)], torch.randn(N, 72, generator=g)
    fresh = hip_temporal(dev, segs, rot, prev, nxt, history_rows=3, row=1)
    added = hip_temporal(dev, segs, rot, prev, nxt, old=old, old_p=old_p, history_rows=3, row=2)
    ref = cpu_temporal(segs, rot, prev, nxt, torch.float64)
    f32 = cpu_temporal(segs, rot, prev, nxt, torch.float32)
    ok = []
    for i, o in enumerate(old + [old_p]):
        got = added[1][i] if i < 2 else added[2]
        r, f = (ref[1][i], f32[1][i]) if i < 2 else (ref[2], f32[2])
        ok.append(within('accumulate', f'tensor {i}', got, (o + f.float()), o.double() + r))
    assert torch.equal(fresh[0], added[0])
    assert torch.equal(fresh[3][1], fresh[0]) and bool(torch.isnan(fresh[3][[0, 2]]).all())   # the row asked for, and nothing else
    assert torch.equal(added[3][2], added[0]) and bool(torch.isnan(added[3][:2]).all())
    assert all(ok)


def test_mixed_accumulate_flags(dev):
    """Each segment and the rotation block carry a flag of their own."""
    from romp_amd import fitting as F
    from romp_amd import lib as L
    prev, nxt = chain(5)
    a, b = segment(prev, nxt, 10, 610, False), segment(prev, nxt, 4, 611, False)
    fresh = hip_temporal(dev, [a, b], None, prev, nxt)
    xa, xb = a['x'].to(dev), b['x'].to(dev)
    wa, wb = a['col_w'].to(dev), b['col_w'].to(dev)
    ga, gb = torch.ones(5, 10, device=dev), torch.ones(5, 4, device=dev)
    table = (L.ClipSegment * 2)(F._clip_segment(xa, ga, wa, a['w_vel'], a['w_acc'], 0., 0., 1), F._clip_segment(xb, gb, wb, b['w_vel'], b['w_acc'], 0., 0., 0))
    F._temporal(table, (prev.to(dev), nxt.to(dev)), 5, nan_like(dev, 5, 4))
    torch.cuda.synchronize()
    # float(1 + g) against 1 + float(g): two roundings of numbers of size 1 + |g|
    assert float((ga - (1. + fresh[1][0])).abs().max()) <= 2.0 ** -22 * (1. + float(fresh[1][0].abs().max())) and torch.equal(gb, fresh[1][1])


def test_a_static_chain_is_exactly_zero(dev):
    prev, nxt = tables('interleaved')
    N = prev.numel()
    g = torch.Generator().manual_seed(620)
    for robust in (0., 0.5):
        segs = [dict(x=torch.randn(1, c, generator=g).expand(N, c).contiguous(), col_w=None, w_vel=1., w_acc=1., sigma_vel=robust,
                     sigma_acc=robust) for c in (213, 3)]
        rot = dict(poses=(0.5 * torch.randn(1, 72, generator=g)).expand(N, 72).contiguous(), joint_w=None, w_rot=1., sigma_rot=robust)
        loss, grads, gp, _ = hip_temporal(dev, segs, rot, prev, nxt)
        for t in [loss, gp] + grads:
            assert bool((t == 0).all())


def test_rotation_edges(dev):
    """One chain of six: row 1 repeats row 0 (a static link: its term is exactly zero); row 2 differs from it by 1e-4 rad in
    one joint; row 3 is the all-zero pose; rows 4 and 5 hold a joint at |theta| = 3.1 about opposite axes, the same rotation up
    to 0.083 rad: the term there is 4 (1 - cos 0.083) and not the 6.2^2 of a difference of vectors."""
    g = torch.Generator().manual_seed(630)
    poses = torch.zeros(6, 72)
    poses[0] = 0.4 * torch.randn(72, generator=g)
    poses[1] = poses[0]
    poses[2] = poses[1]
    poses[2, 30] += 1e-4
    poses[4] = 0.3 * torch.randn(72, generator=g)
    axis = torch.tensor([0.6, -0.48, 0.64])
    poses[4, 15:18] = 3.1 * axis
    poses[5] = poses[4]
    poses[5, 15:18] = -3.1 * axis
    assert float(poses.reshape(-1, 3).norm(dim=1).max()) <= math.pi
    prev, nxt = chain(6)
    for sigma in (0., 1.):
        rot = dict(poses=poses, joint_w=None, w_rot=1., sigma_rot=sigma)
        loss, _, gp = check(dev, f'rotation edges sigma={sigma}', [], rot, prev, nxt)
        loss = loss.cpu()[:, 0]
        assert float(loss[1]) == 0.
        e = 4 * (1 - math.cos(2 * math.pi - 6.2))
        print(f'rotation edges: loss {loss.tolist()}, 4 (1 - cos 0.083) = {e:.6g}')
        if sigma == 0.:
            # float32 storage of 3.1 * axis moves each of the two angles by <= 4e-7 rad: 2 * 1e-6 / 0.083 of e
            assert abs(float(loss[5]) - e) <= 1e-4 * e and 0 < float(loss[2]) <= 4.1e-8
        assert bool(torch.isfinite(gp).all())


def test_a_nan_row_reaches_two_links_and_no_other_chain(dev):
    prev, nxt = tables('interleaved')                            # track A: rows 0, 2, 4, 6, 8; track B: the odd rows
    N = prev.numel()
    segs = [segment(prev, nxt, 65, 640, True)]
    rot = rotation(prev, nxt, 641, True)
    clean = hip_temporal(dev, segs, rot, prev, nxt)
    bad_x, bad_p = segs[0]['x'].clone(), rot['poses'].clone()
    bad_x[0, 7] = float('nan')                                   # the first row of A: it reaches rows 2 and 4
    bad_p[0, 40] = float('nan')                                  # the rotations are first order: it reaches row 2
    loss, grads, gp, _ = hip_temporal(dev, [dict(segs[0], x=bad_x)], dict(rot, poses=bad_p), prev, nxt)
    nan_rows = lambda t: torch.isnan(t).reshape(N, -1).any(1).cpu().tolist()
    assert nan_rows(grads[0]) == [n in (0, 2, 4) for n in range(N)]
    assert nan_rows(gp) == [n in (0, 2) for n in range(N)]
    assert nan_rows(loss) == [n == 2 for n in range(N)]          # Lvel[2], Lacc[2], Lrot[2] read row 0; row 0 has no term of its own
    rest = [n for n in range(N) if n not in (0, 2, 4)]
    assert torch.equal(grads[0][rest], clean[1][0][rest]) and torch.equal(gp[rest], clean[2][rest]) and torch.equal(loss[rest], clean[0][rest])


def test_two_calls_on_a_side_stream_give_equal_bits(dev):
    prev, nxt = tables('shuffled')
    segs, rot = [segment(prev, nxt, 213, 650, True, scale=0.05)], rotation(prev, nxt, 651, True)
    want = hip_temporal(dev, segs, rot, prev, nxt)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        got = hip_temporal(dev, segs, rot, prev, nxt)
    s.synchronize()
    assert torch.equal(want[0], got[0]) and torch.equal(want[1][0], got[1][0]) and torch.equal(want[2], got[2])


# ------------------------------------------------------------------------------------------------ the autograd nodes
@pytest.mark.parametrize('order', [1, 2])
def test_temporal_loss_node(dev, order):
    """Against autograd of temporal_torch, with a different incoming gradient for every row: loss[n] reads its neighbours, so
    the backward is not a scaling of rows."""
    from romp_amd.clip import temporal_loss
    prev, nxt = tables('interleaved')
    N = prev.numel()
    seg = segment(prev, nxt, 65, 700 + order, True)
    sigma = seg['sigma_vel'] if order == 1 else seg['sigma_acc']
    weight = 0.5 + torch.rand(N, generator=torch.Generator().manual_seed(702))

    def cpu(dtype):
        x = seg['x'].to(dtype).clone().requires_grad_(True)
        loss = temporal_torch(x, prev, nxt, seg['col_w'], sigma, sigma, dtype)[order - 1]
        (loss * weight.to(dtype)).sum().backward()
        return loss.detach().double(), x.grad.double()

    ref, f32 = cpu(torch.float64), cpu(torch.float32)
    x = seg['x'].to(dev).requires_grad_(True)
    loss = temporal_loss(x, (prev.to(dev), nxt.to(dev)), order=order, col_w=seg['col_w'].to(dev), sigma=sigma)
    assert loss.shape == (N,) and loss.grad_fn is not None
    (loss * weight.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert all([within(f'temporal_loss order={order}', n, h, f, r) for n, h, f, r in zip(('loss', 'x.grad'), (loss.detach(), x.grad), f32, ref)])


def test_rotation_smoothness_loss_node(dev):
    from romp_amd.clip import rotation_smoothness_loss
    prev, nxt = tables('interleaved')
    N = prev.numel()
    rot = rotation(prev, nxt, 710, True)
    weight = 0.5 + torch.rand(N, generator=torch.Generator().manual_seed(711))

    def cpu(dtype):
        p = rot['poses'].to(dtype).clone().requires_grad_(True)
        loss = rotation_smooth_torch(p, prev, nxt, rot['joint_w'], rot['sigma_rot'], dtype)
        (loss * weight.to(dtype)).sum().backward()
        return loss.detach().double(), p.grad.double()

    ref, f32 = cpu(torch.float64), cpu(torch.float32)
    p = rot['poses'].to(dev).requires_grad_(True)
    loss = rotation_smoothness_loss(p, (prev.to(dev), nxt.to(dev)), joint_w=rot['joint_w'], sigma=rot['sigma_rot'])
    (loss * weight.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert all([within('rotation_smoothness_loss', n, h, f, r) for n, h, f, r in zip(('loss', 'poses.grad'), (loss.detach(), p.grad), f32, ref)])


# ------------------------------------------------------------------------------------------------ romp_clip_accel
def accel_rows(order):
    """One chain whose frames lie in the rows `order`: -> prev, next."""
    prev, nxt = [-1] * len(order), [-1] * len(order)
    for a, b in zip(order[:-1], order[1:]):
        nxt[a], prev[b] = b, a
    return torch.tensor(prev, dtype=torch.int32), torch.tensor(nxt, dtype=torch.int32)


@pytest.mark.parametrize('shuffle', [False, True])
def test_accel_against_the_reference_restatement(dev, shuffle):
    """The inputs of tests/make_golden_clip.py (7 frames x 14 joints, vis hiding the first, a middle and the last frame) against
    accel_np: without and with gt, every vis row, and K < J through an index table.  Values are float32 roundings of float64
    sums of 14 norms: 2^-23 of the value."""
    from romp_amd import evaluation as E
    joints, gt, vis = accel_inputs()
    T = joints.shape[0]
    order = torch.randperm(T, generator=torch.Generator().manual_seed(1)).tolist() if shuffle else list(range(T))
    prev, nxt = accel_rows(order)
    rows = torch.tensor(order)
    put = lambda a: torch.from_numpy(np.asarray(a))
    Jd, Gd = torch.empty(T, 14, 3), torch.empty(T, 14, 3)
    Jd[rows], Gd[rows] = put(joints), put(gt)
    links = (prev.to(dev), nxt.to(dev))
    centre = rows[1:-1]                                          # entry i of accel_np is centred on frame i + 1

    def compare(tag, got, want, keep):
        value, valid = got[0].cpu(), got[1].cpu()
        assert value.dtype == torch.float32 and valid.dtype == torch.uint8
        mask = torch.zeros(T, dtype=torch.bool)
        mask[centre[torch.from_numpy(keep)]] = True
        assert torch.equal(valid.bool(), mask), tag
        assert bool((value[~mask] == 0).all()), tag
        err = float((value[centre].double() - torch.from_numpy(want * keep)).abs().max() / np.abs(want).max())
        print(f'accel {tag}: max|ref| {np.abs(want).max():.3g} err {err:.3e} bound {2.0 ** -23:.3e}')
        assert err <= 2.0 ** -23, tag

    compare('plain', E.accel(Jd.to(dev), links), *accel_np(joints))
    compare('error', E.accel_error(Jd.to(dev), Gd.to(dev), links), *accel_np(joints, gt))
    for k in range(vis.shape[0]):
        v = torch.empty(T, dtype=torch.uint8)
        v[rows] = put(vis[k])
        compare(f'vis {k}', E.accel_error(Jd.to(dev), Gd.to(dev), links, vis=v), *accel_np(joints, gt, vis[k]))
    inds = [11, 2, 7, 0, 5]
    compare('K < J', E.accel_error(Jd.to(dev), Gd.to(dev), links, joint_inds=inds), *accel_np(joints[:, inds], gt[:, inds]))
    value, keep = accel_np(joints)
    mean = float(E.mean_accel(Jd.to(dev), links))
    assert abs(mean - value.mean()) <= 4 * 2.0 ** -23 * value.mean()


def test_accel_on_two_tracks_and_a_singleton(dev):
    from romp_amd import evaluation as E
    prev, nxt = tables('singleton')
    g = torch.Generator().manual_seed(720)
    joints = torch.randn(7, 71, 3, generator=g)
    value, valid = E.accel(joints.to(dev), (prev, nxt))
    rows = [0, 1, 3, 4, 5, 6]
    want, _ = accel_np(joints[rows].numpy())
    assert valid.cpu().tolist() == [0, 1, 0, 1, 1, 1, 0]
    assert float((value.cpu()[rows[1:-1]].double() - torch.from_numpy(want)).abs().max()) <= 2.0 ** -23 * want.max()


# ------------------------------------------------------------------------------------------------ KeypointFitter with links
TRACKS, FRAMES = 2, 6


def clip_case(model, camera, root_align, seed, noise_kp=0.01, noise_start=0.05):
    """2 tracks x 6 frames in frame-major order: a smooth motion (betas per track, poses and camera linear in time plus a slow
    sine), keypoints = its projection plus noise, start values = the truth plus per-frame noise.  -> dict of float32 tensors."""
    from romp_amd.clip import clip_links
    g = torch.Generator().manual_seed(seed)
    N = TRACKS * FRAMES
    frame = torch.arange(FRAMES).repeat_interleave(TRACKS)
    track = torch.arange(TRACKS).repeat(FRAMES) + 5
    t = frame.float()[:, None] / (FRAMES - 1)
    per_track = lambda *s: torch.randn(TRACKS, *s, generator=g)[track - 5]
    betas = 0.5 * per_track(10)
    poses = 0.2 * per_track(72) + t * 0.3 * per_track(72) + 0.1 * torch.sin(3 * t) * per_track(72)
    if camera == 'weak':
        cam = torch.tensor([0.9, 0.05, -0.03]) + 0.05 * per_track(3) + t * 0.1 * per_track(3)
    else:
        cam = torch.tensor([0.1, -0.2, 4.0]) + 0.2 * per_track(3) + t * 0.3 * per_track(3)
    _, jt = smpl_torch(model, betas, poses, root_align, torch.float64)
    kp = (project_torch(jt, cam, camera) + noise_kp * torch.randn(N, J, 2, generator=g).double()).float()
    conf = 0.2 + 0.8 * torch.rand(N, J, generator=g)
    b0 = betas + noise_start * torch.randn(N, 10, generator=g)
    p0 = poses + noise_start * torch.randn(N, 72, generator=g)
    c0 = cam * (1 + 0.02 * torch.randn(N, 3, generator=g))
    return dict(b0=b0, p0=p0, c0=c0, kp=kp, conf=conf, links=clip_links(track, frame), truth=jt.float())


SMOOTH = dict(w_smooth_pose=0.03, w_smooth_joints=(0.2, 0.5), w_smooth_cam=(0.3, 0.1), w_smooth_betas=0.4, sigma_smooth=0.3,
              smooth_joint_inds=list(range(24)) + [40, 70])
FIT_KEYS = ('betas', 'poses', 'cam', 'loss_history', 'smooth_history')


@pytest.mark.parametrize('camera,root_align', [('weak', False), ('perspective', True)])
def test_five_steps_with_every_smoothness_term_equal_the_float64_loop(dev, camera, root_align):
    from romp_amd.fitting import KeypointFitter
    model, smpl = layer(dev)
    c = clip_case(model, camera, root_align, 800)
    joint_w = 0.5 + torch.rand(24, generator=torch.Generator().manual_seed(801))
    args = dict(steps=5, lr=0.02, sigma=0.05, w_betas=1e-3, w_pose=2e-3, joint_w=joint_w, **SMOOTH)
    loop = lambda dtype: fit_clip_loop_torch(model, c['b0'], c['p0'], c['c0'], c['links'], c['kp'], c['conf'], camera=camera,
                                             root_align=root_align, dtype=dtype, **args)
    want, f32 = loop(torch.float64), loop(torch.float32)
    got = KeypointFitter(smpl, camera=camera, root_align=root_align, **args).fit(c['b0'], c['p0'], c['c0'], c['kp'], c['conf'], links=c['links'])
    torch.cuda.synchronize()
    N = TRACKS * FRAMES
    assert got['loss_history'].shape == (6, N) and got['smooth_history'].shape == (6, N, 7) and got['smooth_history'].is_cuda
    ok = [within(f'clip fitter {camera}', k, got[k], f32[k], want[k]) for k in FIT_KEYS]
    v, j, _ = smpl(got['betas'], got['poses'], root_align=root_align)
    assert torch.equal(v, got['verts']) and torch.equal(j, got['joints'])
    assert all(ok)


@pytest.mark.parametrize('camera,root_align', [('weak', False), ('perspective', True)])
def test_without_links_the_fitter_is_the_old_fitter(dev, camera, root_align):
    from romp_amd.fitting import KeypointFitter
    model, smpl = layer(dev)
    c = clip_case(model, camera, root_align, 810)
    old = KeypointFitter(smpl, camera=camera, root_align=root_align, steps=3).fit(c['b0'], c['p0'], c['c0'], c['kp'], c['conf'])
    for fitter, links in ((KeypointFitter(smpl, camera=camera, root_align=root_align, steps=3, **SMOOTH), None),
                          (KeypointFitter(smpl, camera=camera, root_align=root_align, steps=3), c['links'])):
        new = fitter.fit(c['b0'], c['p0'], c['c0'], c['kp'], c['conf'], links=links)
        assert set(new) == set(old) == {'betas', 'poses', 'cam', 'verts', 'joints', 'loss_history'}
        for k in old:
            assert torch.equal(new[k], old[k]), k


PROPERTY = dict(steps=30, lr=0.02, w_smooth_joints=(0., 3.), w_smooth_cam=(0., 1.), w_smooth_betas=1., w_smooth_pose=0.05)


def test_smoothness_terms_lower_the_acceleration_of_the_fit(dev):
    """A smooth motion with noise of 0.02 on the keypoints and 0.1 on the start values, 30 steps: the mean acceleration of the
    fitted joints with the smoothness terms must be below that without.  The float64 CPU loop shows it by a factor of at least
    two, asserted before the device is touched."""
    from romp_amd import evaluation as E
    from romp_amd.fitting import KeypointFitter
    model, smpl = layer(dev)
    c = clip_case(model, 'weak', False, 820, noise_kp=0.02, noise_start=0.1)
    prev, nxt = c['links']
    rows = chains_of(prev, nxt)
    assert [len(r) for r in rows] == [FRAMES] * TRACKS

    def cpu_accel(params):
        _, joints = smpl_torch(model, params['betas'], params['poses'], False, torch.float64)
        return float(np.mean([accel_np(joints[r].numpy())[0].mean() for r in rows]))

    plain = {k: v for k, v in PROPERTY.items() if not k.startswith('w_smooth')}
    cpu = [cpu_accel(fit_clip_loop_torch(model, c['b0'], c['p0'], c['c0'], c['links'], c['kp'], c['conf'], **a)) for a in (plain, PROPERTY)]
    print(f'mean acceleration of the fitted joints, float64 CPU loop: plain {cpu[0]:.5f} smooth {cpu[1]:.5f} factor {cpu[0] / cpu[1]:.2f}')
    assert cpu[0] >= 2 * cpu[1]
    got = []
    for a in (plain, PROPERTY):
        res = KeypointFitter(smpl, **a).fit(c['b0'], c['p0'], c['c0'], c['kp'], c['conf'], links=c['links'])
        got.append(float(E.mean_accel(res['joints'], c['links'])))
    print(f'mean acceleration of the fitted joints, device: plain {got[0]:.5f} smooth {got[1]:.5f} factor {got[0] / got[1]:.2f}')
    assert got[1] < got[0]


# ------------------------------------------------------------------------------------------------ refine_clip
@pytest.mark.parametrize('kind', ['romp', 'bev'])
def test_refine_clip(dev, kind):
    """synthetic_outputs read as one track over three frames.  ROMP: one chain of three, and the smoothness terms pull the
    rows together.  BEV: the middle row is an infant, fitted in its own group, so the track is cut on both sides of it -- no
    link is left, every smoothness loss is zero, and the result is refine_outputs', bit for bit."""
    from romp_amd.clip import refine_clip
    from romp_amd.fitting import refine_outputs
    model = stand_in(dev, kind)
    out = synthetic_outputs(dev, model, kind)
    track, frame = torch.tensor([4, 4, 4]), torch.tensor([10, 11, 12])
    shifted = out['pj2d_org'] + 8.
    args = dict(pad_info=PAD, steps=5, lr=0.01)
    smooth = dict(w_smooth_cam=(1., 0.5), w_smooth_pose=0.1, w_smooth_betas=0.5, w_smooth_joints=(0.5, 0.5))
    plain = refine_outputs(model, out, shifted, **args)
    res = refine_clip(model, out, track, frame, shifted, **args, **smooth)
    torch.cuda.synchronize()
    cam_key = 'cam' if kind == 'romp' else 'cam_trans'
    assert res['smooth_history'].shape == (6, 3, 7) and res['fit_loss'].shape == (3, 2)
    assert 'smooth_history' not in plain
    hist = res['smooth_history'].cpu()
    if kind == 'romp':
        assert bool((hist[:, 0] == 0).all()) and bool((hist[0, 1:, [0, 2, 4, 6]] > 0).all()) and bool((hist[0, 1, [1, 3]] > 0).all())
        assert bool((hist[:, 2, [1, 3, 5]] == 0).all())              # the last row has no acceleration term
        assert float(hist[-1, 1:, 2].sum()) < float(hist[0, 1:, 2].sum())          # the cameras moved towards each other
        assert not torch.equal(res[cam_key], plain[cam_key])
        verts, joints, _ = model.smpl_parser.smpl_model(res['smpl_betas'], res['smpl_thetas'])
        assert torch.equal(verts, res['verts']) and torch.equal(joints, res['joints'])
    else:
        assert bool((hist == 0).all())
        for k in ('smpl_betas', 'smpl_thetas', 'cam_trans', 'verts', 'joints', 'pj2d_org', 'fit_loss'):
            assert torch.equal(res[k], plain[k]), k
    gap = refine_clip(model, out, track, torch.tensor([10, 12, 14]), shifted, **args, **smooth)        # every gap is 2 frames
    assert bool((gap['smooth_history'] == 0).all())
    if kind == 'bev':                                            # max_gap = 2 links the two adults across the infant's frame
        two = refine_clip(model, out, track, frame, shifted, max_gap=2, **args, **smooth)
        assert bool((two['smooth_history'][0, 2, [0, 2, 4, 6]] > 0).all()) and bool((two['smooth_history'][:, 1] == 0).all())
