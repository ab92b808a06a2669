"""The differentiable SMPL layer on the GPU (run with -m gpu): betas.grad / poses.grad of romp_amd.smpl.SMPL (smpl_backward,
csrc/smpl_grad.hip) against float64 CPU autograd through smpl_torch, the restatement of the oracle pinned in
tests/test_smpl_grad.py, for the loss  sum gV.verts + sum gJ.joints  with seeded random gV, gJ.

Error measure: max |delta| / max |float64 reference| per gradient tensor.  The tolerance is not a constant: every case also
runs the restatement's autograd in float32 on the CPU and requires  err_HIP <= 8 * err_CPU_f32.  Both are float32
evaluations of the same sums (up to 20 670 terms) in different orders; three bits cover a difference of order and nothing
else -- a wrong sign, a transpose, a missing term or a lane counted twice is off by orders of magnitude.  Every figure is
printed before it is asserted (pytest -s)."""
import numpy as np
import pytest
import torch

from test_smpl_grad import CHAIN, STAR, model_for, smpl_torch

pytestmark = pytest.mark.gpu
NEAR_PI = (3.1, 0.2, -0.1)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


_LAYERS = {}


def layer(dev, n_betas=10, tree=None):
    """(model dict, SMPL module on the device), cached per (n_betas, tree)."""
    from romp_amd.smpl import SMPL
    key = (n_betas, tree)
    if key not in _LAYERS:
        model = model_for(n_betas, {None: None, 'chain': CHAIN, 'star': STAR}[tree])
        _LAYERS[key] = (model, SMPL(model, model_type='smpl' if n_betas == 10 else 'smpla').to(dev))
    return _LAYERS[key]


def inputs(N, n_betas, seed, theta='ordinary'):
    """Seeded float32 betas (N,n_betas), poses (N,72), gV (N,6890,3), gJ (N,71,3): the float64, the float32 and the HIP
    evaluation all start from the same float32 numbers."""
    g = torch.Generator().manual_seed(seed)
    betas = torch.randn(N, n_betas, generator=g)
    poses = 0.4 * torch.randn(N, 72, generator=g)
    if theta == 'zero':
        poses = torch.zeros(N, 72)
    elif theta == 'pi':
        poses[:, 3 * (seed % 24):3 * (seed % 24) + 3] = torch.tensor(NEAR_PI)
    gV = torch.randn(N, 6890, 3, generator=g)
    gJ = torch.randn(N, 71, 3, generator=g)
    return betas, poses, gV, gJ


def cpu_grads(model, betas, poses, root_align, gV, gJ, dtype):
    b = betas.to(dtype).clone().requires_grad_(True)
    p = poses.to(dtype).clone().requires_grad_(True)
    v, j = smpl_torch(model, b, p, root_align, dtype)
    loss = 0
    if gV is not None:
        loss = loss + (gV.to(dtype) * v).sum()
    if gJ is not None:
        loss = loss + (gJ.to(dtype) * j).sum()
    loss.backward()
    return b.grad.double(), p.grad.double()


def hip_grads(smpl, dev, betas, poses, root_align, gV, gJ, need=(True, True)):
    b = betas.to(dev).requires_grad_(need[0])
    p = poses.to(dev).requires_grad_(need[1])
    v, j, _ = smpl(b, p, root_align=root_align)
    assert v.grad_fn is not None and j.grad_fn is not None
    loss = 0
    if gV is not None:
        loss = loss + (gV.to(dev) * v).sum()
    if gJ is not None:
        loss = loss + (gJ.to(dev) * j).sum()
    loss.backward()
    torch.cuda.synchronize()
    return b.grad, p.grad


def scaled(x, ref):
    return float((x.double().cpu() - ref).abs().max() / ref.abs().max())


def check(dev, N, n_betas=10, root_align=False, tree=None, theta='ordinary', via='both', need=(True, True), seed=0, mask=None):
    """One case: the HIP gradients against float64, with the float32 CPU evaluation as the yardstick."""
    model, smpl = layer(dev, n_betas, tree)
    betas, poses, gV, gJ = inputs(N, n_betas, seed, theta)
    if mask is not None:
        gV, gJ = mask(gV, gJ)
    gV = gV if via in ('both', 'verts') else None
    gJ = gJ if via in ('both', 'joints') else None
    ref = cpu_grads(model, betas, poses, root_align, gV, gJ, torch.float64)
    f32 = cpu_grads(model, betas, poses, root_align, gV, gJ, torch.float32)
    got = hip_grads(smpl, dev, betas, poses, root_align, gV, gJ, need)
    ok = True
    for name, r, f, h, wanted in zip(('betas', 'poses'), ref, f32, got, need):
        if not wanted:
            assert h is None, name
            continue
        assert h is not None and h.shape == r.shape and h.dtype == torch.float32 and bool(torch.isfinite(h).all()), name
        e_hip, e_f32 = scaled(h, r), scaled(f, r)
        print(f'N={N} nb={n_betas} ra={root_align} tree={tree} theta={theta} via={via} {name}: max|ref| {float(r.abs().max()):.3g} '
              f'err_hip {e_hip:.3e} err_cpu_f32 {e_f32:.3e} ratio {e_hip / max(e_f32, 1e-300):.2f}')
        ok = ok and e_hip <= 8 * e_f32
    assert ok


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize('root_align', [False, True])
@pytest.mark.parametrize('n_betas', [10, 11])
@pytest.mark.parametrize('N', [1, 7, 17])          # a lone person, a partial group, a full group plus a partial one
def test_grad_sizes(dev, N, n_betas, root_align):
    check(dev, N, n_betas, root_align, seed=N)


@pytest.mark.parametrize('root_align', [False, True])
@pytest.mark.parametrize('via', ['verts', 'joints'])
def test_grad_through_one_output(dev, via, root_align):
    check(dev, 7, root_align=root_align, via=via, seed=11)


@pytest.mark.parametrize('need', [(True, False), (False, True)])
def test_grad_for_one_input(dev, need):
    check(dev, 7, root_align=True, need=need, seed=12)


@pytest.mark.parametrize('theta', ['zero', 'pi'])
def test_grad_at_zero_and_near_pi(dev, theta):
    check(dev, 7, root_align=False, theta=theta, seed=13)


@pytest.mark.parametrize('first', [6848, 6889])    # the last vertex tile (42 live lanes), and its last vertex alone
def test_grad_from_the_last_tile(dev, first):
    def mask(gV, gJ):
        m = torch.zeros_like(gV)
        m[:, first:] = gV[:, first:]
        return m, gJ
    check(dev, 7, root_align=True, via='verts', seed=14, mask=mask)


@pytest.mark.parametrize('joints,root_align', [((45, 47), True), ((0, 24), False)])   # the root path; the J_tr path
def test_grad_from_some_joints(dev, joints, root_align):
    def mask(gV, gJ):
        m = torch.zeros_like(gJ)
        m[:, joints[0]:joints[1]] = gJ[:, joints[0]:joints[1]]
        return gV, m
    check(dev, 7, root_align=root_align, via='joints', seed=15, mask=mask)


@pytest.mark.parametrize('tree', ['chain', 'star'])
def test_grad_with_another_tree(dev, tree):
    check(dev, 7, root_align=True, tree=tree, seed=16)


# ------------------------------------------------------------------------------------------------ the interface
def test_outputs_of_inputs_that_require_grad_are_differentiable(dev):
    _, smpl = layer(dev)
    betas, poses, _, _ = inputs(2, 10, 20)
    b, p = betas.to(dev).requires_grad_(True), poses.to(dev).requires_grad_(True)
    v, j, f = smpl(b, p)
    assert v.grad_fn is not None and j.grad_fn is not None and f is smpl.faces_tensor
    (v.square().sum() + j.square().sum()).backward()
    assert b.grad is not None and p.grad is not None
    assert float(b.grad.abs().max()) > 0 and float(p.grad.abs().max()) > 0


def test_default_path_is_unchanged(dev):
    _, smpl = layer(dev)
    betas, poses, _, _ = inputs(5, 10, 21)
    b, p = betas.to(dev), poses.to(dev)
    for ra in (False, True):
        v0, j0, _ = smpl(b, p, root_align=ra)                                     # nothing requires grad
        assert v0.grad_fn is None and j0.grad_fn is None and not v0.requires_grad
        bg, pg = b.clone().requires_grad_(True), p.clone().requires_grad_(True)
        with torch.no_grad():
            v1, j1, _ = smpl(bg, pg, root_align=ra)
        assert v1.grad_fn is None and j1.grad_fn is None
        v2, j2, _ = smpl(bg, pg, root_align=ra)                                   # the differentiable path's forward
        assert v2.grad_fn is not None
        for a, c in ((v0, v2), (j0, j2), (v1, v2), (j1, j2)):
            assert torch.equal(a, c.detach())
    vn, jn, _ = smpl(betas.numpy(), poses.numpy())                                # numpy inputs: no grad, same bits
    v0, j0, _ = smpl(b, p)
    assert vn.grad_fn is None and torch.equal(vn, v0) and torch.equal(jn, j0)


def test_backward_is_deterministic(dev):
    _, smpl = layer(dev)
    betas, poses, gV, gJ = inputs(17, 10, 22)
    a = hip_grads(smpl, dev, betas, poses, True, gV, gJ)
    b = hip_grads(smpl, dev, betas, poses, True, gV, gJ)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_interleaved_forwards_and_backwards(dev):
    """forward A (N = 3), forward B (N = 17), a forward of 65 persons that makes the context reallocate its staging buffers,
    then backward A and backward B (whose scratch grows past A's): each equals its own separate result."""
    from romp_amd.smpl import SMPL
    model, shared = layer(dev)
    smpl = SMPL(model).to(dev)                                                    # a fresh context and fresh scratch
    ia, ib = inputs(3, 10, 23), inputs(17, 10, 24)
    want_a = hip_grads(shared, dev, ia[0], ia[1], True, ia[2], ia[3])
    want_b = hip_grads(shared, dev, ib[0], ib[1], True, ib[2], ib[3])
    ba, pa = ia[0].to(dev).requires_grad_(True), ia[1].to(dev).requires_grad_(True)
    bb, pb = ib[0].to(dev).requires_grad_(True), ib[1].to(dev).requires_grad_(True)
    va, ja, _ = smpl(ba, pa, root_align=True)
    vb, jb, _ = smpl(bb, pb, root_align=True)
    big = inputs(65, 10, 25)
    smpl(big[0].to(dev), big[1].to(dev))
    ((ia[2].to(dev) * va).sum() + (ia[3].to(dev) * ja).sum()).backward()
    ((ib[2].to(dev) * vb).sum() + (ib[3].to(dev) * jb).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(ba.grad, want_a[0]) and torch.equal(pa.grad, want_a[1])
    assert torch.equal(bb.grad, want_b[0]) and torch.equal(pb.grad, want_b[1])


def test_backward_on_a_side_stream(dev):
    _, smpl = layer(dev)
    betas, poses, gV, gJ = inputs(7, 10, 26)
    want = hip_grads(smpl, dev, betas, poses, True, gV, gJ)
    tensors = [t.to(dev) for t in (betas, poses, gV, gJ)]
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        b, p = tensors[0].requires_grad_(True), tensors[1].requires_grad_(True)
        v, j, _ = smpl(b, p, root_align=True)
        ((tensors[2] * v).sum() + (tensors[3] * j).sum()).backward()
    s.synchronize()
    assert torch.equal(b.grad, want[0]) and torch.equal(p.grad, want[1])


def test_fit_two_persons(dev):
    """Adam, lr 0.05, 30 steps from zeros towards the mesh and joints of a seeded beta*, theta* = 0.3 randn; loss = mean
    squared vertex distance + mean squared joint distance.  The float64 CPU restatement under this recipe falls 33x; the
    HIP layer must reach a tenth of its starting loss."""
    _, smpl = layer(dev)
    g = torch.Generator().manual_seed(5)
    beta_t, theta_t = torch.randn(2, 10, generator=g).to(dev), (0.3 * torch.randn(2, 72, generator=g)).to(dev)
    with torch.no_grad():
        v_t, j_t, _ = smpl(beta_t, theta_t)
    b = torch.zeros(2, 10, device=dev, requires_grad=True)
    p = torch.zeros(2, 72, device=dev, requires_grad=True)
    opt = torch.optim.Adam([b, p], lr=0.05)
    losses = []
    for _ in range(31):
        opt.zero_grad()
        v, j, _ = smpl(b, p)
        loss = (v - v_t).square().sum(-1).mean() + (j - j_t).square().sum(-1).mean()
        losses.append(float(loss.detach()))
        if len(losses) == 31:
            break
        loss.backward()
        opt.step()
    print(f'fit: loss {losses[0]:.4g} -> {losses[-1]:.4g} ({losses[0] / losses[-1]:.1f}x) after 30 steps')
    assert losses[-1] <= losses[0] / 10
