"""GPU tests of the per-person kernels, each ALONE through the C ABI against the plain restatements of
oracle/body_kernels_ref.py: csrc/smpl.hip (smpl_ctx_create / smpl_forward: prep, pose, skin, joints, root_sub) and the
projection half of csrc/parse.hip (romp_project, romp_project_verts, romp_bev_project_verts, romp_cam_to_trans,
romp_estimate_translation, romp_rot6d_to_aa).  Every output buffer is pre-filled with NaN and is larger than the call needs.

Bounds.  A comparison is either bit for bit, or  |device - float64| <= C_ORDER * d32 + FLOOR_ULPS ulps of the output's size,
where d32 is the float32 restatement's own distance to float64 on that very input and person (computed here, on the CPU).
C_ORDER = 8 stands for the orderings in which the kernels legitimately differ from the restatement: rest joints from the
pre-regressed template instead of the 6890-term regression, the pose blend summed in four quarters, the extra joints summed
per 64-vertex tile and then over tiles, fused multiply-adds.  Each is again a float32 evaluation of the same sums, whose
error is of the size of d32; none was fitted to a device result (oracle/body_kernels_ref.py gives the rule).  Lines starting
with BOUND report the largest err / bound seen; profiles/body_kernel_tests.txt keeps them."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import body_kernels_ref as K
from oracle import romp_oracle as O

pytestmark = pytest.mark.gpu

ROMP_EINVAL = -1
NV = 6890


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan(dev, *shape):
    return torch.full(shape, float('nan'), device=dev, dtype=torch.float32)


_DEV_MODEL = {}


def _model_on(dev, nb, last=False):
    if (nb, last) not in _DEV_MODEL:
        m = K.smpl_model(nb, last)
        keys = dict(v_template='v_template', shapedirs='smpla_shapedirs' if nb == 11 else 'shapedirs', posedirs='posedirs',
                    J_regressor='J_regressor', weights='weights', e9='J_regressor_extra9', h17='J_regressor_h36m17')
        _DEV_MODEL[(nb, last)] = {k: m[v].float().contiguous().to(dev) for k, v in keys.items()}
        _DEV_MODEL[(nb, last)]['pick'] = [int(v) for v in m['extra_joints_index']]
    return _DEV_MODEL[(nb, last)]


def _create(dev, nb, parents=None, pick=None, max_persons=64, last=False):
    """smpl_ctx_create on the CURRENT torch stream -> (return code, handle)."""
    from romp_amd import lib as L
    m = _model_on(dev, nb, last)
    par = (C.c_int64 * 24)(*[int(v) for v in (K.tree('smpl') if parents is None else parents)])
    ext = (C.c_int64 * 21)(*(m['pick'] if pick is None else pick))
    h = C.c_void_p()
    rc = L.load().smpl_ctx_create(C.byref(h), L.ptr(m['v_template']), L.ptr(m['shapedirs']), nb, L.ptr(m['posedirs']), L.ptr(m['J_regressor']),
                                  L.ptr(m['weights']), par, L.ptr(m['e9']), L.ptr(m['h17']), ext, max_persons, L.stream_ptr(dev))
    return rc, h


class _Smpl:
    """A context over any tree; forward() hands back the WHOLE over-allocated, NaN-pre-filled output buffers."""

    def __init__(self, dev, nb, parents=None, last=False):
        from romp_amd import lib as L
        self.L, self.dev, self.nb = L, dev, nb
        rc, self.h = _create(dev, nb, parents, last=last)
        L.check(rc)

    def raw(self, betas, poses, ra, n_betas=None):
        """-> return code, verts (rows,6890,3), joints (rows,71,3) numpy; rows = N rounded up to whole groups of 16, plus 16."""
        L, dev = self.L, self.dev
        N = len(betas)
        rows = (N + 15) // 16 * 16 + 16
        be, po = _dev(betas, dev), _dev(poses, dev)
        v, j = _nan(dev, rows, NV, 3), _nan(dev, rows, 71, 3)
        rc = L.load().smpl_forward(self.h, L.ptr(be), self.nb if n_betas is None else n_betas, L.ptr(po), N, int(ra), L.ptr(v), L.ptr(j),
                                   L.stream_ptr(dev))
        torch.cuda.current_stream(dev).synchronize()
        return rc, v.cpu().numpy(), j.cpu().numpy()

    def forward(self, betas, poses, ra):
        rc, v, j = self.raw(betas, poses, ra)
        self.L.check(rc)
        return v, j

    def close(self):
        self.L.load().smpl_ctx_destroy(self.h)


def _check_smpl(label, v, j, N, ref, ra, pick, v_ra0=None, j_ra0=None):
    """v, j: the whole device buffers.  ref = (v32, j32, v64, j64) without root alignment.  Rows >= N still NaN, rows < N
    finite and inside the bound per person (vertices; all 71 joints, of which 0..23 are G[:, :3, 3] of the float64 chain),
    joints 24..44 bit-equal to the picked output vertices; with root alignment, bit-equal to the unaligned call minus
    (joint45 + joint46) / 2 in float32."""
    assert np.isnan(v[N:]).all() and np.isnan(j[N:]).all(), f'{label}: rows past N were written'
    v, j = v[:N], j[:N]
    assert np.isfinite(v).all() and np.isfinite(j).all(), label
    v32, j32, v64, j64 = ref
    if ra:
        (v32, j32), (v64, j64) = K.root_aligned(v32, j32), K.root_aligned(v64, j64)
    bv, _ = K.order_bound(v32, v64, (1, 2))
    bj, _ = K.order_bound(j32, j64, (1, 2))
    ev, ej = np.abs(v.astype(np.float64) - v64), np.abs(j.astype(np.float64) - j64)
    rv, rj = (ev / bv).max(), (ej / bj).max()
    print(f'BOUND smpl {label} ra={int(ra)}: largest err/bound verts {rv:.4f} joints {rj:.4f} (max-abs err {ev.max():.3e} / {ej.max():.3e}, '
          f'smallest bound {bv.min():.3e} / {bj.min():.3e})')
    assert _bits(j[:, 24:45], v[:, pick]), f'{label}: joints 24..44 are not the picked vertices'
    if ra:
        root = (j_ra0[:N, 45] + j_ra0[:N, 46]) / np.float32(2)
        assert _bits(v, v_ra0[:N] - root[:, None]) and _bits(j, j_ra0[:N] - root[:, None]), f'{label}: root alignment is not v - root'
    assert rv <= 1 and rj <= 1, f'{label}: err/bound verts {rv:.3f} joints {rj:.3f}'


def _run_case(dev, name):
    case = [c for c in K.smpl_cases() if c['name'] == name][0]
    ref = K.smpl_case_outputs(name)
    N, pick = len(case['betas']), _model_on(dev, case['nb'])['pick']
    ctx = _Smpl(dev, case['nb'], K.tree(case['tree']), last=case.get('last', False))
    try:
        v0, j0 = ctx.forward(case['betas'], case['poses'], 0)
        _check_smpl(name, v0, j0, N, ref, 0, pick)
        v1, j1 = ctx.forward(case['betas'], case['poses'], 1)
        _check_smpl(name, v1, j1, N, ref, 1, pick, v0, j0)
    finally:
        ctx.close()
    return v0, j0


@pytest.mark.parametrize('nb', [10, 11])
@pytest.mark.parametrize('N', K.SMPL_NS)
def test_smpl_sizes(dev, N, nb):
    """0.3 sigma poses at N around the 16-person groups (15, 16, 17), at and past the context's first capacity (64, 65: the
    second grows it) and large (200), both model types, without and with root alignment on one context."""
    _run_case(dev, f'n{N}_nb{nb}')


@pytest.mark.parametrize('name', ['edges_nb10_smpl', 'edges_nb11_smpl', 'edges_nb10_chain', 'edges_nb10_star', 'edges_nb11_random'])
def test_smpl_edge_poses_and_trees(dev, name):
    """The 42-person edge batch (K.smpl_edge_batch: angles of 0 .. 1e-4 whose `+ 1e-8` cancels components, pi -+ 1e-3, pi,
    2 pi, 50, one joint at a time, 1.5 and 6 sigma; betas zero / one-hot / +-5) on SMPL's tree, the 23-deep chain (24
    levels), the star (23 joints on one level: five passes of the 5-group loop) and a random tree.  In the one-joint rows a
    wrong parent, level or group stride moves exactly the descendants of that joint by far more than the bound."""
    _run_case(dev, name)


@pytest.mark.parametrize('name', ['n17_nb10_lastvertex', 'edges_nb11_lastvertex'])
def test_smpl_last_vertex_regressed(dev, name):
    """A model whose 26 extra-joint regressors put a quarter of their weight on vertex 6889 (K.smpl_model(last=True); the
    seeded synthetic regressors leave it at zero).  The last 64-vertex tile holds 42 vertices; its 22 idle lanes recompute
    vertex 6889 and must enter the regression with weight zero, otherwise joints 45..70 move by 22 * 0.25 * |v|."""
    _run_case(dev, name)


def test_smpl_call_sequence_on_one_context(dev):
    """200, then 3, then 65, then 1 person on ONE context: capacity growth with reallocation, then small calls whose last
    group of 16 holds stale rows of the large call.  Each result is inside the bound and bit-equal to the same inputs on a
    fresh context (persons do not interact)."""
    cases = {c['name']: c for c in K.smpl_cases()}
    seq = [('n200_nb10', 200), ('n17_nb10', 3), ('n65_nb10', 65), ('n1_nb10', 1)]
    pick = _model_on(dev, 10)['pick']
    ctx = _Smpl(dev, 10)
    try:
        for name, n in seq:
            be, po = cases[name]['betas'][:n], cases[name]['poses'][:n]
            ref = tuple(a[:n] for a in K.smpl_case_outputs(name))
            for ra in (0, 1):
                v, j = ctx.forward(be, po, ra)
                fresh = _Smpl(dev, 10)
                vf, jf = fresh.forward(be, po, ra)
                fresh.close()
                assert _bits(v, vf) and _bits(j, jf), f'{name}[:{n}] ra={ra} differs from a fresh context'
                if ra == 0:
                    v0, j0 = v, j
                _check_smpl(f'sequence {name}[:{n}]', v, j, n, ref, ra, pick, v0, j0)
    finally:
        ctx.close()


@pytest.mark.parametrize('N', [3, 65, 200])
def test_smpl_side_stream(dev, N):
    """The same inputs on a non-default, non-blocking torch stream -- context creation and the first call, which for
    N > 64 grows the capacity (fresh staging buffers are cleared inside that call) -- bit-equal to the default stream."""
    case = [c for c in K.smpl_cases() if c['name'] == 'n200_nb10'][0]
    be, po = case['betas'][:N], case['poses'][:N]
    ctx = _Smpl(dev, 10)
    want = [ctx.forward(be, po, ra) for ra in (0, 1)]
    ctx.close()
    _model_on(dev, 10)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        ctx = _Smpl(dev, 10)
        got = [ctx.forward(be, po, ra) for ra in (0, 1)]
        again = ctx.forward(be, po, 0)
        ctx.close()
    s.synchronize()
    for ra in (0, 1):
        assert _bits(got[ra][0], want[ra][0]) and _bits(got[ra][1], want[ra][1]), f'side stream differs, ra={ra}'
    assert _bits(again[0], want[0][0]) and _bits(again[1], want[0][1])


def test_smpl_bad_arguments(dev):
    """n_betas mismatch, parents[j] >= j (or negative), pick index out of range: each returns ROMP_EINVAL, and a context
    refused a call still computes the same bits afterwards."""
    from romp_amd import lib as L
    case = [c for c in K.smpl_cases() if c['name'] == 'n17_nb10'][0]
    ctx = _Smpl(dev, 10)
    try:
        v, j = ctx.forward(case['betas'], case['poses'], 0)
        rc, vb, jb = ctx.raw(case['betas'], case['poses'], 0, n_betas=11)
        assert rc == ROMP_EINVAL and np.isnan(vb).all() and np.isnan(jb).all()
        assert b'n_betas' in L.load().romp_last_error()
        v2, j2 = ctx.forward(case['betas'], case['poses'], 0)
        assert _bits(v, v2) and _bits(j, j2)
    finally:
        ctx.close()
    for bad in ({5: 5}, {5: 7}, {3: -1}, {23: 23}):
        p = K.tree('smpl')
        for k, val in bad.items():
            p[k] = val
        rc, _ = _create(dev, 10, parents=p)
        assert rc == ROMP_EINVAL, bad
    good = _model_on(dev, 10)['pick']
    for bad in (NV, -1, NV + 64):
        rc, _ = _create(dev, 10, pick=good[:20] + [bad])
        assert rc == ROMP_EINVAL, bad
    ctx = _Smpl(dev, 10)
    v3, j3 = ctx.forward(case['betas'], case['poses'], 0)
    ctx.close()
    assert _bits(v, v3) and _bits(j, j3)


# ------------------------------------------------------------------------------------------------ projection
def _pad_arr(pad):
    return (C.c_float * 6)(*pad)


def _inputs(N, M, seed):
    return np.random.RandomState(7000 + seed).randn(N, M, 3).astype(np.float32)


@pytest.mark.parametrize('pad', list(K.PADS))
@pytest.mark.parametrize('N,J', [(1, 71), (3, 71), (37, 71), (5, 24), (300, 1)])
def test_project_bit_exact(dev, N, J, pad):
    """romp_project against the float32 restatement, bit for bit: the file compiles with fp contraction off, so `x * s + t`
    is the reference's multiply-then-add, and every other step is one float32 operation in the reference's order.  N x J of
    71, 213, 2627, 120, 300 (no multiple of 256; 300 x 1 has more persons than joints per block); pads with h > w, w > h
    and non-zero top / left; negative and tiny scales.  cam_trans bit-equal to romp_cam_to_trans(weight = 2)."""
    from romp_amd import lib as L
    lib = L.load()
    X, cam = _inputs(N, J, N * 100 + J), K.edge_cams(N, seed=N)
    pj, org, ct, ct2 = _nan(dev, N + 2, J, 2), _nan(dev, N + 2, J, 2), _nan(dev, N + 2, 3), _nan(dev, N + 2, 3)
    Xd, cd = _dev(X, dev), _dev(cam, dev)
    L.check(lib.romp_project(L.ptr(Xd), N, J, L.ptr(cd), _pad_arr(K.PADS[pad]), L.ptr(pj), L.ptr(org), L.ptr(ct), L.stream_ptr(dev)))
    L.check(lib.romp_cam_to_trans(L.ptr(cd), N, 2.0, L.ptr(ct2), L.stream_ptr(dev)))
    torch.cuda.synchronize()
    want = K.project(X, cam, K.PADS[pad])
    for got, w, name in zip((pj, org, ct), want, ('pj2d', 'pj2d_org', 'cam_trans')):
        got = got.cpu().numpy()
        assert np.isnan(got[N:]).all(), name
        assert _bits(got[:N], w), name
    assert _bits(ct.cpu().numpy(), ct2.cpu().numpy())


@pytest.mark.parametrize('pad', list(K.PADS))
@pytest.mark.parametrize('N,V', [(3, 6890), (1, 6890), (5, 1), (5, 301)])
def test_project_verts_bit_exact(dev, N, V, pad):
    """romp_project_verts, with and without the optional `camed` output, bit for bit against the float32 restatement: the
    renderer's z-test reads these bits.  The whole file is compiled with fp contraction off (the pragma at its head; the
    second one above this kernel repeats it), so `x * s + t` is a multiply, then an add.  A build that allows contraction
    for this kernel fuses them, changes the low bit of a share of the results and fails here."""
    from romp_amd import lib as L
    lib = L.load()
    X, cam = _inputs(N, V, N * 7 + V), K.edge_cams(N, seed=V)
    Xd, cd = _dev(X, dev), _dev(cam, dev)
    want_c, want_o = K.project_verts(X, cam, K.PADS[pad])
    for with_camed in (True, False):
        camed, org = _nan(dev, N + 1, V, 3), _nan(dev, N + 1, V, 3)
        L.check(lib.romp_project_verts(L.ptr(Xd), N, V, L.ptr(cd), _pad_arr(K.PADS[pad]), L.ptr(camed) if with_camed else None, L.ptr(org),
                                       L.stream_ptr(dev)))
        torch.cuda.synchronize()
        camed, org = camed.cpu().numpy(), org.cpu().numpy()
        assert np.isnan(org[N:]).all() and np.isnan(camed[N:]).all()
        assert _bits(org[:N], want_o)
        assert _bits(camed[:N], want_c) if with_camed else np.isnan(camed).all()


@pytest.mark.parametrize('pad', list(K.PADS))
@pytest.mark.parametrize('N,V', [(3, 6890), (1, 6890), (5, 1), (5, 301)])
def test_bev_project_verts_bit_exact(dev, N, V, pad):
    """romp_bev_project_verts bit for bit: (v + t), (z + t.z) + 1e-6, the division, * float32(443.4), / 256, then the image
    transform -- one correctly rounded float32 operation per step in the reference's order (its product with diag(f, f, 1)
    adds exact zeros), contraction off.  Depths from 0.05 to 40 and one camera behind the mesh."""
    from romp_amd import lib as L
    lib = L.load()
    X, tr = _inputs(N, V, N * 11 + V), K.bev_trans(N, seed=V)
    Xd, td = _dev(X, dev), _dev(tr, dev)
    org = _nan(dev, N + 1, V, 3)
    L.check(lib.romp_bev_project_verts(L.ptr(Xd), N, V, L.ptr(td), _pad_arr(K.PADS[pad]), L.ptr(org), L.stream_ptr(dev)))
    torch.cuda.synchronize()
    org = org.cpu().numpy()
    assert np.isnan(org[N:]).all()
    assert _bits(org[:N], K.bev_project_verts(X, tr, K.PADS[pad]))


@pytest.mark.parametrize('weight', [2.0, 1.0, 0.3])
@pytest.mark.parametrize('N', [1, 256, 257])
def test_cam_to_trans_bit_exact(dev, N, weight):
    """(t / s) * w in float32, bit for bit: s of +-1e-30, +-1e-3, +-0 (inf, and NaN for 0 / 0, as IEEE and the reference's
    torch expression give them), 1e30, denormals."""
    from romp_amd import lib as L
    cam = K.cam_to_trans_cams(257)[:N]
    out = _nan(dev, N + 3, 3)
    cd = _dev(cam, dev)
    L.check(L.load().romp_cam_to_trans(L.ptr(cd), N, weight, L.ptr(out), L.stream_ptr(dev)))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.isnan(out[N:]).all()
    assert _bits(out[:N], K.cam_to_trans(cam, np.float32(weight)))


# ------------------------------------------------------------------------------------------------ least-squares translation
FOCAL = float(np.float32(443.4))     # the entry takes the focal length as a float: its truth is evaluated on that very value


def _lsq(dev, X, pj, Kj):
    from romp_amd import lib as L
    N = len(X)
    out = _nan(dev, N + 2, 3)
    Xd, pd = _dev(X, dev), _dev(pj, dev)
    L.check(L.load().romp_estimate_translation(L.ptr(Xd), N, 71, Kj, L.ptr(pd), 443.4, 512., L.ptr(out), L.stream_ptr(dev)))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.isnan(out[N:]).all()
    return out[:N]


def _lsq_bound(t64, kappa, n_rows):
    """The kernel accumulates and solves in float64 and rounds the result to float32 once: 2^-24 |t_k| (half an ulp) for the
    rounding, plus the float64 solve of the 3x3 normal equations, (n + 8) 2^-53 kappa_2(A) max|t| with n = 2 K products per
    accumulated entry (the usual forward bound of a backward-stable solve of a system formed with n-term sums)."""
    t = np.abs(t64)
    return 2.0 ** -24 * t * (1 + 2.0 ** -22) + (n_rows + 8) * 2.0 ** -53 * kappa[:, None] * t.max(1, keepdims=True)


@pytest.mark.parametrize('Kj', [2, 4, 24, 64, 65, 71])
def test_estimate_translation_recovery(dev, Kj):
    """Known translations on well-spread joints, first K of J = 71 joints (K > 64: the second pass of the 64-lane loop),
    against the extended-precision solve of the same normal equations; K = 2 has too few joints: (-1, -1, -1) exactly.
    The truth takes the inputs as the entry receives them, the focal length among them: the C ABI passes it as a float
    (443.4f = 443.4 (1 - 1.4e-8)) where the reference holds a double.  The depth scales with the focal length, so against
    the double's truth the device lies up to 1.4e-8 |t| further away: a quarter of the output's half ulp, and no part of
    this bound."""
    X, pj = K.lsq_recovery_case(33, seed=1)
    got = _lsq(dev, X, pj, Kj)
    t64, nv, kappa = K.estimate_translation(X[:, :Kj], K.px(pj, Kj), focal_length=FOCAL, dtype=np.float64)
    if Kj < 4:
        assert (got == -1).all() and (t64 == -1).all()
        return
    assert (nv == Kj).all()
    bound = _lsq_bound(t64, kappa, 2 * Kj)
    err = np.abs(got.astype(np.float64) - t64)
    print(f'BOUND estimate_translation K={Kj}: largest err/bound {(err / bound).max():.4f} (max-abs err {err.max():.3e}, largest condition number {kappa.max():.1f})')
    assert (err <= bound).all()


def test_estimate_translation_validity_edges(dev, golden_dir):
    """The validity rule at its edges (K.lsq_edge_cases): a pixel row of exactly -2 does not count and one input ulp above it
    does; a depth of exactly -2 does not count and one ulp either side does; exactly 3 counted joints give (-1, -1, -1) and
    exactly 4 a solution.  Expected values: the reference's own results (tests/golden/body_edges.npz) and the extended-
    precision solve.  All joints on the optical axis at one depth make the system singular: the reference's np.linalg.solve
    RAISES there (recorded in the fixture), so it defines no answer; this project's documented answer for a vanishing
    pivot is INVALID_TRANS, and exactly (-1, -1, -1) is pinned."""
    import os
    g = np.load(os.path.join(golden_dir, 'body_edges.npz'))
    X, pj = K.lsq_edge_cases()
    got = _lsq(dev, X, pj, 24)
    t64, nv, kappa = K.estimate_translation(X[:, :24], K.px(pj, 24), focal_length=FOCAL, dtype=np.float64)
    t64_ref, _, _ = K.estimate_translation(X[:, :24], K.px(pj, 24), dtype=np.float64)       # the reference's focal length is the double
    worst = 0.0
    for i, name in enumerate(K.LSQ_EDGE_NAMES):
        if name == 'on_axis':
            assert g['lsq_edges_raised'][i] == 1
            assert (got[i] == -1).all(), got[i]
            continue
        if nv[i] < 4:
            assert (got[i] == -1).all() and (g['lsq_edges'][i] == -1).all(), (name, got[i])
            continue
        bound = _lsq_bound(t64[i:i + 1], kappa[i:i + 1], 2 * int(nv[i]))[0]
        err = np.abs(got[i].astype(np.float64) - t64[i])
        worst = max(worst, (err / bound).max())
        assert (err <= bound).all(), (name, got[i], t64[i])
        assert (np.abs(g['lsq_edges'][i].astype(np.float64) - t64_ref[i]) <= bound).all(), name  # the reference keeps it too
    print(f'BOUND estimate_translation validity edges: largest err/bound {worst:.4f}')


# ------------------------------------------------------------------------------------------------ rot6d
@pytest.mark.parametrize('n', [1, 128, 129])
def test_rot6d_rotation_angle(dev, n):
    """romp_rot6d_to_aa at n of one workgroup, exactly and one past: the angle of R(aa_device)^T R_true in float64, R_true
    the float64 Gram-Schmidt of the input, under  C_ORDER * d32 + FLOOR_ULPS * EPS32  (d32 of that very case, which carries
    its own conditioning; the floor is 4 ulps of 1.0, the size of a rotation matrix's entries, for the cases where the float32
    restatement happens to land on the truth) for every case whose Gram-Schmidt condition kappa <= 100; the others (4 of 128, fixed
    by the generator and counted on the CPU in tests/test_body_kernel_refs.py, never by the device's error) at the
    rotation level with the existing tolerance 2e-3."""
    from romp_amd import lib as L
    x = K.rot6d_inputs(n)
    out = _nan(dev, n + 3, 3)
    xd = _dev(x, dev)
    L.check(L.load().romp_rot6d_to_aa(L.ptr(xd), n, L.ptr(out), L.stream_ptr(dev)))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.isnan(out[n:]).all() and np.isfinite(out[:n]).all()
    aa = out[:n]
    Rt, kappa = K.rot6d_to_rotmat64(x)
    tight = kappa <= K.ROT6D_KAPPA_MAX
    assert (~tight).mean() <= 0.05
    aa32 = O.rot6d_to_angular(x)
    d32 = K.rotation_angle(K.rodrigues64(aa32), Rt)
    err = K.rotation_angle(K.rodrigues64(aa), Rt)
    bound = K.C_ORDER * d32 + K.FLOOR_ULPS * K.EPS32
    print(f'BOUND rot6d n={n}: largest err/bound {(err / bound)[tight].max():.4f} (largest angle err {err[tight].max():.3e}; {int((~tight).sum())} loose cases, '
          f'angle err {err[~tight].max() if (~tight).any() else 0.0:.3e})')
    assert (err[tight] <= bound[tight]).all()
    if (~tight).any():
        np.testing.assert_allclose(O.batch_rodrigues(aa[~tight]), O.batch_rodrigues(aa32[~tight]), atol=2e-3)
