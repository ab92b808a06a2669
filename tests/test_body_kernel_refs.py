"""CPU tests of oracle/body_kernels_ref.py, the restatements the GPU tests of the per-person kernels are judged by: the
float32 restatements against the reference-written fixture tests/golden/body_edges.npz (oracle/make_golden_body_edges.py),
and the float32-to-float64 distance of every restatement on every input of tests/test_gpu_body_kernels.py, printed (run with
-s): those distances are what the GPU bounds are built from."""
import os

import numpy as np
import pytest

from oracle import body_kernels_ref as K
from oracle import romp_oracle as O


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'body_edges.npz'))


def _bits(a, b):
    """Bit equality of two float32 arrays, NaN payloads aside (NaN == NaN, +0 != -0)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | nan).all())


@pytest.mark.parametrize('tag,nb', [('smpl', 10), ('smpla', 11)])
def test_smpl_restatement_vs_reference(g, tag, nb):
    """The reference's SMPL.forward is float32 torch: its einsum / matmul block their sums as the BLAS likes, numpy's block
    theirs differently, so the two float32 evaluations are not bit-equal.  Each is one legitimate float32 ordering; the
    reference's output is held to the very bound the device is held to (C_ORDER * d32 + floor against float64, per person),
    on the stored vertex subset and all 71 joints, with and without root alignment."""
    model = O.make_synthetic_smpl(seed=0, n_betas=nb)
    be, po, sl = K.smpl_edge_batch(nb)
    vi = g[f'{tag}_vertex_index']
    assert np.array_equal(vi, K.fixture_vertices(model))
    for ra in (0, 1):
        v32, j32, _ = K.smpl_forward(model, be, po, root_align=bool(ra))
        v64, j64, _ = K.smpl_forward(model, be, po, root_align=bool(ra), dtype=np.float64)
        bv, dv = K.order_bound(v32, v64, (1, 2))
        bj, dj = K.order_bound(j32, j64, (1, 2))
        ev = np.abs(g[f'{tag}_verts_ra{ra}'].astype(np.float64) - v64[:, vi])
        ej = np.abs(g[f'{tag}_joints_ra{ra}'].astype(np.float64) - j64)
        for k, s in sl.items():
            print(f'D32 {tag} ra={ra} {k}: verts d32 {dv[s].max():.3e} joints d32 {dj[s].max():.3e}; reference err/bound verts '
                  f'{(ev / bv)[s].max():.3f} joints {(ej / bj)[s].max():.3f}')
        assert (ev <= bv).all() and (ej <= bj).all()


def test_projection_restatements_bit_exact(g):
    """Elementwise float32 operations in the reference's order: bit for bit, every pad layout, negative and tiny scales."""
    rs = np.random.RandomState(6000)
    joints = rs.randn(5, 71, 3).astype(np.float32)
    verts = rs.randn(5, 301, 3).astype(np.float32)
    cams, tr = K.edge_cams(5), K.bev_trans(5)
    for name, pad in K.PADS.items():
        pj, org, ct = K.project(joints, cams, pad)
        assert _bits(pj, g[f'pj2d_{name}']) and _bits(org, g[f'pj2d_org_{name}']) and _bits(ct, g['cam_trans'])
        vc, vo = K.project_verts(verts, cams, pad)
        assert _bits(vc, g[f'verts_camed_{name}']) and _bits(vo, g[f'verts_camed_org_{name}'])
        assert _bits(K.bev_project_verts(verts, tr, pad), g[f'bev_verts_camed_org_{name}'])
        for fn, args in ((K.project, (joints, cams, pad)), (K.project_verts, (verts, cams, pad)), (K.bev_project_verts, (verts, tr, pad))):
            a32, a64 = fn(*args), fn(*args, dtype=np.float64)
            a32, a64 = (a32, a64) if isinstance(a32, tuple) else ((a32,), (a64,))
            print(f'D32 {fn.__name__} pad={name}:', ' '.join('%.3e' % np.nanmax(np.abs(x.astype(np.float64) - y)) for x, y in zip(a32, a64)))


def test_cam_to_trans_restatement_bit_exact(g):
    c = K.cam_to_trans_cams(257)
    assert np.isinf(K.cam_to_trans(c)[4:6, 2]).all() and np.isnan(K.cam_to_trans(c)[4, 0])      # 1 / +-0, 0 / 0
    assert _bits(K.cam_to_trans(c, 2.0), g['cam_to_trans_w2']) and _bits(K.cam_to_trans(c, 1.0), g['cam_to_trans_w1'])


def test_estimate_translation_restatement_vs_reference(g):
    """The float32 restatement follows the reference operation for operation (float64 arithmetic on the float32 inputs,
    np.linalg.solve, float32 result): bit for bit.  The validity edges give the reference's (-1, -1, -1) exactly where the
    rule says so, and the singular on-axis system is the one input for which the reference raises."""
    X, pj = K.lsq_recovery_case(9)
    for Kj in (2, 4, 24, 64, 65, 71):
        t32, nv, kappa = K.estimate_translation(X[:, :Kj], K.px(pj, Kj))
        t64, _, _ = K.estimate_translation(X[:, :Kj], K.px(pj, Kj), dtype=np.float64)
        assert _bits(t32, g[f'lsq_recovery_K{Kj}'])
        assert (nv == Kj).all() and ((t32 == -1).all() if Kj < 4 else np.isfinite(t32).all())
        print(f'D32 estimate_translation K={Kj}: d32 {np.abs(t32 - t64).max():.3e}, condition number up to {kappa.max():.3e}')
    X, pj = K.lsq_edge_cases()
    t32, nv, _ = K.estimate_translation(X[:, :24], K.px(pj, 24))
    want_valid = dict(row_at_m2_plus3=3, row_above_m2_plus3=4, row_below_m2_plus3=3, row_at_m2_plus4=4, depth_m2_plus3=3,
                      depth_m2_up_plus3=4, depth_m2_down_plus3=4, three_valid=3, four_valid=4, all_valid=24, on_axis=24)
    raised = g['lsq_edges_raised']
    for i, name in enumerate(K.LSQ_EDGE_NAMES):
        assert nv[i] == want_valid[name], name
        if name == 'on_axis':
            assert raised[i] == 1 and np.isnan(t32[i]).all()
            continue
        assert raised[i] == 0
        assert _bits(t32[i], g['lsq_edges'][i]), name
        assert (g['lsq_edges'][i] == -1).all() == (want_valid[name] < 4), name


def test_rot6d_generator_and_bound():
    """The share of rot6d cases judged at the rotation level only (kappa > ROT6D_KAPPA_MAX) stays under 5 %, and the float32
    restatement alone keeps the derived angle bound on every other case -- on the CPU, before any device is asked.  The
    ill-conditioned rows keep 16 EPS32 kappa below 2e-3, the looser check's tolerance."""
    for n in (1, 128, 129):
        x = K.rot6d_inputs(n)
        Rt, kappa = K.rot6d_to_rotmat64(x)
        tight = kappa <= K.ROT6D_KAPPA_MAX
        assert (~tight).mean() <= 0.05
        assert n < 64 or (~tight).sum() == 4
        assert np.isfinite(kappa).all() and K.rot6d_bound(kappa).max() < 1e-3
        aa32 = O.rot6d_to_angular(x)
        d32 = K.rotation_angle(K.rodrigues64(aa32), Rt)
        print(f'D32 rot6d n={n}: angle d32 {d32[tight].max():.3e} (tight), {d32.max():.3e} (all); largest d32 / bound '
              f'{(d32 / K.rot6d_bound(kappa)).max():.3f}; loose share {(~tight).mean():.3f}')
        assert (d32 <= K.rot6d_bound(kappa)).all()


def test_rot6d_rotmat64_vs_oracle():
    x = K.rot6d_inputs(129)
    Rt, _ = K.rot6d_to_rotmat64(x)
    assert np.abs(Rt - O.rot6d_to_rotmat(x)).max() < 2e-3
    assert np.abs(Rt @ np.transpose(Rt, (0, 2, 1)) - np.eye(3)).max() < 1e-12


@pytest.mark.parametrize('name', K.TREES)
def test_trees_are_legal_and_distinct(name):
    p = K.tree(name)
    assert p.shape == (24,) and all(0 <= p[j] < j for j in range(1, 24))
    depth = np.zeros(24, int)
    for j in range(1, 24):
        depth[j] = depth[p[j]] + 1
    levels = depth.max() + 1
    widest = np.bincount(depth).max()
    print(name, 'levels', levels, 'widest level', widest)
    assert dict(smpl=(9, 5), chain=(24, 1), star=(2, 23)).get(name, (levels, widest)) == (levels, widest)


def test_tiny_poses_cancel_components_but_never_all():
    """The tiny family must contain joints whose float32 `r + 1e-8` has a zero component, and none whose angle is zero (there
    the reference itself divides by zero)."""
    e = K.poses('tiny').reshape(-1, 3) + np.float32(1e-8)
    assert (e == 0).any() and (np.abs(e).sum(1) > 0).all()


def test_smpl_d32_of_gpu_inputs():
    """The float32 restatement's distance to float64 on every SMPL input of the GPU tests, by case (the GPU bound is 8 x the
    per-person figure plus 4 ulps of the mesh's size)."""
    for case in K.smpl_cases():
        v32, j32, v64, j64 = K.smpl_case_outputs(case['name'])
        dv, dj = np.abs(v32 - v64).max((1, 2)), np.abs(j32 - j64).max((1, 2))
        print(f"D32 smpl {case['name']}: verts d32 {dv.min():.3e} .. {dv.max():.3e}, joints {dj.min():.3e} .. {dj.max():.3e}, |v| max {np.abs(v64).max():.2f}")
        assert np.isfinite(v32).all() and np.isfinite(j32).all()
        assert dv.max() < 1e-5 and dj.max() < 1e-5
