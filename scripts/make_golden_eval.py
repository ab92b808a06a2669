"""Golden fixture for the scoring kernels (tests/golden/eval_metrics.npz), written by the reference's own functions,
imported read-only by file path:

  romp/lib/evaluation/evaluation_matrix.py   batch_compute_similarity_transform_torch, compute_mpjpe, compute_error_verts
                                             (its `import config`, `import constants`, `from smplx import SMPL` are unused
                                             by these three: empty stand-in modules are registered first)
  simple_romp/evaluation/RH_evaluation/matching.py   match_2d_greedy

Arrays only.  Procrustes cases `<c>` (N is 4 or 5 everywhere: the reference's layout guard `shape[0] not in (2, 3)` misreads
a batch of 2 or 3 people): inputs `<c>_pred`, `<c>_target` (N,P,3) float32 (`verts`: rebuilt from verts_inputs() below,
not stored); the reference's float32 answer `<c>_ref_err` (N,), `<c>_ref_sRt` (N,13), `<c>_ref_aligned`; the same in
float64 numpy `<c>_f64_*`; and the measured deviation of the two, `<c>_dev_err` (relative, on the per-person error),
`<c>_dev_aligned`, `<c>_dev_t`, `<c>_dev_R` (absolute), `<c>_dev_scale` (relative).  `verts` keeps every STRIDE-th aligned point.
`quirk3_ref_err`: the reference on the first 3 people of j14 alone (its layout guard misfires).
Matching cases `m<k>`: `_pred` (P,14,2), `_gt` (G,14,2), `_valid` (G,14), the reference's `_matches` (M,2), `_fp`, `_miss`.
The seed is the first one for which, in every image, consecutive sorted pair errors (Frobenius and matrix 2-norm) differ
by at least 1e-3 relative outside the deliberate tie, so that the float32 order is no coin toss.

Build container only (needs the reference checkout):  python scripts/make_golden_eval.py
The file regenerates bit for bit (fixed zip timestamps, sorted names).
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402

REFERENCE = os.path.dirname(mg.REF)
OUT = os.path.join(ROOT, 'tests', 'golden', 'eval_metrics.npz')
F = np.float32
J = 14
STRIDE = 53                    # verts: aligned points kept
MIN_GAP = 1e-3


def load_reference():
    for name in ('config', 'constants'):
        sys.modules.setdefault(name, types.ModuleType(name))
    if 'smplx' not in sys.modules:
        m = types.ModuleType('smplx')
        m.SMPL = None
        sys.modules['smplx'] = m
    mods = []
    for name, path in (('ref_evaluation_matrix', 'romp/lib/evaluation/evaluation_matrix.py'),
                       ('ref_matching', 'simple_romp/evaluation/RH_evaluation/matching.py')):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REFERENCE, path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


# ---------------------------------------------------------------------------------------------------- Procrustes cases
def quat_rot(w, x, y, z):
    n = w * w + x * x + y * y + z * z
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], np.float64) / n


def verts_inputs(n=4, p=6890):
    """The `verts` inputs by a closed formula in integer and correctly rounded float64 arithmetic (the same bits anywhere):
    a point cloud of body extent and its image under a rational rotation, a scale and a shift, plus 1 cm of 'noise'."""
    i = np.arange(p, dtype=np.int64)[None, :, None]
    k = np.arange(n, dtype=np.int64)[:, None, None]
    c = np.arange(3, dtype=np.int64)[None, None, :]
    ext = np.array([0.3, 0.9, 0.2], np.float64)
    pred = (((i * (37 + 6 * c) + 101 * k + 17 * c) % 1009).astype(np.float64) / 1009.0 - 0.5) * ext
    noise = (((i * (53 + 4 * c) + 29 * k + 7 * c) % 997).astype(np.float64) / 997.0 - 0.5) * 0.02
    pred = pred.astype(F)
    x, y, z = (pred[..., a].astype(np.float64) for a in range(3))
    target = np.empty((n, p, 3), np.float64)
    for m in range(n):
        R = quat_rot(1 + m, 2, 2, 4)
        s, t = 0.8 + 0.125 * m, (0.25 * m, -0.5, 2.0 + m)
        for r in range(3):
            target[m, :, r] = s * ((R[r, 0] * x[m] + R[r, 1] * y[m]) + R[r, 2] * z[m]) + t[r]
    return pred, (target + noise).astype(F)


def random_rot(rng):
    q = rng.standard_normal(4)
    return quat_rot(*q)


def transformed(rng, pred, noise, mirror=False):
    out = np.empty_like(pred, dtype=np.float64)
    for n in range(len(pred)):
        R, s, t = random_rot(rng), rng.uniform(0.6, 1.5), rng.uniform(-0.5, 0.5, 3)
        y = s * pred[n].astype(np.float64) @ R.T + t
        if mirror:
            y[:, 0] = -y[:, 0]
        out[n] = y + noise * rng.standard_normal(pred[n].shape)
    return out.astype(F)


def procrustes_cases(rng):
    body = lambda n, p: (rng.standard_normal((n, p, 3)) * np.array([0.2, 0.45, 0.15])).astype(F)
    cases = {}
    p = body(5, 14)
    cases['j14'] = (p, transformed(rng, p, 0.02), None)
    p = body(4, 14)
    cases['reflect'] = (p, transformed(rng, p, 0.005, mirror=True), None)
    p = body(4, 17)
    p[:, :, 2] = F(0.75)                                             # z constant: K has an exactly vanishing row
    cases['planar'] = (p, transformed(rng, p, 0.02), None)
    a = (rng.standard_normal((4, 10)) * 0.4).astype(F)
    p = np.stack([a, a, np.full_like(a, 2.0)], -1)                   # exactly on the line (s, s, 2): K has rank 1
    cases['collinear'] = (p, transformed(rng, p, 0.02), None)
    p = body(5, 3)
    cases['p3'] = (p, transformed(rng, p, 0.02), None)
    p = body(4, 24)
    off = np.array([3.0, -2.0, 12.0])
    cases['far'] = ((p + off).astype(F), (transformed(rng, p, 0.005) + off).astype(F), None)
    p = body(5, 17)
    t = transformed(rng, p, 0.02)
    mask = np.ones(17, bool)
    mask[[2, 9, 16]] = False
    t[:, ~mask] = F(-2.0)                                            # the reference's marker of a missing annotation
    cases['masked'] = (p, t, mask)
    cases['verts'] = verts_inputs() + (None,)
    return cases


def procrustes_f64(S1, S2):
    """evaluation_matrix.py:252-303 on (N,P,3) float64, one person at a time."""
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    aligned, sRt = np.empty_like(S1), np.empty((len(S1), 13))
    for n, (a, b) in enumerate(zip(S1, S2)):
        mu1, mu2 = a.mean(0), b.mean(0)
        X1, X2 = (a - mu1).T, (b - mu2).T
        var1 = (X1 ** 2).sum()
        K = X1 @ X2.T
        U, s, Vh = np.linalg.svd(K)
        V = Vh.T
        Z = np.eye(3)
        Z[2, 2] = np.sign(np.linalg.det(U @ V.T))
        R = V @ Z @ U.T
        scale = np.trace(R @ K) / var1
        t = mu2 - scale * (R @ mu1)
        aligned[n] = scale * (a @ R.T) + t
        sRt[n] = np.concatenate([[scale], R.reshape(-1), t])
    return aligned, sRt


# ---------------------------------------------------------------------------------------------------- matching cases
def person(rng, centre):
    return (np.asarray(centre, np.float64) + rng.standard_normal((J, 2)) * np.array([35.0, 60.0])).astype(F)


def near(rng, kp, px=3.0):
    return (kp.astype(np.float64) + px * rng.standard_normal(kp.shape)).astype(F)


def matching_cases(rng):
    cases = []
    # 0: 4 preds x 3 gts: pred 0 ~ gt 2, pred 1 ~ gt 0, two strangers, gt 1 unmatched; gt 2 has 4 invalid joints (with
    #    annotations far off, so that using them would change the order)
    gt = np.stack([person(rng, (300, 400)), person(rng, (900, 380)), person(rng, (1500, 420))])
    valid = np.ones((3, J), bool)
    valid[2, [3, 4, 10, 13]] = False
    pred = np.stack([near(rng, gt[2]), near(rng, gt[0]), person(rng, (2300, 400)), person(rng, (2900, 300))])
    gt[2, [3, 4, 10, 13]] += F(45.0)
    cases.append((pred, gt, valid))
    # 1: duplicate predictions, an exact tie: the lower index wins
    gt = np.stack([person(rng, (400, 300)), person(rng, (1100, 350))])
    dup = near(rng, gt[0])
    cases.append((np.stack([dup, dup.copy(), near(rng, gt[1])]), gt, np.ones((2, J), bool)))
    # 2: 1 x 3
    gt = np.stack([person(rng, (300, 300)), person(rng, (420, 330)), person(rng, (1300, 300))])
    cases.append((near(rng, gt[1])[None], gt, np.ones((3, J), bool)))
    # 3: 4 x 1
    gt = person(rng, (700, 500))[None]
    cases.append((np.stack([person(rng, (1500, 500)), near(rng, gt[0], 6.0), near(rng, gt[0], 2.0), person(rng, (760, 540))]),
                  gt, np.ones((1, J), bool)))
    # 4: no preds; 5: no ground truth
    cases.append((np.zeros((0, J, 2), F), np.stack([person(rng, (300, 300)), person(rng, (900, 300))]), np.ones((2, J), bool)))
    cases.append((np.stack([person(rng, (300, 300)), person(rng, (900, 300))]), np.zeros((0, J, 2), F), np.ones((0, J), bool)))
    # 6: the cap, 64 preds x 5 gts.  One skeleton for everybody, so that a stranger's error is sqrt(14) * the distance of
    #    the centres: gts side by side at x = 0,14,30,48,70 (all differences distinct), preds 0..3 on gts 0..3, gt 4 unmatched,
    #    60 strangers at x = 4000 * 1.02^k (steps > 70): 4 matches, then false-positive events through the sorted strangers
    shape = rng.standard_normal((J, 2)) * np.array([35.0, 60.0])
    xs = [0.0, 14.0, 30.0, 48.0, 70.0]
    gt = np.stack([(shape + (500.0 + x, 500.0)).astype(F) for x in xs])
    pred = [near(rng, gt[k], 0.6) for k in range(4)]
    pred += [(shape + (500.0 + 4000.0 * 1.02 ** k, 500.0)).astype(F) for k in range(60)]
    cases.append((np.stack(pred), gt, np.ones((5, J), bool)))
    return cases


def pair_errors(pred, gt, valid):
    """(frobenius, 2-norm) float64 tables (P, G)."""
    fro, spec = np.zeros((len(pred), len(gt))), np.zeros((len(pred), len(gt)))
    for p in range(len(pred)):
        for g in range(len(gt)):
            d = pred[p][valid[g]].astype(np.float64) - gt[g][valid[g]].astype(np.float64)
            fro[p, g], spec[p, g] = np.linalg.norm(d), np.linalg.norm(d, 2)
    return fro, spec


def min_relative_gap(table):
    e = np.sort(table.reshape(-1))
    if len(e) < 2:
        return np.inf
    gap = np.diff(e) / e[1:]
    return gap[np.diff(e) != 0].min(initial=np.inf)                 # (an exact tie is deliberate)


def write_npz(path, arrays):
    """np.savez_compressed with sorted names and a fixed timestamp: the same bytes on every run."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name], order='C'), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    em, matching = load_reference()
    out = {}
    for seed in range(1000):
        rng = np.random.default_rng(seed)
        mcases = matching_cases(rng)
        if all(min_relative_gap(t) >= MIN_GAP for c in mcases for t in pair_errors(*c)):
            break
    else:
        raise SystemExit('no seed separates the pair errors')
    out['seed'] = np.int64(seed)
    for k, (pred, gt, valid) in enumerate(mcases):
        best, fps, misses = matching.match_2d_greedy(pred, gt, valid)
        out.update({f'm{k}_pred': pred, f'm{k}_gt': gt, f'm{k}_valid': valid,
                    f'm{k}_matches': np.asarray(best, np.int64).reshape(-1, 2), f'm{k}_fp': np.asarray(fps, np.int64),
                    f'm{k}_miss': np.asarray(misses, np.int64)})
        print(f'm{k}: {len(pred)} x {len(gt)} matches {np.asarray(best).tolist()} fp {len(fps)} miss {list(misses)}')
    out['n_match_cases'] = np.int64(len(mcases))

    names = []
    for name, (pred, target, mask) in procrustes_cases(rng).items():
        names.append(name)
        sel = slice(None) if mask is None else mask
        a, b = torch.from_numpy(pred[:, sel].copy()), torch.from_numpy(target[:, sel].copy())
        ref_al, (s, R, t) = em.batch_compute_similarity_transform_torch(a, b)
        ref_err = em.compute_mpjpe(ref_al, b).numpy()
        ref_sRt = np.concatenate([s.numpy()[:, None], R.numpy().reshape(len(pred), 9), t.numpy().reshape(len(pred), 3)], 1)
        f_al, f_sRt = procrustes_f64(pred[:, sel], target[:, sel])
        f_err = np.linalg.norm(f_al - target[:, sel].astype(np.float64), axis=-1).mean(-1)
        keep = slice(None, None, STRIDE) if name == 'verts' else slice(None)
        if name != 'verts':
            out[f'{name}_pred'], out[f'{name}_target'] = pred, target
        if mask is not None:
            out[f'{name}_mask'] = mask
        out.update({f'{name}_ref_err': ref_err, f'{name}_ref_sRt': ref_sRt.astype(F), f'{name}_ref_aligned': ref_al.numpy()[:, keep],
                    f'{name}_f64_err': f_err, f'{name}_f64_sRt': f_sRt, f'{name}_f64_aligned': f_al[:, keep],
                    f'{name}_dev_err': (np.abs(ref_err - f_err) / f_err).max(),
                    f'{name}_dev_aligned': np.abs(ref_al.numpy() - f_al).max(),
                    f'{name}_dev_scale': (np.abs(ref_sRt[:, 0] - f_sRt[:, 0]) / f_sRt[:, 0]).max(),
                    f'{name}_dev_R': np.abs(ref_sRt[:, 1:10] - f_sRt[:, 1:10]).max(),
                    f'{name}_dev_t': np.abs(ref_sRt[:, 10:] - f_sRt[:, 10:]).max()})
        print(f'{name}: N {pred.shape[0]} P {pred.shape[1]}  dev err {out[name + "_dev_err"]:.2e} aligned {out[name + "_dev_aligned"]:.2e} '
              f'scale {out[name + "_dev_scale"]:.2e} R {out[name + "_dev_R"]:.2e} t {out[name + "_dev_t"]:.2e}')
    out['cases'] = np.array(names)

    # compute_mpjpe proper on the j14 data: plain, aligned by joint 13 (align_by_parts restated), and visibility-weighted
    pred, target = out['j14_pred'], out['j14_target']
    vis = rng.random(pred.shape[:2]) > 0.25
    vis[:, 0] = True
    tp, tt = torch.from_numpy(pred), torch.from_numpy(target)
    al = lambda x: x - x[:, [13]].mean(1, keepdim=True)
    out['j14_vis'] = vis
    out['j14_ref_mpjpe'] = em.compute_mpjpe(tp, tt).numpy()
    out['j14_ref_mpjpe_root13'] = em.compute_mpjpe(al(tp), al(tt)).numpy()
    out['j14_ref_mpjpe_root13_vis'] = em.compute_mpjpe(al(tp), al(tt), torch.from_numpy(vis)).numpy()
    # the layout guard: the same call on the first 3 people of j14 takes (3,14,3) for (batch, dims, points)
    q_al, _ = em.batch_compute_similarity_transform_torch(tp[:3], tt[:3])
    out['quirk3_ref_err'] = em.compute_mpjpe(q_al, tt[:3]).numpy()
    vp, vt = verts_inputs()
    out['verts_ref_pve'] = em.compute_error_verts(target_verts=vt, pred_verts=vp).astype(F)
    write_npz(OUT, out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes, seed', seed)


if __name__ == '__main__':
    main()
