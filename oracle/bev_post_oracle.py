"""CPU oracle for BEV's per-image post-processing -- TEST INFRASTRUCTURE ONLY.

Restates simple_romp/bev/post_parser.py: denormalize_cam_params_to_trans :114-128,
perspective_projection :68-107, convert_proejection_from_input_to_orgimg :129-136,
suppressing_redundant_prediction_via_projection :167-198, remove_outlier :200-222 (numpy, float32 unless a dtype is given).
Pinned by tests/golden/bev_post.npz (oracle/make_golden_bev_post.py runs the reference itself) and by
tests/golden/bev_post_edges.npz (oracle/make_golden_bev_post_edges.py).
"""
import numpy as np

TAN_FOV = np.float32(np.tan(np.radians(60 / 2.)))


def cam_to_trans(cam, dtype=np.float32):
    cam = np.asarray(cam, dtype)
    tan_fov = dtype(np.tan(np.radians(60 / 2.)))
    depth = (dtype(1) / (cam[:, 0] * tan_fov + dtype(1e-3)))[:, None]
    return np.concatenate([cam[:, 1:][:, ::-1] * depth * tan_fov, depth], 1).astype(dtype)


def project(joints, cam, pad_info, dtype=np.float32):
    """-> pj2d (normalised), pj2d_org (original-image pixels), cam_trans."""
    t = cam_to_trans(cam, dtype)
    p = np.asarray(joints, dtype) + t[:, None]
    pj = p[:, :, :2] / (p[:, :, 2:3] + dtype(1e-6)) * dtype(443.4) / dtype(256.0)
    top, bottom, left, right, h, w = [dtype(v) for v in pad_info]
    s = max(h, w)
    org = np.stack([(pj[:, :, 0] + 1) * s / 2 - left, (pj[:, :, 1] + 1) * s / 2 - top], -1).astype(dtype)
    return pj.astype(dtype), org, t


def _margin(margins, x, thr):
    """The smallest |x / thr - 1| of the finite values of x (0/0 rows compare false against everything)."""
    x = np.asarray(x, np.float64).ravel()
    x = x[np.isfinite(x)]
    if x.size:
        margins.append(float(np.min(np.abs(x / float(thr) - 1))))


def postprocess(joints, cam, pad_info, nms_thresh=20.0, relative_scale_thresh=1.6, scale_thresh=0.25, dtype=np.float32):
    """-> dict(pj2d, pj2d_org, cam_trans, keep (bool mask),
    margin: the smallest |x / threshold - 1| over every value compared with a threshold -- the normalised pair distances
    against the suppression threshold, and rel against relative_scale_thresh for the survivors with cam[:, 0] < scale_thresh,
    stages: dict(suppressed, outliers) -- how many rows each pass removed).
    All arithmetic and the threshold comparisons are made in `dtype`."""
    cam = np.asarray(cam, dtype)
    pj, org, t = project(joints, cam, pad_info, dtype)
    N = cam.shape[0]
    removed = np.zeros(N, bool)
    margins = []
    if N > 1:
        d = np.sqrt(((org[:, None] - org[None]) ** 2).sum(-1)).mean(-1)
        sc = cam[:, 0] * 2
        d = d / np.maximum(sc[:, None], sc[None])
        thr = dtype(nms_thresh) * max(dtype(pad_info[4]), dtype(pad_info[5])) / dtype(640)
        _margin(margins, d[np.triu_indices(N, 1)], thr)
        for a in range(N):
            for b in range(a + 1, N):
                if d[a, b] < thr:
                    removed[a if sc[a] < sc[b] else b] = True
    suppressed = int(removed.sum())
    alive = np.nonzero(~removed)[0]
    m = alive.size
    if m >= 3:
        tt = t[alive]
        dm = np.sqrt(((tt[:, None] - tt[None]) ** 2).sum(-1))
        mean = np.sort(dm, 1)[:, 1:-1].mean(1)
        with np.errstate(invalid='ignore', divide='ignore'):
            rel = mean / ((mean.sum() - mean) / (m - 1))
        small = cam[alive, 0] < dtype(scale_thresh)
        _margin(margins, rel[small], dtype(relative_scale_thresh))
        out = (rel > dtype(relative_scale_thresh)) & small
        removed[alive[out]] = True
    return {'pj2d': pj, 'pj2d_org': org, 'cam_trans': t, 'keep': ~removed, 'margin': min(margins + [1.]),
            'stages': {'suppressed': suppressed, 'outliers': int(removed.sum()) - suppressed}}
