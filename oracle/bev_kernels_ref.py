"""High-precision restatements of the BEV head's own kernels (romp_amd/csrc/bev.hip), one operation each,
with the error bounds their tests use.  Written against the OPERATION (bev/model.py:52-75, 188-215, 89-102,
131-140; bev/post_parser.py:109-128), not against today's kernel boundaries.

  conv3d_ref / refiner_ref     3x3x3 conv + folded BN (+ residual) (+ ReLU) in float64, with a per-voxel bound
  impulse_sites / impulse_volume / impulse_expected
                               single 1.0 voxels at every corner, mid-face and brick seam; the exact response
  bev_maps_ref                 center_map_3d / cam_maps_3d in float32, in the reference's order of operations
  bev_pack_ref                 summon_feats (model.py:190) as the Conv1d stack reads it
  mlp_ref                      the 3-layer regression MLP in float64 with a running forward error bound
  cam_trans_ref                denormalize_cam_params_to_trans in float64
  edge_cams / anchor_tie_scales / edge_parse_cases
                               the crafted camera triples and planted-peak volumes of tests/golden/bev_edges.npz

Tests import this module; the product never does.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import bev_oracle as BO

MAP, DEPTH = 128, 64
VOX = DEPTH * MAP * MAP
U = 2.0 ** -24                       # unit roundoff of float32 (round to nearest)

# every kind of seam a brick decomposition of the volume has today (bricks of 16 x 8 x 128, float4 rows), both sides each,
# plus the volume's own first and last index
SEAM_D = (0, 15, 16, 31, 32, 47, 48, 63)
SEAM_H = (0, 7, 8, 119, 120, 127)
SEAM_W = (0, 3, 4, 123, 124, 127)
MID_FACES = ((0, 64, 64), (63, 64, 64), (32, 0, 64), (32, 127, 64), (32, 64, 0), (32, 64, 127))


# ------------------------------------------------------------------------------------------------ conv3d
def conv3d_ref(x, w, scale, shift, res=None, relu=False):
    """x (B,C,D,H,W), w (C,C,3,3,3), scale / shift (C,), res like x or None.  Everything is taken to float64.
    -> (y, bound): y = [relu](conv(x, w) * scale + shift [+ res]) and the per-voxel float32 forward bound
    (27 C + 3) * 2^-24 * (|scale| * (|x| conv |w|) + |shift| + |res|): 27 C products summed in any order plus the
    scale, shift and residual roundings (Higham, Accuracy and Stability, sec. 3.1: gamma_n <= n u to first order;
    fused multiply-adds only round less).  ReLU is 1-Lipschitz and does not widen it."""
    C = w.shape[0]
    xd, wd = torch.as_tensor(x).double(), torch.as_tensor(w).double()
    sc = torch.as_tensor(scale).double().view(1, C, 1, 1, 1)
    sh = torch.as_tensor(shift).double().view(1, C, 1, 1, 1)
    y = F.conv3d(xd, wd, None, padding=1) * sc + sh
    mag = F.conv3d(xd.abs(), wd.abs(), None, padding=1) * sc.abs() + sh.abs()
    if res is not None:
        rd = torch.as_tensor(res).double()
        y = y + rd
        mag = mag + rd.abs()
    if relu:
        y = torch.relu(y)
    return y, (27 * C + 3) * U * mag


def refiner_ref(x, w1, s1, b1, w2, s2, b2):
    """BasicBlock_3D as the plan lowers it (conv1 + BN + ReLU -> conv2 + BN + residual x, no final ReLU) in float64.
    -> (y, bound): the stage-2 bound of the float32 intermediate's magnitude, plus the stage-1 error pushed through
    conv2: sum|w2[co]| * |scale2[co]| times the largest stage-1 bound."""
    t, e1 = conv3d_ref(x, w1, s1, b1, None, True)
    y, e2 = conv3d_ref(t, w2, s2, b2, x, False)
    C = w2.shape[0]
    amp = torch.as_tensor(w2).double().abs().reshape(C, -1).sum(1) * torch.as_tensor(s2).double().abs()
    # the device's stage-2 input is its own float32 intermediate t', |t' - t| <= e1: conv2 moves by at most amp * max(e1), and the
    # magnitude its rounding bound is taken of grows by the same amount (the second-order factor)
    return y, e2 + (amp * e1.max() * (1 + (27 * C + 3) * U)).view(1, C, 1, 1, 1)


def bn_fold(sd, p, eps=BO.BN_EPS):
    """(scale, shift) of an inference BatchNorm, in float64."""
    s = sd[p + '.weight'].double() / torch.sqrt(sd[p + '.running_var'].double() + eps)
    return s, sd[p + '.bias'].double() - sd[p + '.running_mean'].double() * s


def impulse_sites(n_sets, seed=0):
    """n_sets lists of (d, h, w): the 8 corners and 6 mid-faces in every set, then the seam lattice SEAM_D x SEAM_H x
    SEAM_W dealt greedily so that two sites of one set are at least 3 apart along some axis (their 3^3 responses do
    not overlap).  Every set touches every seam index of every axis."""
    rs = np.random.RandomState(seed)
    lattice = [(d, h, w) for d in SEAM_D for h in SEAM_H for w in SEAM_W]
    corners = [p for p in lattice if p[0] in (0, 63) and p[1] in (0, 127) and p[2] in (0, 127)]
    rest = [p for p in lattice if p not in corners]
    sets = []
    for _ in range(n_sets):
        order = [rest[i] for i in rs.permutation(len(rest))]
        acc = list(corners) + list(MID_FACES)
        for p in order:
            if all(max(abs(p[0] - q[0]), abs(p[1] - q[1]), abs(p[2] - q[2])) >= 3 for q in acc):
                acc.append(p)
        for ax, seam in enumerate((SEAM_D, SEAM_H, SEAM_W)):
            assert set(seam) <= {p[ax] for p in acc}, 'a seam index is missing from an impulse set'
        sets.append(acc)
    return sets


def impulse_volume(sites_per_image, C, ci):
    """(B,C,D,H,W) float32: 1.0 at the given sites of input channel ci, zero elsewhere."""
    x = np.zeros((len(sites_per_image), C, DEPTH, MAP, MAP), np.float32)
    for b, sites in enumerate(sites_per_image):
        for d, h, w in sites:
            x[b, ci, d, h, w] = 1.0
    return x


def impulse_expected(sites_per_image, w, ci):
    """The exact response to impulse_volume(.., ci) of a 3x3x3 cross-correlation with zero padding 1: around each site the
    FLIPPED kernel w[:, ci], cropped at the borders.  w (C,C,3,3,3) float32 -> (B,C,D,H,W) float32."""
    w = np.asarray(w, np.float32)
    C = w.shape[0]
    out = np.zeros((len(sites_per_image), C, DEPTH, MAP, MAP), np.float32)
    for b, sites in enumerate(sites_per_image):
        for d, h, x in sites:
            for dz in range(3):
                for dy in range(3):
                    for dx in range(3):
                        od, oh, ow = d + 1 - dz, h + 1 - dy, x + 1 - dx          # out[o] = sum_k in[o + k - 1] w[k]
                        if 0 <= od < DEPTH and 0 <= oh < MAP and 0 <= ow < MAP:
                            assert not out[b, :, od, oh, ow].any(), 'impulse responses overlap'
                            out[b, :, od, oh, ow] = w[:, ci, dz, dy, dx]
    return out


def distinct_weights(C, seed=0, signed=True):
    """27 C^2 distinct, exactly representable values in a random order (so a wrong tap lands on a different number)."""
    n = 27 * C * C
    v = (np.arange(1, n + 1, dtype=np.float32)) / 256.0
    if signed:
        v[1::3] *= -1.0
    return np.random.RandomState(seed).permutation(v).reshape(C, C, 3, 3, 3).astype(np.float32)


# ------------------------------------------------------------------------------------------------ maps / pack
def bev_maps_ref(center_fv, cam_off, center_bv, cam_off_bv):
    """center_fv (B,128,128), cam_off (B,3,128,128), center_bv / cam_off_bv (B,64,128 [d][w]) float32 ->
    center_map_3d (B,64,128,128), cam_maps_3d (B,3,64,128,128), float32 throughout and in the reference's order:
    center_fv * center_bv (model.py:195-196); coordmap + cam_off, THEN + cam_off_bv on channel 2 (:209-212)."""
    f32 = np.float32
    center_fv, cam_off = np.asarray(center_fv, f32), np.asarray(cam_off, f32)
    center_bv, cam_off_bv = np.asarray(center_bv, f32), np.asarray(cam_off_bv, f32)
    c3d = center_fv[:, None, :, :] * center_bv[:, :, None, :]
    anchor = BO.cam3dmap_anchor(60, MAP).astype(f32)
    r = np.arange(MAP, dtype=f32) / f32(MAP) * f32(2) - f32(1)
    B = center_fv.shape[0]
    cam = np.empty((B, 3, DEPTH, MAP, MAP), f32)
    cam[:, 0] = anchor[None, :, None, None] + cam_off[:, 0][:, None]
    cam[:, 1] = r[None, None, :, None] + cam_off[:, 1][:, None]
    cam[:, 2] = (r[None, None, None, :] + cam_off[:, 2][:, None]) + cam_off_bv[:, :, None, :]
    assert c3d.dtype == f32 and cam.dtype == f32
    return c3d, cam


def bev_pack_ref(maps_fv, feats):
    """maps_fv (B,4,128,128), feats (B,16,128,128) NCHW -> (B, W=128, 2560): torch.cat(..., 1).view(B, -1, 128)
    (model.py:190) with the sequence axis first, as the Conv1d layers of this project read it."""
    B = maps_fv.shape[0]
    return torch.cat([torch.as_tensor(maps_fv), torch.as_tensor(feats)], 1).reshape(B, -1, MAP).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------------ regression
def mlp_ref(x, layers):
    """x (N,128) float32 inputs (exact as given); layers [(W (out,in), b (out,)), ...] float32, ReLU between layers.
    -> (y, bound) float64.  Per layer  e_out = |W| e_in + (n + 2) 2^-24 (|W| |x| + |b|)  with n the fan-in: n products
    accumulated in any order onto the bias; ReLU is 1-Lipschitz.  |x| is taken from the float64 activations plus e_in."""
    h = np.asarray(x, np.float64)
    e = np.zeros_like(h)
    for i, (W, b) in enumerate(layers):
        W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
        n = W.shape[1]
        mag = (np.abs(h) + e) @ np.abs(W).T + np.abs(b)
        e = e @ np.abs(W).T + (n + 2) * U * mag
        h = h @ W.T + b
        if i + 1 < len(layers):
            h = np.maximum(h, 0.0)
    return h, e


def cam_trans_ref(cams):
    """denormalize_cam_params_to_trans (post_parser.py:109-128) in float64 on float32 cams -> (N,3) [x, y, depth]."""
    c = np.asarray(cams, np.float32).astype(np.float64)
    depth = 1.0 / (c[:, 0] * BO.TAN_FOV + 1e-3)
    return np.stack([c[:, 2] * depth * BO.TAN_FOV, c[:, 1] * depth * BO.TAN_FOV, depth], 1)


def anchor_tie_scales():
    """Float32 scales s whose float32 distances |s - a_k|, |s - a_{k+1}| to two adjacent anchors are EQUAL and minimal
    (argmin must take the lower index).  Searched around each midpoint; -> list of (s, k) (may be empty)."""
    a = BO.cam3dmap_anchor(60, MAP).astype(np.float32)
    found = []
    for k in range(len(a) - 1):
        m = np.float32((np.float64(a[k]) + np.float64(a[k + 1])) / 2)
        s = m
        cands = [m]
        lo = hi = m
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            cands += [lo, hi]
        for s in cands:
            d = np.abs(np.float32(s) - a)
            if d[k] == d[k + 1] and d[k] == d.min():
                found.append((np.float32(s), k))
                break
    return found


def edge_cams():
    """(M,3) float32 [scale, y, x] triples at every edge of cam_to_czyx / cam_to_trans, with no anchor tie (ties are listed
    by anchor_tie_scales and judged against this project's rule only)."""
    f32 = np.float32
    a = BO.cam3dmap_anchor(60, MAP).astype(f32)
    scales = list(a)
    for k in range(len(a) - 1):                                   # both sides of every midpoint, 1/8 of the gap away from it
        m, g = (np.float64(a[k]) + np.float64(a[k + 1])) / 2, np.float64(a[k]) - np.float64(a[k + 1])
        scales += [f32(m + g / 8), f32(m - g / 8)]
    scales += [f32(8.5), f32(100.0), f32(a[-1] / 2), f32(0.0), f32(-0.25), f32(-3.0)]
    # scale * tan_fov + 1e-3 small: depth of order 1e5 (and its sign flips just beyond)
    scales += [f32(-1e-3 / BO.TAN_FOV + 1e-5 / BO.TAN_FOV), f32(-1e-3 / BO.TAN_FOV - 1e-5 / BO.TAN_FOV)]
    yx = [f32(-1.5), f32(-1.0), f32(-1.0 + 2.0 ** -7), f32(-0.984375), f32(-0.5), f32(0.0), f32(0.015625), f32(0.5),
          f32(0.96875), f32(0.984375), f32(0.984375 + 2.0 ** -8), f32(1.0), f32(1.5), f32(1e30),
          f32(-0.984375 - 2.0 ** -24), f32(0.984375 - 2.0 ** -24), f32(0.3), f32(-0.7)]
    cams = np.empty((len(scales), 3), f32)
    cams[:, 0] = scales
    for i in range(len(scales)):
        cams[i, 1], cams[i, 2] = yx[i % len(yx)], yx[(i * 7 + 3) % len(yx)]
    d = np.abs(cams[:, :1] - a[None])
    srt = np.sort(d, 1)
    assert (srt[:, 0] < srt[:, 1]).all(), 'edge_cams must be tie-free'
    return cams


def volume_border_sites():
    """One site on each of the 8 corners, 12 edges and 6 faces of the 64 x 128 x 128 volume, pairwise >= 5 apart."""
    sites = []
    for d in (0, 32, 63):
        for h in (0, 64, 127):
            for w in (0, 64, 127):
                n_border = (d != 32) + (h != 64) + (w != 64)
                if n_border:
                    sites.append((d, h, w))
    assert len(sites) == 26
    return sites


def planted_volume(B, seed, peaks, background=(0.0, 0.05)):
    """(B,64,128,128) float32: uniform background in [lo, hi) from `seed`, then each (b, d, h, w, score) written."""
    g = torch.Generator().manual_seed(int(seed))
    lo, hi = background
    cm = torch.rand(B, DEPTH, MAP, MAP, generator=g) * (hi - lo) + lo
    for b, d, h, w, s in peaks:
        cm[int(b), int(d), int(h), int(w)] = float(np.float32(s))
    return cm


def edge_parse_cases():
    """Tie-free planted-peak volumes for the 3-D parse: name -> dict(B, seed, background, thresh, max_person, peaks (n,5))."""
    f32 = np.float32
    cases = {}
    border = volume_border_sites()
    pk = [(0, d, h, w, f32(0.5 + 0.01 * i)) for i, (d, h, w) in enumerate(border)]
    pk += [(1, d, h, w, f32(0.9 - 0.01 * i)) for i, (d, h, w) in enumerate(border[::2])]
    cases['border'] = dict(B=2, seed=1, background=(0.0, 0.05), thresh=0.25, max_person=64, peaks=pk)
    # a peak exactly at the threshold is excluded (strict >), one ulp above is kept; background partly negative
    t = f32(0.3)
    pk = [(0, 10, 20, 30, t), (0, 20, 40, 60, np.nextafter(t, f32(1))), (0, 30, 60, 90, np.nextafter(t, f32(0))),
          (0, 40, 80, 100, f32(0.7)), (0, 63, 127, 0, f32(0.31))]
    cases['threshold'] = dict(B=1, seed=2, background=(-0.2, 0.05), thresh=float(t), max_person=64, peaks=pk)
    return cases
