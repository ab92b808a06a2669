"""Plain restatements of the per-person kernels (csrc/smpl.hip and the projection half of csrc/parse.hip), one function per
kernel, numpy only.  Each takes `dtype`: np.float32 gives the reference's own operation order in the reference's own
precision (simple_romp/romp file:line cited per function), np.float64 the truth the bounds of tests/test_gpu_body_kernels.py
are measured against.  Below them the seeded generators of the edge inputs, shared by oracle/make_golden_body_edges.py and
the tests so that both draw the same cases.

The rule for every bound that is not zero:  bound = C_ORDER * d32 + floor,  d32 = |float32 restatement - float64| on that
very input, floor = FLOOR_ULPS float32 ulps of the output's magnitude (d32 can be zero).  C_ORDER = 8 covers the legitimate
differences in summation order between a kernel and the restatement (see the tests' docstrings); neither constant was
chosen from a device result."""
import numpy as np

from oracle import romp_oracle as O

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23: one ulp of 1.0
C_ORDER = 8.0
FLOOR_ULPS = 4.0
NV, NJ, NJOUT = 6890, 24, 71
INVALID_TRANS = -1.0                              # utils.py:15 INVALID_TRANS = np.ones(3) * -1


# ------------------------------------------------------------------------------------------------ restatements
def smpl_forward(model, betas, poses, root_align=False, dtype=np.float32, parents=None):
    """SMPL.forward (smpl.py:62-108) over any kinematic tree: O.smpl_forward with its `parents` argument.
    -> verts (N,6890,3), joints (N,71,3), J_transformed (N,24,3) = G[:, :, :3, 3] of the chain."""
    return O.smpl_forward(model, betas, poses, root_align=root_align, dtype=dtype, parents=parents)


def _pad(pad_info, dtype):
    top, bottom, left, right, h, w = [dtype(v) for v in np.asarray(pad_info, np.float32)]
    return top, left, max(h, w)


def to_org(k, pad_info, dtype=np.float32):
    """convert_proejection_from_input_to_orgimg (post_parser.py:81-88): ((k + 1) * max(h, w)) / 2 - (left | top | nothing),
    in that order, on 2 or 3 columns.  pad_info is a float32 tensor in the reference, so every operand is float32."""
    top, left, size = _pad(pad_info, dtype)
    k = np.asarray(k, dtype)
    out = np.empty_like(k)
    out[..., 0] = (k[..., 0] + dtype(1)) * size / dtype(2) - left
    out[..., 1] = (k[..., 1] + dtype(1)) * size / dtype(2) - top
    if k.shape[-1] == 3:
        out[..., 2] = (k[..., 2] + dtype(1)) * size / dtype(2)
    return out


def cam_to_trans(cam, weight=2.0, dtype=np.float32):
    """convert_cam_to_3d_trans (utils.py:303-307): stack(tx / s, ty / s, 1 / s) * weight -- the division first, then the weight.
    s = 0 gives inf / NaN as IEEE does, like the torch expression."""
    c = np.asarray(cam, np.float32).astype(dtype)
    s, tx, ty = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        return (np.stack([tx / s, ty / s, dtype(1) / s], 1) * dtype(weight)).astype(dtype)


def project(joints, cam, pad_info, dtype=np.float32):
    """romp_project: batch_orth_proj mode '2d' (utils.py:309-315: X[:, :, :2] * s, THEN += t -- two tensor ops, no fused
    multiply-add), to_org of it, and convert_cam_to_3d_trans.  -> pj2d (N,J,2), pj2d_org (N,J,2), cam_trans (N,3)."""
    X = np.asarray(joints, np.float32).astype(dtype)
    c = np.asarray(cam, np.float32).astype(dtype).reshape(-1, 1, 3)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        pj = X[:, :, :2] * c[:, :, 0:1]
        pj = pj + c[:, :, 1:]
        return pj, to_org(pj, pad_info, dtype), cam_to_trans(cam, 2.0, dtype)


def project_verts(verts, cam, pad_info, dtype=np.float32):
    """romp_project_verts: batch_orth_proj(mode '3d', keep_dim=True) (utils.py:309-315; z kept) and to_org on three columns
    (post_parser.py:109,113).  -> verts_camed (N,V,3), verts_camed_org (N,V,3)."""
    X = np.asarray(verts, np.float32).astype(dtype)
    c = np.asarray(cam, np.float32).astype(dtype).reshape(-1, 1, 3)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        xy = X[:, :, :2] * c[:, :, 0:1]
        xy = xy + c[:, :, 1:]
        camed = np.concatenate([xy, X[:, :, 2:3]], -1)
        return camed, to_org(camed, pad_info, dtype)


def bev_project_verts(verts, trans, pad_info, dtype=np.float32):
    """romp_bev_project_verts: perspective_projection (bev/post_parser.py:68-107) with focal 443.4, no rotation, no camera
    centre, normalize=True, the vertex z appended (:145-146), then to_org (:130-137).  p = v + t; p / (p.z + 1e-6); the
    product with K = diag(f, f, 1) is x * f + y * 0 + z' * 0, exact in any order for finite values, so one multiplication
    by float32(443.4) restates it; / 256."""
    X = np.asarray(verts, np.float32).astype(dtype)
    t = np.asarray(trans, np.float32).astype(dtype)[:, None, :]
    with np.errstate(over='ignore', invalid='ignore', divide='ignore', under='ignore'):
        p = X + t
        den = p[:, :, 2:3] + dtype(1e-6)
        xy = p[:, :, :2] / den * dtype(np.float32(443.4)) / dtype(256)
        return to_org(np.concatenate([xy, X[:, :, 2:3]], -1), pad_info, dtype)


def estimate_translation(joints_3d, joints_px, focal_length=443.4, img_size=512.0, dtype=np.float32):
    """estimate_translation with OpenCV absent (utils.py:391-434 -> estimate_translation_np :347-389, unit weights),
    vectorised over persons.  joints_3d (N,K,3) float32, joints_px (N,K,2) float32 pixels.  A joint counts when its ROW pixel
    coordinate is > -2 (:405 reads the last of two columns) and its depth is not -2 (:408); fewer than 4 -> INVALID_TRANS.
    The reference computes in float64 from the float32 inputs and stores float32, so:
      dtype float32: exactly that -- normal equations and np.linalg.solve in float64, result rounded to float32;
      dtype float64: the truth -- the same normal equations accumulated and eliminated in extended precision
                     (np.longdouble), returned as float64.
    A singular system (np.linalg.solve raises in the reference) gives NaN here; the callers decide what to do with it.
    -> trans (N,3), n_valid (N,), kappa (N,) the 2-norm condition number of the 3x3 normal matrix (inf where unsolved)."""
    X32, P32 = np.asarray(joints_3d, np.float32), np.asarray(joints_px, np.float32)
    N = X32.shape[0]
    valid = (P32[:, :, -1] > np.float32(-2.)) & (X32[:, :, -1] != np.float32(-2.))
    work = np.float64 if dtype == np.float32 else np.longdouble
    out = np.full((N, 3), INVALID_TRANS, np.float64)
    kappa = np.full(N, np.inf)
    f, c = work(focal_length), work(img_size) / work(2)
    for n in range(N):
        m = valid[n]
        if m.sum() < 4:
            continue
        X, uv = X32[n][m].astype(work), P32[n][m].astype(work)
        K = X.shape[0]
        Q = np.zeros((2 * K, 3), work)
        Q[0::2, 0], Q[1::2, 1] = f, f
        Q[:, 2] = c - uv.reshape(-1)
        rhs = (uv.reshape(-1) - c) * np.repeat(X[:, 2], 2) - f * X[:, :2].reshape(-1)
        A, b = Q.T @ Q, Q.T @ rhs
        A64 = A.astype(np.float64)
        kappa[n] = np.linalg.cond(A64) if np.isfinite(A64).all() else np.inf
        if work is np.float64:
            try:
                out[n] = np.linalg.solve(A, b)
            except np.linalg.LinAlgError:
                out[n] = np.nan
        else:                                    # A = [[d,0,a],[0,d,e],[a,e,g]]: eliminate the first two unknowns
            d, a, e, g = A[0, 0], A[0, 2], A[1, 2], A[2, 2]
            piv = g - (a * a + e * e) / d
            if piv == 0:
                out[n] = np.nan
                continue
            z = (b[2] - (a * b[0] + e * b[1]) / d) / piv
            out[n] = [np.float64((b[0] - a * z) / d), np.float64((b[1] - e * z) / d), np.float64(z)]
    return out.astype(dtype), valid.sum(1), kappa


def rot6d_to_rotmat64(x6):
    """rot6d_to_rotmat (utils.py:477-491) in float64 on float32 inputs: Gram-Schmidt of the two interleaved columns.
    -> R (n,3,3) with columns b1 b2 b3, and kappa (n,) = |a2| / |a2 - (b1.a2) b1| (>= 1; inf for a degenerate pair): the
    factor by which the subtraction amplifies the relative rounding of its operands."""
    x = np.asarray(x6, np.float32).astype(np.float64).reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    with np.errstate(invalid='ignore', divide='ignore'):
        b1 = a1 / np.maximum(np.linalg.norm(a1, axis=1, keepdims=True), 1e-6)
        u = a2 - (b1 * a2).sum(1, keepdims=True) * b1
        nu = np.linalg.norm(u, axis=1, keepdims=True)
        b2 = u / np.maximum(nu, 1e-6)
        kappa = np.where((nu[:, 0] > 0) & (np.linalg.norm(a1, axis=1) > 1e-3), np.linalg.norm(a2, axis=1) / nu[:, 0], np.inf)
    return np.stack([b1, b2, np.cross(b1, b2)], -1), kappa


def rodrigues64(aa):
    """The exact exponential map in float64 (no + 1e-8): (n,3) -> (n,3,3)."""
    aa = np.asarray(aa, np.float64)
    th = np.linalg.norm(aa, axis=1)
    small = th < 1e-12
    k = aa / np.where(small, 1.0, th)[:, None]
    K = np.zeros((len(aa), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    R = np.eye(3)[None] + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)
    R[small] = np.eye(3)
    return R


def rotation_angle(Ra, Rb):
    """Angle of Ra^T Rb in float64, from the skew part (accurate near zero) and the trace."""
    D = np.transpose(Ra, (0, 2, 1)) @ Rb
    s = 0.5 * np.sqrt((D[:, 2, 1] - D[:, 1, 2]) ** 2 + (D[:, 0, 2] - D[:, 2, 0]) ** 2 + (D[:, 1, 0] - D[:, 0, 1]) ** 2)
    c = 0.5 * (np.trace(D, axis1=1, axis2=2) - 1.0)
    return np.arctan2(s, c)


ROT6D_ROUNDINGS = 16.0     # see rot6d_bound (a CPU-side check of the generator; the GPU bound is C_ORDER * d32 + floor)
ROT6D_KAPPA_MAX = 100.0    # above this a case is judged at the rotation level only (the existing looser check)


def rot6d_bound(kappa):
    """A-priori angle bound of the float32 chain rot6d -> rotation -> quaternion -> axis-angle, per case: about 32 float32 operations
    lie on the longest path from an input to an output (normalise 7, dot 5, subtract 2, normalise 7, cross 3, quaternion 6,
    angle-axis 8 with atan2 counted as 2), each at most half an ulp relative = EPS32 / 2, so 16 EPS32; the Gram-Schmidt
    subtraction hands its operands' error on multiplied by kappa, and everything after it inherits that."""
    return ROT6D_ROUNDINGS * EPS32 * np.asarray(kappa, np.float64)


# ------------------------------------------------------------------------------------------------ bounds
def order_bound(x32, x64, axes):
    """C_ORDER * d32 + FLOOR_ULPS ulps of the magnitude, d32 and the magnitude taken as the max over `axes` (kept)."""
    x64 = np.asarray(x64, np.float64)
    d32 = np.abs(np.asarray(x32, np.float64) - x64).max(axes, keepdims=True)
    return C_ORDER * d32 + FLOOR_ULPS * EPS32 * np.abs(x64).max(axes, keepdims=True), d32


# ------------------------------------------------------------------------------------------------ inputs
TREES = ('smpl', 'chain', 'star', 'random')


def tree(name, seed=0):
    """Legal kinematic trees (parents[j] < j): SMPL's own (9 levels), the 23-deep chain (24 levels, the level-table limit),
    the star (23 joints on one level) and a seeded random one."""
    if name == 'smpl':
        return O.SMPL_PARENTS.copy()
    if name == 'chain':
        return np.arange(-1, 23, dtype=np.int64)
    if name == 'star':
        return np.array([-1] + [0] * 23, np.int64)
    rs = np.random.RandomState(100 + seed)
    return np.array([-1] + [rs.randint(0, j) for j in range(1, 24)], np.int64)


# axis and diagonal directions with mixed signs.  (-1,-1,-1) is left out: at an angle of exactly 1e-8 the reference's
# float32 `+ 1e-8` cancels all three components, the angle is 0 and the reference itself returns NaN (smpl.py:206-210).
_DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1],
                  [1, 1, -1], [-1, 1, -1], [1, -1, -1], [-1, 1, 1], [0, -1, 1], [-1, 0, 1], [-1, 1, 0]], np.float64)
TINY_ANGLES = (0.0, 1e-9, 1e-8, 1e-7, 1e-4)
BIG_ANGLES = (np.pi - 1e-3, np.pi, np.pi + 1e-3, 2 * np.pi, 50.0)


def poses(name, n=None, seed=0):
    """(n,72) float32.  'sigma0.3' | 'sigma1.5' | 'sigma6': seeded normal; 'tiny': one person per TINY_ANGLES, every
    COMPONENT of joint j is +-angle along _DIRS[(person + j) % 16] (so `+ 1e-8` cancels one or two components of some
    joints); 'big': one person per BIG_ANGLES, joint j turned by that angle about the unit vector of _DIRS[(person + j) % 16];
    'one_joint': 24 persons, person j has joint j alone turned by 1 rad."""
    if name.startswith('sigma'):
        return (float(name[5:]) * np.random.RandomState(1000 + seed).randn(n, 72)).astype(np.float32)
    if name == 'tiny':
        return np.stack([np.concatenate([a * _DIRS[(p + j) % 16] for j in range(24)]) for p, a in enumerate(TINY_ANGLES)]).astype(np.float32)
    if name == 'big':
        unit = _DIRS / np.linalg.norm(_DIRS, axis=1, keepdims=True)
        return np.stack([np.concatenate([a * unit[(p + j) % 16] for j in range(24)]) for p, a in enumerate(BIG_ANGLES)]).astype(np.float32)
    if name == 'one_joint':
        out = np.zeros((24, 72), np.float32)
        for j in range(24):
            out[j, 3 * j:3 * j + 3] = np.array([0.6, -0.5, 0.62]) / np.linalg.norm([0.6, -0.5, 0.62])
        return out
    raise KeyError(name)


def betas(n, nb, seed=0):
    """(n,nb) float32 cycling through zero, one-hot (each coefficient in turn, value 2), all +5, all -5, alternating +-5 and
    seeded normal rows."""
    rs = np.random.RandomState(2000 + seed)
    out = np.zeros((n, nb), np.float32)
    for i in range(n):
        k = i % 6
        if k == 1:
            out[i, (i // 6) % nb] = 2.0
        elif k == 2:
            out[i] = 5.0
        elif k == 3:
            out[i] = -5.0
        elif k == 4:
            out[i] = 5.0 * (-1.0) ** np.arange(nb)
        elif k == 5:
            out[i] = rs.randn(nb)
    return out


def smpl_edge_batch(nb):
    """The SMPL edge inputs of the fixture and the tests: tiny (5) + big (5) + one_joint (24) + 1.5 sigma (4) + 6 sigma (4)
    = 42 persons, with betas(42, nb).  -> betas, poses, slices by family name."""
    fam = [('tiny', poses('tiny')), ('big', poses('big')), ('one_joint', poses('one_joint')),
           ('sigma1.5', poses('sigma1.5', 4, seed=1)), ('sigma6', poses('sigma6', 4, seed=2))]
    sl, at = {}, 0
    for k, p in fam:
        sl[k] = slice(at, at + len(p))
        at += len(p)
    return betas(at, nb, seed=nb), np.concatenate([p for _, p in fam]), sl


def fixture_vertices(model):
    """The vertex subset kept in tests/golden/body_edges.npz: first, last, both sides of the 64-vertex tile seams of the two
    first and two last tiles, the 21 picked vertices, and every 97th of the rest."""
    idx = {0, NV - 1, 63, 64, 127, 128, 6783, 6784, 6847, 6848} | set(int(v) for v in np.asarray(model['extra_joints_index']))
    return np.array(sorted(idx | set(range(0, NV, 97))), np.int64)


PADS = {'tall': (0., 0., 280., 280., 1280., 720.), 'wide': (280., 280., 0., 0., 720., 1280.), 'offset': (37., 91., 13., 5., 600., 731.)}


def edge_cams(n, seed=0):
    """(n,3) float32 [s, tx, ty]: mid-range, negative, tiny (1e-3, 1e-6) scales and large offsets, cycled; the rest seeded."""
    rs = np.random.RandomState(3000 + seed)
    c = np.stack([rs.uniform(0.3, 1.4, n), rs.uniform(-0.6, 0.6, n), rs.uniform(-0.6, 0.6, n)], 1)
    special = [(-0.7, 0.2, -0.3), (1e-3, 0.5, -0.5), (-1e-3, -0.1, 0.1), (1e-6, 0.0, 0.9), (3.0, -40.0, 25.0)]
    for i in range(1, n, 2):
        if i // 2 < len(special):
            c[i] = special[i // 2]
    return c.astype(np.float32)


def cam_to_trans_cams(n, seed=0):
    """(n,3) float32 whose leading rows carry the scale edges: +-1e-30, +-1e-3, +-0, 1e30, the smallest denormal and a larger
    one; the rest seeded."""
    rs = np.random.RandomState(3100 + seed)
    c = np.stack([rs.uniform(0.2, 2.0, n), rs.uniform(-1, 1, n), rs.uniform(-1, 1, n)], 1).astype(np.float32)
    s = np.array([1e-30, -1e-30, 1e-3, -1e-3, 0.0, -0.0, 1e30, 1e-45, 3e-39], np.float32)[:n]
    c[:len(s), 0] = s
    if n > 4:
        c[4, 1] = 0.0                                           # 0 / 0
    return c


def bev_trans(n, seed=0):
    """(n,3) float32 camera translations: depths 0.5 .. 40, one close to the mesh (|v.z + t.z| small) and one behind it."""
    rs = np.random.RandomState(3200 + seed)
    t = np.stack([rs.uniform(-1, 1, n), rs.uniform(-1, 1, n), rs.uniform(0.5, 40, n)], 1)
    if n > 2:
        t[1, 2], t[2, 2] = 0.05, -3.0
    return t.astype(np.float32)


def lsq_recovery_case(n, seed=0):
    """Well-spread joints and the pixels a perspective camera (f = 443.4, centre 256) sees them at after a known
    translation.  -> joints (n,71,3) float32, pj2d (n,71,2) float32 normalised coordinates (pixels = (pj2d + 1) * 256)."""
    rs = np.random.RandomState(4000 + seed)
    X = np.clip(rs.randn(n, 71, 3) * 0.3, -0.9, 0.9)
    tz = rs.uniform(3.0, 12.0, n)                                # |x / z| <= (0.2 * 3 + 0.9) / 3 = 0.5: every pixel inside the image
    t = np.stack([rs.uniform(-0.2, 0.2, n) * tz, rs.uniform(-0.2, 0.2, n) * tz, tz], 1)[:, None]
    p = X + t
    px = 443.4 * p[:, :, :2] / p[:, :, 2:3] + 256.0
    return X.astype(np.float32), (px / 256.0 - 1.0).astype(np.float32)


LSQ_EDGE_NAMES = ('row_at_m2_plus3', 'row_above_m2_plus3', 'row_below_m2_plus3', 'row_at_m2_plus4', 'depth_m2_plus3',
                  'depth_m2_up_plus3', 'depth_m2_down_plus3', 'three_valid', 'four_valid', 'all_valid', 'on_axis')


def lsq_edge_cases(seed=0):
    """K = 24 joints of J = 71 per person, one person per LSQ_EDGE_NAMES.  Joints that must not count get the row coordinate
    -1.5 (-128 px).  `row_at_m2`: a joint whose pixel row (pj + 1) * 256 is EXACTLY -2 (pj = -1.0078125; does not count),
    `above` / `below`: that pj one float32 ulp towards / away from zero (counts / does not); `depth_m2`: a joint of depth
    exactly -2 (does not count), `up` / `down`: one ulp either side (counts); `plus3` / `plus4`: with that many plainly valid
    joints beside it.  `on_axis`: every joint at (0, 0, 1.5) seen at the image centre -- the third column of the system
    vanishes.  -> joints (11,71,3), pj2d (11,71,2) float32."""
    f32 = np.float32
    names = LSQ_EDGE_NAMES
    X, pj = lsq_recovery_case(len(names), seed=10 + seed)
    row = f32(-1.0078125)
    assert (row + f32(1)) * f32(256) == f32(-2)

    def keep(i, k):                      # only the first k joints of person i count
        pj[i, k:24, 1] = -1.5
    for i, nm in enumerate(names):
        if nm.startswith('row_'):
            k = 4 if nm.endswith('plus4') else 3
            keep(i, k + 1)
            pj[i, k, 1] = {'at': row, 'above': np.nextafter(row, f32(0)), 'below': np.nextafter(row, f32(-2))}[nm.split('_')[1]]
        elif nm.startswith('depth_'):
            keep(i, 4)
            X[i, 3, 2] = {'plus3': f32(-2), 'up': np.nextafter(f32(-2), f32(0)), 'down': np.nextafter(f32(-2), f32(-3))}[nm.split('_')[2]]
        elif nm == 'three_valid':
            keep(i, 3)
        elif nm == 'four_valid':
            keep(i, 4)
        elif nm == 'on_axis':
            X[i, :, :2], X[i, :, 2], pj[i] = 0.0, 1.5, 0.0
    return X, pj


def px(pj2d, K):
    """The pixel array the reference hands to estimate_translation: (pj2d[:, :K] + 1) * 256 in float32 (post_parser.py:98)."""
    return (np.asarray(pj2d, np.float32)[:, :K] + np.float32(1)) * np.float32(256)


def rot6d_inputs(n, seed=0):
    """(n,6) float32: seeded normal pairs; for n >= 64 four rows are replaced by ill-conditioned pairs (a2 nearly parallel to
    a1, kappa 150 .. 450: 3 % of 128) and six by rotations of pi - 1e-3, pi, 3.1 about the axes (well conditioned as
    rotations, ill conditioned as axis-angle vectors)."""
    rs = np.random.RandomState(5000 + seed)
    x = rs.randn(n, 3, 2)
    if n >= 64:
        for i, k in enumerate((150.0, 250.0, 350.0, 450.0)):
            a1 = x[8 + i, :, 0]
            perp = np.cross(a1, [0.3, -0.2, 0.9])
            x[8 + i, :, 1] = 1.3 * a1 + perp / np.linalg.norm(perp) * (1.3 * np.linalg.norm(a1) / k)
        for i, (ang, ax) in enumerate([(np.pi - 1e-3, 0), (np.pi, 1), (3.1, 2), (np.pi, 0), (np.pi - 1e-3, 2), (3.1, 1)]):
            v = np.zeros(3)
            v[ax] = ang
            R = rodrigues64(v[None])[0]
            x[20 + i, :, 0], x[20 + i, :, 1] = R[:, 0], R[:, 1]
    return x.reshape(n, 6).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the SMPL cases of the GPU tests
SMPL_NS = (1, 15, 16, 17, 64, 65, 200)           # around the 16-person groups, at and past the first capacity (64), large


def smpl_cases():
    """name, nb, tree, betas, poses of every SMPL input of tests/test_gpu_body_kernels.py: 0.3 sigma poses at every N of
    SMPL_NS for both model types on SMPL's tree, and the 42-person edge batch on each tree."""
    out = []
    for N in SMPL_NS:
        for nb in (10, 11):
            out.append(dict(name=f'n{N}_nb{nb}', nb=nb, tree='smpl', betas=betas(N, nb, seed=N), poses=poses('sigma0.3', N, seed=N)))
    for nb, tr in ((10, 'smpl'), (11, 'smpl'), (10, 'chain'), (10, 'star'), (11, 'random')):
        be, po, _ = smpl_edge_batch(nb)
        out.append(dict(name=f'edges_nb{nb}_{tr}', nb=nb, tree=tr, betas=be, poses=po))
    # the model whose extra-joint regressors weigh the LAST vertex (see smpl_model): N = 17 and the edge batch
    out.append(dict(name='n17_nb10_lastvertex', nb=10, tree='smpl', last=True, betas=betas(17, 10, seed=17), poses=poses('sigma0.3', 17, seed=17)))
    be, po, _ = smpl_edge_batch(11)
    out.append(dict(name='edges_nb11_lastvertex', nb=11, tree='smpl', last=True, betas=be, poses=po))
    return out


_MODELS, _OUT = {}, {}


def smpl_model(nb, last=False):
    """The synthetic model.  Its sparse seeded regressors put no weight on vertex 6889, the one the skinning kernel's tail
    tile recomputes in its 22 idle lanes; `last`: a copy whose 26 extra-joint regressor rows give that vertex a quarter of
    their weight (rows still sum to 1), so that those lanes' zero weight is observable."""
    if (nb, last) not in _MODELS:
        m = dict(O.make_synthetic_smpl(seed=0, n_betas=nb))
        if last:
            for k in ('J_regressor_extra9', 'J_regressor_h36m17'):
                r = m[k].clone() * 0.75
                r[:, NV - 1] += 0.25
                m[k] = r.contiguous()
        _MODELS[(nb, last)] = m
    return _MODELS[(nb, last)]


def smpl_case_outputs(name):
    """(verts32, joints32, verts64, joints64) of a case of smpl_cases(), without root alignment; the last three results are
    kept (the GPU tests ask for each case a few times in a row)."""
    if name not in _OUT:
        case = [c for c in smpl_cases() if c['name'] == name][0]
        m, p = smpl_model(case['nb'], case.get('last', False)), tree(case['tree'])
        v32, j32, _ = smpl_forward(m, case['betas'], case['poses'], parents=p)
        v64, j64, _ = smpl_forward(m, case['betas'], case['poses'], dtype=np.float64, parents=p)
        while len(_OUT) >= 3:
            _OUT.pop(next(iter(_OUT)))
        _OUT[name] = (v32, j32, v64, j64)
    return _OUT[name]


def root_aligned(verts, joints):
    """smpl.py:102-106 in the arrays' own precision: root = joints[:, [45, 46]].mean(1), subtracted from both."""
    root = joints[:, [45, 46]].mean(1, keepdims=True)
    return verts - root, joints - root
