"""Named input sequences for the OneEuro smoother tests (a helper, not a conftest): one person each, 3 to 9 frames, float32.

The root axis-angle of every frame is scripted so that the set, taken together, drives the matrix -> axis-angle step behind the filter
(``rmat_t_to_aa_dev``, csrc/rot6d.h) through all four of its branches, both signs of q0 inside the first three, the zero-rotation arm
and a small quantity under the root -- on a FILTERED matrix, which is not orthonormal.  tests/test_temporal_cases.py asserts that
coverage on the float64 path.  Body pose 0.4 * randn, betas 3 * randn (magnitudes reach about 10), cam (0.8, 0.1, -0.2) + 0.5 * randn,
each with a drift and a jitter per frame as oracle.temporal_oracle.make_sequence has them.
"""
import functools

import numpy as np

from oracle import temporal_oracle as TO

PI = np.pi
F32 = np.float32
MAX_BETAS = 16


def _axis(i, a, sign=1.0):
    v = [0.01, 0.02]
    v.insert(i, sign * a)
    return v


def _near_pi(i, sign=1.0):
    return [_axis(i, PI - 0.05 + 0.02 * k, sign) for k in range(6)]


_B = float(np.arccos(1e-6))
X, Y, Z, O3 = [PI, 0, 0], [0, PI, 0], [0, 0, PI], [0, 0, 0]
_FLIP = [0.3, 0.2, 0.1]

# name -> root axis-angle per frame
ROOTS = [
    ('zero', [O3] * 4),
    ('zero_then_small', [O3, [1e-4, 0, 0], [0, -1e-4, 1e-4], O3]),
    ('tiny', [[1e-9, -1e-9, 1e-9], [1e-7, 0, 0], O3]),
    ('x_near_pi', _near_pi(0)),
    ('y_near_pi', _near_pi(1)),
    ('z_near_pi', _near_pi(2)),
    ('x_near_minus_pi', _near_pi(0, -1.0)),
    ('y_near_minus_pi', _near_pi(1, -1.0)),
    ('z_near_minus_pi', _near_pi(2, -1.0)),
    ('x_exact_pi', [X] * 3),
    ('y_2.5', [[0.1, 2.5 + 0.05 * k, 0.1] for k in range(5)]),
    ('flip', [[s * v for v in _FLIP] for s in (1, -1, 1, -1, 1, -1)]),
    ('big_jump', [[.1, .1, .1], [3, .1, .1], [.1, 3, .1], [.1, .1, 3]]),
    ('alt_0_pix', [O3, X] * 4),
    ('alt_pix_piy', [X, Y] * 4),
    ('alt_pix_piy_piz', [X, Y, Z] * 3),
    ('x_90', [[PI / 2, 0, 0]] * 3),
    ('x_m22_boundary', [[_B, 0, 0], [_B + 1e-7, 0, 0], [_B - 1e-7, 0, 0], [_B, 0, 0]]),
    ('diag_tie', [[0, 0, 2]] * 3),
    ('two_pi', [[2 * PI - 0.01, 0, 0], [2 * PI + 0.01, 0, 0], [0, 4, 0], [0, 0, -5]]),
]
EDGE_NAMES = [n for n, _ in ROOTS]
RANDOM_SEEDS = (3, 1)                                              # fixture-style sequences, oracle.temporal_oracle.make_sequence
NAMES = EDGE_NAMES + ['random_s%d' % s for s in RANDOM_SEEDS] + ['rest']
MAX_FRAMES = 9


def aa_elementwise(name):
    """Whether the smoothed root axis-angle of the case is compared element by element.  At an angle of pi both signs of the axis
    are the same rotation, so the cases that sit there are compared as rotation matrices only."""
    return not (name.endswith('_exact_pi') or name.startswith('alt_'))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(name, thetas (T, 72), betas (T, 16), cam (T, 3)), float32.  A test with fewer betas takes the first n_betas.  Read-only."""
    if name.startswith('random_s'):
        seq = TO.make_sequence(seed=int(name[len('random_s'):]), frames=MAX_FRAMES, n_betas=MAX_BETAS)
        th, be, ca = (np.stack([f[i].numpy() for f in seq]) for i in range(3))
    else:
        rs = np.random.RandomState(100 + NAMES.index(name))
        roots = np.asarray([[0.3, -0.2, 0.5]] * 4 if name == 'rest' else dict(ROOTS)[name], np.float64)
        T = len(roots)
        pose, drift = 0.4 * rs.randn(69), 0.05 * rs.randn(69)
        betas, cam = 3.0 * rs.randn(MAX_BETAS), np.array([0.8, 0.1, -0.2]) + 0.5 * rs.randn(3)
        still = name == 'rest'                                    # every frame identical: dx is exactly 0
        th = np.stack([np.concatenate([roots[f], pose if still else pose + f * drift + 0.03 * rs.randn(69)]) for f in range(T)])
        be = np.stack([betas if still else betas + 0.05 * rs.randn(MAX_BETAS) for f in range(T)])
        ca = np.stack([cam if still else cam + 0.01 * rs.randn(3) for f in range(T)])
    out = dict(name=name, thetas=th.astype(F32), betas=be.astype(F32), cam=ca.astype(F32))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    assert 3 <= len(out['thetas']) <= MAX_FRAMES
    return out


def cases():
    return [case(n) for n in NAMES]


SEGMENTS = ('root', 'pose', 'betas', 'cam')
UNIT = 2.0 ** -24
# The device bound in units of 2^-24 * max(1, |float64|): four times the float32 oracle's own worst distance from float64 over this
# table (tests/test_temporal_cases.py measures it and holds these to it), rounded up to a power of two.
K_LINEAR, K_ROOT = 16, 32


def ratio(got, ref):
    """max |got - ref| / max(1, |ref|) in units of 2^-24 (0 for an empty array; NaN if anything is not finite)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max() / UNIT)


def output_ratios(thetas, betas, cam, ref, name):
    """One person's smoothed frame against oracle.temporal_ref64.smooth's tuple -> {root, aa, pose, betas, cam}.  The root is compared
    as a rotation matrix, and element by element (aa) where the case allows it."""
    from oracle import temporal_ref64 as R64
    t64, b64, c64 = ref[:3]
    thetas = np.asarray(thetas, np.float64)
    return {'root': ratio(R64.rodrigues9(thetas[:3]), R64.rodrigues9(t64[:3])),
            'aa': ratio(thetas[:3], t64[:3]) if aa_elementwise(name) else 0.0,
            'pose': ratio(thetas[3:], t64[3:]), 'betas': ratio(betas, b64), 'cam': ratio(cam, c64)}


def state_ratios(row, ref_row, n_betas):
    """A state row [1, x_raw, x_f, dx_f] against oracle.temporal_ref64.state_row -> {segment: ratio over x_raw and x_f,
    'dx_' + segment: ratio over dx_f}.  dx_f is a filtered difference of two consecutive x times the 30 Hz rate, so on the root, whose
    x_raw is computed (Rodrigues) and not given, it carries up to 30 times the error of two x: the float32 oracle itself is 20 units
    from float64 there (4 on the linear lanes, whose x_raw is exact).  It is listed apart for that reason; the bound is the same."""
    D = 81 + n_betas
    row, ref_row = np.asarray(row, np.float64), np.asarray(ref_row, np.float64)
    lanes = {'root': slice(0, 9), 'pose': slice(9, 78), 'betas': slice(78, 78 + n_betas), 'cam': slice(78 + n_betas, D)}
    part = lambda j, sl: ratio(row[1 + j * D:1 + (j + 1) * D][sl], ref_row[1 + j * D:1 + (j + 1) * D][sl])
    out = {}
    for seg, sl in lanes.items():
        out[seg], out['dx_' + seg] = max(part(0, sl), part(1, sl)), part(2, sl)
    return out


def oracle_state_row(filters):
    """The state row of the float32 oracle's filters (oracle.temporal_oracle.make_filters), as the device lays it out."""
    order = ('global_rot', 'smpl_thetas', 'smpl_betas', 'cam')
    dx = [filters[k].dx.filtered for k in order]
    dx = [np.zeros(len(filters[k].x.raw), F32) if isinstance(d, float) else d.numpy() for k, d in zip(order, dx)]
    return np.concatenate([np.ones(1, F32)] + [filters[k].x.raw.numpy() for k in order] + [filters[k].x.filtered.numpy() for k in order] + dx)
