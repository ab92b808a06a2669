"""float64 restatement of the temporal smoothing -- TEST INFRASTRUCTURE ONLY (imported by tests/ only).

The same formulae as oracle/temporal_oracle.py (the OneEuro filter, Rodrigues with its ``+1e-8`` and the quaternion
renormalisation) and oracle/romp_oracle.py (rotmat_to_quat / quat_to_angle_axis with the four branches, the ``1e-6`` test on m22
and NaN -> 0), in plain numpy float64 on float32 inputs, plus a model of the bookkeeping of ``oneeuro_frames_kernel``
(csrc/temporal.hip): which reported entry is filtered with which history, and the state word each slot ends with.
"""
import copy

import numpy as np

F64 = np.float64
FREQ, BETA, DCUTOFF = 30.0, 0.7, 1.0


def mincutoffs(coeff):
    """Per segment: global rotation, body pose, betas, cam."""
    return (float(coeff), float(coeff), 0.6, 1.6)


def _alpha(cutoff):
    te = 1.0 / FREQ
    tau = 1.0 / (2 * np.pi * cutoff)
    return 1.0 / (1.0 + tau / te)


class OneEuro64:
    """One OneEuro filter over a vector of independent scalars."""

    def __init__(self, mincutoff):
        self.mincutoff = mincutoff
        self.raw = self.filtered = self.dx = None

    def step(self, x):
        x = np.array(x, F64)
        with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
            if self.raw is None:                                 # the first step passes the value through, edx = 0
                out, edx = x.copy(), np.zeros_like(x)
            else:
                dx = (x - self.raw) * FREQ
                a_d = _alpha(DCUTOFF)
                edx = a_d * dx + (1.0 - a_d) * self.dx
                a = _alpha(self.mincutoff + BETA * np.abs(edx))
                out = a * x + (1.0 - a) * self.filtered
        self.raw, self.filtered, self.dx = x, out, edx
        return out


def make_filters(smooth_coeff):
    mc = mincutoffs(smooth_coeff)
    return {'global_rot': OneEuro64(mc[0]), 'smpl_thetas': OneEuro64(mc[1]), 'smpl_betas': OneEuro64(mc[2]), 'cam': OneEuro64(mc[3])}


def state_row(filters):
    """The device's state row of a track: [initialised, x_raw[D], x_filtered[D], dx_filtered[D]], lanes root 9, pose 69, betas, cam."""
    order = ('global_rot', 'smpl_thetas', 'smpl_betas', 'cam')
    if filters['global_rot'].raw is None:
        return None
    return np.concatenate([[1.0]] + [np.concatenate([getattr(filters[k], a) for k in order]) for a in ('raw', 'filtered', 'dx')])


def rodrigues9(aa):
    """Axis-angle (3,) -> row-major 3x3 (9,)."""
    aa = np.asarray(aa, F64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        angle = np.sqrt(((aa + 1e-8) ** 2).sum())
        n = aa / angle
        half = angle * 0.5
        q = np.concatenate([[np.cos(half)], np.sin(half) * n])
        q = q / np.sqrt((q * q).sum())
    w, x, y, z = q
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    return np.array([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz, 2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                     2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2])


def rotmat_to_aa(R9):
    """Row-major 3x3 (9,), not necessarily orthonormal -> (axis-angle (3,), info).  info: branch 0..3 in the order of the reference's
    masks (d2 & d01, d2 & !d01, !d2 & d0n1, !d2 & !d0n1), t (the quantity under the root), q0_negative, s2_zero."""
    R = np.asarray(R9, F64).reshape(3, 3)
    m = R.T                                                        # the reference works on the transpose
    d2, d01, d0n1 = m[2, 2] < 1e-6, m[0, 0] > m[1, 1], m[0, 0] < -m[1, 1]
    if d2 and d01:
        branch, t = 0, 1 + m[0, 0] - m[1, 1] - m[2, 2]
        q = [m[1, 2] - m[2, 1], t, m[0, 1] + m[1, 0], m[2, 0] + m[0, 2]]
    elif d2 and not d01:
        branch, t = 1, 1 - m[0, 0] + m[1, 1] - m[2, 2]
        q = [m[2, 0] - m[0, 2], m[0, 1] + m[1, 0], t, m[1, 2] + m[2, 1]]
    elif not d2 and d0n1:
        branch, t = 2, 1 - m[0, 0] - m[1, 1] + m[2, 2]
        q = [m[0, 1] - m[1, 0], m[2, 0] + m[0, 2], m[1, 2] + m[2, 1], t]
    else:
        branch, t = 3, 1 + m[0, 0] + m[1, 1] + m[2, 2]
        q = [t, m[1, 2] - m[2, 1], m[2, 0] - m[0, 2], m[0, 1] - m[1, 0]]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        q = np.array(q, F64) / np.sqrt(F64(t)) * 0.5
        s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
        s = np.sqrt(s2)
        two_theta = 2.0 * (np.arctan2(-s, -q[0]) if q[0] < 0 else np.arctan2(s, q[0]))
        k = two_theta / s if s2 > 0 else 2.0
        aa = q[1:] * k
    aa[np.isnan(aa)] = 0.0
    return aa, dict(branch=branch, t=float(t), q0_negative=bool(q[0] < 0), s2_zero=not s2 > 0)


def smooth(filters, thetas, betas, cam):
    """oracle.temporal_oracle.smooth in float64: one person, one frame.  -> (thetas (72,), betas, cam, filtered root 3x3 as (9,), info
    of rotmat_to_aa)."""
    R = filters['global_rot'].step(rodrigues9(np.asarray(thetas, F64)[:3]))
    aa, info = rotmat_to_aa(R)
    pose = np.concatenate([aa, filters['smpl_thetas'].step(np.asarray(thetas, F64)[3:])])
    return pose, filters['smpl_betas'].step(betas), filters['cam'].step(cam), R, info


def simulate_frames(state_words, T, capacity, out_count, out_rows, out_slots, inputs, filters=None, smooth_coeff=3.0):
    """The bookkeeping of oneeuro_frames_kernel, one call.

    state_words[slot]: 0 no history; 1 history; -(t + 1): the slot's earlier track keeps its history up to frame t of this call and
    the track begun there starts afresh; -(t + 1.5): the same, and the earlier track was itself begun in this call.
    out_count (T,), out_rows / out_slots (T, capacity); inputs = (thetas, betas, cam) indexed by out_rows; filters[slot]: the
    slot's history as a dict of make_filters (changed in place; a slot without one gets it when first filtered).

    -> dict(entries=[(t, k, slot, history, (thetas, betas, cam, R, info))], words=final state words, filters=filters)
    history: 'fresh', 'continued' or 'restarted' (afresh because t >= reset_at)."""
    thetas, betas, cam = inputs
    out_rows, out_slots = np.asarray(out_rows).reshape(T, capacity), np.asarray(out_slots).reshape(T, capacity)
    filters = {} if filters is None else filters
    words = [float(w) for w in state_words]
    entries = []
    for slot in range(capacity):
        f0 = words[slot]
        reset_at = int(-f0) - 1 if f0 < 0 else -1
        fresh = f0 == 0 or (f0 < 0 and -f0 - int(-f0) > 0.25)
        for t in range(T):
            cnt = min(int(out_count[t]), capacity)
            ks = [k for k in range(cnt) if out_slots[t, k] == slot]
            if not ks:
                continue
            assert len(ks) == 1, 'a slot is reported at most once per frame'
            k = ks[0]
            history = 'fresh' if fresh else 'continued'
            if reset_at >= 0 and t >= reset_at:
                fresh, reset_at, history = True, -1, 'restarted'
            if fresh or slot not in filters:
                filters[slot] = make_filters(smooth_coeff)
            r = int(out_rows[t, k])
            entries.append((t, k, slot, history, smooth(filters[slot], thetas[r], betas[r], cam[r])))
            fresh = False
            words[slot] = 1.0
        if reset_at >= 0:
            words[slot] = 0.0                                     # begun in this call, not reported yet
    entries.sort(key=lambda e: (e[0], e[1]))
    return dict(entries=entries, words=words, filters=filters)


def clone_filters(filters):
    return copy.deepcopy(filters)
