"""The fixture tests/golden/mot_metrics.npz (written by tests/make_golden_mot.py) for test_mot.py and test_gpu_mot.py: the clips'
inputs, what the reference's TrackEval returned for them, and the bound under which a float64 result is compared with those
float32-kept values."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mot_metrics.npz')
INPUTS = ('pred_ids', 'pred_frames', 'gt_boxes', 'gt_ids', 'gt_frames', 'pred_boxes', 'pred_kp2d', 'frames')
_cache = {}


def load():
    """-> (names, {name: keyword arguments of add_clip / score_clip_host}, {name: {'HOTA', 'CLEAR', 'Identity'} as recorded}, settings)"""
    if not _cache:
        z = np.load(GOLD)
        names = [str(n) for n in z['names']]
        args, ref = {}, {}
        for n in names:
            args[n] = {k: z['%s/%s' % (n, k)] for k in INPUTS if '%s/%s' % (n, k) in z.files}
            h = {str(k): z[n + '/HOTA_arrays'][i] for i, k in enumerate(z['HOTA_arrays'])}
            h.update({str(k): z[n + '/HOTA_scalars'][i] for i, k in enumerate(z['HOTA_scalars'])})
            ref[n] = {'HOTA': h, 'CLEAR': {str(k): z[n + '/CLEAR'][i] for i, k in enumerate(z['CLEAR'])},
                      'Identity': {str(k): z[n + '/Identity'][i] for i, k in enumerate(z['Identity'])}}
        settings = dict(threshold=float(z['threshold']), max_iou=float(z['max_iou']), enlarge_xy=tuple(z['enlarge_xy'].tolist()))
        _cache['v'] = (names, args, ref, settings)
    return _cache['v']


def reference_bound(only=None):
    """TrackEval keeps HOTA's arrays in float32: a sum of n terms carries up to n roundings of 2^-24 relative (all terms are >= 0).
    Its longest sum is LocA's, one similarity per matched pair, so at most min(ground-truth rows, predicted rows) terms; the largest
    such clip of the fixture sets n.  Four more roundings for a final field: the division, the product and the root of
    HOTA = sqrt(DetA * AssA), and the store.

    The bound grows with the clips it covers, so `only` (a list of clip names) keeps it to those: the cap-sized clip 'caps' (1024
    rows a side, (1024 + 4) 2^-24 = 6.1e-5) is held to its own bound, every other clip to the bound of the others, (146 + 4) 2^-24."""
    names, args, _, _ = load()
    n = max(min(len(args[k]['gt_ids']), len(args[k]['pred_ids'])) for k in (names if only is None else only))
    return (n + 4) * 2.0 ** -24


def bound_of(name):
    """The bound a clip is held to: its own for 'caps', that of all the other clips for any other."""
    names = load()[0]
    return reference_bound([name] if name == 'caps' else [k for k in names if k != 'caps'])


def against_reference(got, want, bound):
    """-> the largest relative gap of the float fields; the integer fields must be equal."""
    from romp_amd import tracking_metrics as M
    worst = 0.
    for metric, ints in (('HOTA', M.HOTA_INT), ('CLEAR', M.CLEAR_INT), ('Identity', M.ID_INT)):
        assert set(got[metric]) == set(want[metric]), metric
        for k, w in want[metric].items():
            g, w = np.asarray(got[metric][k], np.float64), np.asarray(w, np.float64)
            if k in ints:
                assert np.array_equal(g, w), (metric, k, g.tolist(), w.tolist())
            else:
                gap = np.abs(g - w)
                assert np.all(gap <= bound * np.abs(w)), (metric, k, g.tolist(), w.tolist())
                worst = max(worst, float(np.max(gap / np.where(w != 0, np.abs(w), 1.))))
    return worst
