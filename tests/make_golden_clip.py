"""Writes tests/golden/clip_accel.npz: one chain of 7 frames x 14 joints with what the reference's acceleration metrics return.

    PYTHONDONTWRITEBYTECODE=1 python tests/make_golden_clip.py /path/to/romp/lib/evaluation/evaluation_matrix.py

The module is imported by path and its compute_accel / compute_error_accel are called as they are (evaluation_matrix.py:424-465).
A second path may name simple_romp/trace2/evaluation/eval_3DPW.py, whose compute_error_accel_np stands in when the first module
does not import; the arrays then carry no 'accel'.  Stored: the inputs joints, gt (7,14,3) float32 and vis (4,7) uint8 -- all
visible, the first frame hidden, a middle one, the last one -- and the outputs accel (5,), error (5,) without vis, and
error_vis<k> for each row k of vis (as many entries as the mask keeps), float64 as the reference returns them; 'source' names
the module used."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(path):
    spec = importlib.util.spec_from_file_location('reference_accel', path)
    mod = importlib.util.module_from_spec(spec)
    here = os.path.dirname(path)
    sys.path[:0] = [here, os.path.dirname(here)]                  # the module's own imports (config, constants) live beside it
    try:
        spec.loader.exec_module(mod)
    finally:
        del sys.path[:2]
    return mod


def inputs():
    """-> joints, gt (7,14,3) float32: a smooth seeded motion and a noisy copy; vis (4,7) uint8."""
    rs = np.random.RandomState(7)
    t = np.linspace(0., 1., 7)[:, None, None]
    base = rs.randn(1, 14, 3)
    gt = (base + t * rs.randn(1, 14, 3) + 0.3 * np.sin(3 * t) * rs.randn(1, 14, 3)).astype(np.float32)
    joints = (gt + 0.05 * rs.randn(7, 14, 3)).astype(np.float32)
    vis = np.ones((4, 7), np.uint8)
    vis[1, 0] = vis[2, 3] = vis[3, 6] = 0
    return joints, gt, vis


def main(paths):
    sys.dont_write_bytecode = True
    joints, gt, vis = inputs()
    out = {'joints': joints, 'gt': gt, 'vis': vis}
    accel = error = None
    for path in paths:
        try:
            mod = load(path)
        except Exception as e:                                    # a dependency of the module that is not installed here
            print('cannot import %s: %r' % (path, e))
            continue
        if hasattr(mod, 'compute_error_accel'):
            accel, error = mod.compute_accel, mod.compute_error_accel
        elif hasattr(mod, 'compute_error_accel_np'):
            error = mod.compute_error_accel_np
        else:
            continue
        out['source'] = np.asarray(os.path.basename(path), dtype=np.str_)
        break
    assert error is not None, 'neither module could be imported'
    if accel is not None:
        out['accel'] = np.asarray(accel(joints.astype(np.float64)), np.float64)
    out['error'] = np.asarray(error(gt.astype(np.float64), joints.astype(np.float64)), np.float64)
    for k in range(4):
        out['error_vis%d' % k] = np.asarray(error(gt.astype(np.float64), joints.astype(np.float64), vis[k].astype(bool)), np.float64)
    path = os.path.join(ROOT, 'tests', 'golden', 'clip_accel.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main(sys.argv[1:])
