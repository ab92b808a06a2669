"""Writes tests/golden/fit_scene.npz: depths, depth-layer labels and image ids of 26 rows with what the reference's own
relative_depth_loss (romp/lib/loss_funcs/relative_loss.py:46-99) returns for them, for both depth_loss_type values.

    python scripts/make_golden_fit_scene.py [path of the reference checkout, default /root/reference]

The module is imported by file path with `config`, `constants` and `utils.cam_utils` stubbed (config.args() carries
depth_loss_type and nothing else).  No test runs this script; tests/test_fit_scene.py reads the file.

Keys: z (N,) float64, ids (N,) int64 (-1 = unlabelled), frames (N,) int64, thresh; for kind in ('Piecewise', 'Log'):
scalar_<kind> (the function's result over all rows), grad_<kind> (N,) (its gradient in z, by autograd), image_<kind> (F,)
(the function's result on the rows of one image alone: that image's mean, 0 where the image has no active pair).
The images: 0 one labelled row; 1 two; 2 three and an unlabelled one; 3 six; 4 three of one layer; 5 two rows in the right
order beyond the margin (no active pair under Piecewise); 6 and 7 interleaved row by row; 8 a lone unlabelled row."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
THRESH = 0.3


def load_reference(root, settings):
    cfg = types.ModuleType('config')
    cfg.args = lambda: settings
    cam_utils = types.ModuleType('utils.cam_utils')
    cam_utils.convert_scale_to_depth = None
    utils = types.ModuleType('utils')
    utils.cam_utils = cam_utils
    stubs = {'config': cfg, 'constants': types.ModuleType('constants'), 'utils': utils, 'utils.cam_utils': cam_utils}
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location('reference_relative_loss', os.path.join(root, 'romp', 'lib', 'loss_funcs', 'relative_loss.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def inputs():
    g = torch.Generator().manual_seed(2024)
    rnd = lambda n: (2.0 + 3.0 * torch.rand(n, generator=g, dtype=torch.float64)).tolist()
    rows = []                                                        # (frame, id, z)
    rows += [(0, 2, 3.1)]
    rows += [(1, 1, 2.5), (1, 0, 4.0)]                               # the smaller id lies deeper: violated
    rows += [(2, i, z) for i, z in zip([0, -1, 2, 1], rnd(4))]
    rows += [(3, i, z) for i, z in zip([3, 0, 1, 1, 2, 0], rnd(6))]
    rows += [(4, 1, z) for z in rnd(3)]
    rows += [(5, 0, 1.0), (5, 1, 3.0)]
    for i, z in zip([0, 1, 2, 0, 1, 1, 2, 0], rnd(8)):               # images 6 and 7 alternate
        rows.append((6 + len(rows) % 2, i, z))
    rows += [(8, -1, 2.2)]
    frames, ids, z = zip(*rows)
    return np.array(z, np.float64), np.array(ids, np.int64), np.array(frames, np.int64)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    settings = types.SimpleNamespace(depth_loss_type='Piecewise')
    ref = load_reference(root, settings)
    z, ids, frames = inputs()
    out = {'z': z, 'ids': ids, 'frames': frames, 'thresh': np.float64(THRESH),
           'source': np.array('relative_depth_loss, romp/lib/loss_funcs/relative_loss.py:46-99')}
    n_frames = int(frames.max()) + 1
    for kind in ('Piecewise', 'Log'):
        settings.depth_loss_type = kind
        zt = torch.tensor(z, requires_grad=True)
        scalar = ref.relative_depth_loss(zt, torch.tensor(ids), torch.tensor(frames), dist_thresh=THRESH)
        scalar.backward()
        per_image = np.zeros(n_frames)
        for f in range(n_frames):
            keep = frames == f
            v = ref.relative_depth_loss(torch.tensor(z[keep]), torch.tensor(ids[keep]), torch.tensor(frames[keep]), dist_thresh=THRESH)
            per_image[f] = float(v)
        out['scalar_' + kind], out['grad_' + kind], out['image_' + kind] = np.float64(float(scalar.detach())), zt.grad.numpy().copy(), per_image
        print(kind, float(scalar.detach()), per_image)
    path = os.path.join(HERE, '..', 'tests', 'golden', 'fit_scene.npz')
    np.savez(path, **out)
    print('wrote', os.path.normpath(path), os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
