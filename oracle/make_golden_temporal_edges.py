"""tests/golden/temporal_edges.npz from THE REFERENCE: simple_romp/romp/utils.py create_OneEuroFilter + smooth_results (imported by
file path with an empty cv2 stub) run over the root-rotation edge cases of tests/temporal_cases.py with smooth_coeff 3 and 16 betas.
Per case: the reference's thetas / betas / cam per frame -- recorded numbers only.  Needs /root/reference."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import temporal_cases as TC  # noqa: E402
from oracle import temporal_oracle as TO  # noqa: E402

COEFF = 3.0


def main():
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    spec = importlib.util.spec_from_file_location('ref_romp_utils', '/root/reference/simple_romp/romp/utils.py')
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    out, worst = {}, 0.0
    for c in TC.cases():
        filters, mine = ru.create_OneEuroFilter(COEFF), TO.make_filters(COEFF)
        rows = [], [], []
        for th, be, ca in zip(c['thetas'], c['betas'], c['cam']):
            th, be, ca = (torch.from_numpy(v.copy()) for v in (th, be, ca))
            got = ru.smooth_results(filters, th.clone(), be.clone(), ca.clone())
            own = TO.smooth(mine, th.clone(), be.clone(), ca.clone())
            for a, r, dst in zip(own, got, rows):
                assert torch.equal(torch.isnan(a), torch.isnan(r)), c['name']
                d = ((a - r).abs() / r.abs().clamp(min=1))[~torch.isnan(r)]
                worst = max(worst, float(d.max()))
                assert d.max() < 2e-6, (c['name'], float(d.max()))
                dst.append(r.numpy().astype(np.float32))
        for key, src in zip(('thetas', 'betas', 'cam'), rows):
            out['%s/%s' % (c['name'], key)] = np.stack(src)
    path = os.path.join(ROOT, 'tests', 'golden', 'temporal_edges.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes; the float32 oracle is within %.2e of the reference' % worst)


if __name__ == '__main__':
    main()
