"""Golden fixture for the BEV head's edge cases, produced by the reference's own functions: CenterMap3D.parse_3dcentermap
(bev/post_parser.py:44-66) on planted-peak volumes, convert_cam_params_to_centermap_coords + denormalize_center
(bev/model.py:89-102) and denormalize_cam_params_to_trans (bev/post_parser.py:109-128) on crafted camera triples.
Inputs come from oracle/bev_kernels_ref.py (edge_parse_cases, edge_cams): tie-free, so the reference's answer is defined.
The parse inputs are stored as (seed, background, peak list), never as volumes.  Build container only; does nothing where
the reference is absent.   python oracle/make_golden_bev_edges.py"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location('mg', os.path.join(ROOT, 'oracle', 'make_golden.py'))
mg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mg)


if __name__ == '__main__':
    if not os.path.isdir(os.path.join(mg.REF, 'bev')):
        print('reference not present: nothing written')
        sys.exit(0)
    from oracle import bev_kernels_ref as K
    mg._load_reference()
    bev = mg._load_reference_bev()
    pp, model = bev['post_parser'], bev['model']
    out = {}
    cams = K.edge_cams()
    anchor = torch.from_numpy(model.get_cam3dmap_anchor(60, 128)).float()                      # as BEVv1.__init__ :127
    c = torch.from_numpy(cams)
    out['cams'] = cams
    out['cam_czyx'] = model.denormalize_center(model.convert_cam_params_to_centermap_coords(c.clone(), anchor), size=128).numpy()
    out['cam_trans'] = pp.denormalize_cam_params_to_trans(c.clone()).numpy()
    names = []
    for name, case in K.edge_parse_cases().items():
        parser = pp.CenterMap3D(conf_thresh=case['thresh'])
        parser.max_person = case['max_person']
        cm = K.planted_volume(case['B'], case['seed'], case['peaks'], case['background'])
        with torch.no_grad():
            bids, czyx, confs = parser.parse_3dcentermap(cm)
        names.append(name)
        out[f'parse_{name}_meta'] = np.array([case['B'], case['seed'], case['background'][0], case['background'][1],
                                              case['thresh'], case['max_person']], np.float64)
        out[f'parse_{name}_peaks'] = np.array(case['peaks'], np.float64)
        out[f'parse_{name}_bids'] = bids.numpy().astype(np.int64)
        out[f'parse_{name}_czyx'] = czyx.numpy().astype(np.int64)
        out[f'parse_{name}_confs'] = confs.numpy().astype(np.float32)
        print(name, 'detections', len(bids))
    path = os.path.join(ROOT, 'tests', 'golden', 'bev_edges.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes; parse cases', names)
