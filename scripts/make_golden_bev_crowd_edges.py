"""Golden fixture for the crafted crowd-merge cases (tests/golden/bev_crowd_edges.npz): the rows that survive each stage of the
merge according to the reference's own stage functions -- bev/split2process.py's exclude_boudary_subjects and
convert_crop_cam_params2full_image, bev/post_parser.py's body_mesh_projection2image,
suppressing_redundant_prediction_via_projection (conf_based=True) and remove_outlier -- on the `ties`, `counts`, `bounds` and
`nonfinite` inputs of tests/crowd_cases.py.

Build container only (needs the reference checkout).  The functions are called stage by stage, in process_long_image's order
(bev/main.py:208-256), because process_long_image itself raises on an empty crop before a full one; each crop is projected with
its own shape.  A stage function that raises on a case is recorded (`<case>/raised`), not worked around.

    python scripts/make_golden_bev_crowd_edges.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
spec = importlib.util.spec_from_file_location('mg', os.path.join(ROOT, 'oracle', 'make_golden.py'))
mg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mg)
import crowd_cases as CC  # noqa: E402

STAGES = ('excluded', 'crop_suppressed', 'crop_outliers', 'suppressed', 'outliers')


def load_reference():
    mg._load_reference()
    pp = mg._load_reference_bev()['post_parser']
    sp_spec = importlib.util.spec_from_file_location('bev.split2process', os.path.join(mg.REF, 'bev', 'split2process.py'))
    sp = importlib.util.module_from_spec(sp_spec)
    sys.modules['bev.split2process'] = sp
    sp_spec.loader.exec_module(sp)
    return pp, sp


def _alive(outs):
    return np.sort(np.concatenate([o['idx'].numpy() for o in outs if o is not None] + [np.zeros(0, np.int64)]))


def run_case(case, pp, sp):
    """-> {stage: rows alive after it}, the final survivors' cam / cam_trans / pj2d_org."""
    H, W, K, crops = case['H'], case['W'], case['K'], case['crops'].copy()
    outs = []
    for c in range(K):
        sel = np.nonzero(case['crop_id'] == c)[0]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel]))
        outs.append(None if len(sel) == 0 else {'cam': t(case['cam']), 'joints': t(case['joints']), 'center_confs': t(case['conf']),
                                               'params_pred': torch.zeros(len(sel), 1), 'idx': torch.from_numpy(sel.astype(np.int64))})
    shapes = [(int(b - t), int(r - l)) for l, r, t, b in crops]
    alive = {}
    for cid in range(K):                                                # the right of this crop, then its own projection
        o = outs[cid]
        if o is None:
            continue
        if cid != K - 1:
            sp.exclude_boudary_subjects(o, (crops[cid, 1] - crops[cid + 1, 0]) / H / 2, ptype='left', torlerance=0)
        ch, cw = shapes[cid]
        o.update(pp.body_mesh_projection2image(o['joints'], o['cam'], input2org_offsets=torch.Tensor([0, ch, 0, cw, ch, cw])))
    for cid in range(1, K - 1):                                         # the left of the next crop
        if outs[cid + 1] is not None:
            sp.exclude_boudary_subjects(outs[cid + 1], (crops[cid, 1] - crops[cid + 1, 0]) / H / 2, ptype='right', torlerance=0)
    alive['excluded'] = _alive(outs)
    for cid in range(K):
        if outs[cid] is not None:
            outs[cid] = pp.suppressing_redundant_prediction_via_projection(outs[cid], list(shapes[cid]), thresh=case['nms'],
                                                                           conf_based=True)
    alive['crop_suppressed'] = _alive(outs)
    for cid in range(K):
        if outs[cid] is not None:
            outs[cid] = pp.remove_outlier(outs[cid], scale_thresh=1, relative_scale_thresh=case['rel'])
    alive['crop_outliers'] = _alive(outs)
    merged = {}
    for cid in range(K):
        o = outs[cid]
        if o is None:
            continue
        box = crops[cid].copy()
        box[:2] -= case['pad_length']
        o['cam'] = sp.convert_crop_cam_params2full_image(o['cam'], box, (H, W))
        for k in ('pj2d', 'pj2d_org', 'cam_trans'):
            o.pop(k, None)
        sp.collect_outputs(o, merged)
    _, pad_info, _ = sp.padding_image_overlap(np.zeros((H, W, 3), np.uint8), overlap_ratio=0.5)
    merged.update(pp.body_mesh_projection2image(merged['joints'], merged['cam'], input2org_offsets=pad_info))
    merged = pp.suppressing_redundant_prediction_via_projection(merged, (H, W, 3), thresh=case['nms'], conf_based=True)
    alive['suppressed'] = np.sort(merged['idx'].numpy())
    merged = pp.remove_outlier(merged, scale_thresh=0.5, relative_scale_thresh=case['rel'])
    alive['outliers'] = np.sort(merged['idx'].numpy())
    assert np.array_equal(alive['outliers'], merged['idx'].numpy())      # (crop order is row order)
    return alive, merged


if __name__ == '__main__':
    pp, sp = load_reference()
    arrays, names = {}, []
    for builder in CC.FIXTURE:
        for case in CC.cases(builder):
            n = case['name']
            names.append(n)
            for k in ('cam', 'conf', 'crop_id', 'crops'):                # (the inputs the sets belong to; joints by their sum)
                arrays['%s/%s' % (n, k)] = case[k]
            arrays[n + '/joints_sum'] = np.nansum(np.where(np.isfinite(case['joints']), case['joints'], 0).astype(np.float64))
            try:
                alive, merged = run_case(case, pp, sp)
            except Exception as e:                                      # the reference cannot take this case: recorded as such
                arrays[n + '/raised'] = np.array(type(e).__name__ + ': ' + str(e)[:200])
                print('%-32s raised %s: %s' % (n, type(e).__name__, e))
                continue
            for s in STAGES:
                arrays['%s/alive_%s' % (n, s)] = alive[s].astype(np.int32)
            arrays[n + '/cam_full'] = merged['cam'].numpy()
            arrays[n + '/cam_trans'] = merged['cam_trans'].numpy()
            arrays[n + '/pj2d_org'] = merged['pj2d_org'].numpy()
            print('%-32s N %2d alive %s' % (n, case['N'], [len(alive[s]) for s in STAGES]))
    arrays['names'] = np.array(names)
    path = os.path.join(ROOT, 'tests', 'golden', 'bev_crowd_edges.npz')
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), 'bytes')
