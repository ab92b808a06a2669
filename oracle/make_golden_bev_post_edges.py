"""Golden fixture of edge scenes for BEV post-processing, produced by the reference's own functions
(bev/post_parser.py: body_mesh_projection2image, suppressing_redundant_prediction_via_projection, remove_outlier).
Build container only.   python oracle/make_golden_bev_post_edges.py

Every scene is small (at most 4 persons) and named for the one behaviour it shows; the script asserts that behaviour with
the reference before it writes tests/golden/bev_post_edges.npz (per scene: joints, cam, pad -> pj2d_org, cam_trans,
kept_after_nms, kept_final)."""
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

F32 = np.float32
NMS, REL = 20, 1.6
PAD_720 = [280, 1000, 0, 1280, 720, 1280]                       # a 720 x 1280 frame: top > 0
A, B, TINY = [0.6, 0.1, -0.3], [0.5, -0.05, 0.2], [0.1, 0.5, -0.8]    # two ordinary persons; one remote (depth 17 m) and tiny


def make_scenes(seed=0):
    """-> {name: (joints (n,71,3), cam (n,3), pad (6,))}, float32."""
    rs = np.random.RandomState(seed)
    body = lambda: rs.randn(71, 3) * [0.25, 0.45, 0.1]
    near = lambda j: j + 0.002 * rs.randn(71, 3)
    ja, jb, jt = body(), body(), body()
    three = np.stack([ja, jb, jt])
    s = {}
    s['one'] = (ja[None], [[0.6, 0.1, -0.2]], PAD_720)
    s['pair'] = ([ja, near(ja)], [[0.55, 0.1, 0.2], [0.6, 0.103, 0.203]], PAD_720)             # row 0 is the smaller one
    s['tie'] = ([jb, jb], [[0.5, -0.2, 0.3]] * 2, PAD_720)
    s['chain'] = ([ja, ja, ja], [[0.52, 0., -0.05], [0.51, 0., 0.], [0.50, 0., 0.05]], PAD_720)
    s['outlier3'] = (three, [A, B, TINY], PAD_720)
    s['gate_at'] = (three, [A, B, [0.25] + TINY[1:]], PAD_720)
    s['gate_above'] = (three, [A, B, [0.26] + TINY[1:]], PAD_720)
    # A and two near-duplicates of A (both pairs with A are inside the threshold), and the remote person: two survivors
    s['nms_then_few'] = ([ja, jt, near(ja), near(ja)], [A, TINY, [0.58, 0.102, -0.298], [0.57, 0.098, -0.302]], PAD_720)
    # the remote person twice: with both rows present neither is isolated, with the duplicate gone the other one is
    s['survivors_only'] = ([ja, jt, jb, near(jt)], [A, TINY, B, [0.099, 0.5005, -0.7995]], PAD_720)
    s['same_place'] = ([jb, jb + [1., 0, 0], jb + [0, 1., 0]], [[0.2, 0.1, -0.2]] * 3, PAD_720)
    s['portrait'] = (three, [A, B, TINY], [0, 800, 100, 700, 800, 600])                       # left > 0
    s['landscape'] = (three, [A, B, TINY], [80, 560, 0, 640, 480, 640])                       # top > 0
    s['square'] = (three, [A, B, TINY], [0, 512, 0, 512, 512, 512])
    return {k: tuple(np.asarray(v, F32) for v in t) for k, t in s.items()}


def run_reference(pp, joints, cam, pad, suppress=True):
    n = len(cam)
    out = {'joints': torch.from_numpy(joints).clone(), 'cam': torch.from_numpy(cam).clone(), 'params_pred': torch.zeros(n, 146),
           'idx': torch.arange(n)}
    out.update(pp.body_mesh_projection2image(out['joints'], out['cam'], input2org_offsets=torch.from_numpy(pad)))
    res = {'pj2d_org': out['pj2d_org'].clone().numpy(), 'cam_trans': out['cam_trans'].clone().numpy()}
    if suppress:
        out = pp.suppressing_redundant_prediction_via_projection(out, (int(pad[4]), int(pad[5]), 3), thresh=NMS)
    res['kept_after_nms'] = out['idx'].clone().numpy()
    out = pp.remove_outlier(out, relative_scale_thresh=REL)
    res['kept_final'] = out['idx'].clone().numpy()
    return res


EXPECTED = {                                                      # name: (kept after suppression, kept at the end)
    'one': ([0], [0]), 'pair': ([1], [1]), 'tie': ([0], [0]), 'chain': ([0], [0]),
    'outlier3': ([0, 1, 2], [0, 1]), 'gate_at': ([0, 1, 2], [0, 1, 2]), 'gate_above': ([0, 1, 2], [0, 1, 2]),
    'nms_then_few': ([0, 1], [0, 1]), 'survivors_only': ([0, 1, 2], [0, 2]), 'same_place': ([0, 1, 2], [0, 1, 2]),
    'portrait': ([0, 1, 2], [0, 1]), 'landscape': ([0, 1, 2], [0, 1]), 'square': ([0, 1, 2], [0, 1]),
}


if __name__ == '__main__':
    mg._load_reference()
    pp = mg._load_reference_bev()['post_parser']
    scenes = make_scenes()
    data = {'scenes': np.array(list(scenes))}
    for name, (joints, cam, pad) in scenes.items():
        r = run_reference(pp, joints, cam, pad)
        print('%-15s kept after nms %s final %s' % (name, r['kept_after_nms'].tolist(), r['kept_final'].tolist()))
        assert (r['kept_after_nms'].tolist(), r['kept_final'].tolist()) == EXPECTED[name], name
        data.update({name + '_joints': joints, name + '_cam': cam, name + '_pad': pad})
        data.update({name + '_' + k: v for k, v in r.items()})
    # survivors_only: without the suppression the reference's outlier pass keeps the remote rows 1 and 3
    r = run_reference(pp, *scenes['survivors_only'], suppress=False)
    print('survivors_only, suppression off: final', r['kept_final'].tolist())
    assert r['kept_final'].tolist() == [0, 1, 2, 3]
    # gate: at scale_thresh 0.3 the reference removes the remote row of both gate scenes -- the gate alone keeps it
    for name in ('gate_at', 'gate_above'):
        joints, cam, pad = scenes[name]
        out = {'cam': torch.from_numpy(cam), 'params_pred': torch.zeros(3, 146), 'idx': torch.arange(3)}
        out.update(pp.body_mesh_projection2image(torch.from_numpy(joints), out['cam'], input2org_offsets=torch.from_numpy(pad)))
        assert pp.remove_outlier(out, relative_scale_thresh=REL, scale_thresh=0.3)['idx'].tolist() == [0, 1], name
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'bev_post_edges.npz'), **data)
