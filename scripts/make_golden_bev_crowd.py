"""Golden fixture for BEV's crowd mode (tests/golden/bev_crowd.npz), produced by the reference's own
BEV.process_long_image (simple_romp/bev/main.py:184-258) with its own split2process.py / post_parser.py.

Build container only (needs the reference checkout).  bev/main.py's module body is NOT executed (its
default_settings = bev_settings([]) would try to fetch the checkpoint): only the process_long_image FunctionDef is
compiled out of the file's AST and run on a stand-in `self` whose single_image_forward returns recorded synthetic
per-crop detections and whose smpl_parser returns recorded joints / small vertex arrays.

    python scripts/make_golden_bev_crowd.py
"""
import argparse
import ast
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

# (H, W, overlap_ratio, seed, trailing empty crop)
CASES = [(512, 1280, 0.8, 1, False), (720, 2560, 0.8, 2, False), (720, 2560, 0.46, 3, True), (1080, 2160, 0.8, 4, False),
         (512, 1280, 0.46, 5, True)]
NV = 8          # vertices per person (the merge does not read them; they only travel with the rows)


def load_process_long_image():
    ref = mg._load_reference()
    bev = mg._load_reference_bev()
    sp_spec = importlib.util.spec_from_file_location('bev.split2process', os.path.join(mg.REF, 'bev', 'split2process.py'))
    sp = importlib.util.module_from_spec(sp_spec)
    sys.modules['bev.split2process'] = sp
    sp_spec.loader.exec_module(sp)
    path = os.path.join(mg.REF, 'bev', 'main.py')
    tree = ast.parse(open(path).read(), path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'BEV')
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == 'process_long_image')
    fn.decorator_list = []
    mod = ast.Module(body=[fn], type_ignores=[])
    pp = bev['post_parser']
    g = {'__name__': 'bev.main', '__package__': 'bev', 'torch': torch, 'np': np,
         'body_mesh_projection2image': pp.body_mesh_projection2image,
         'suppressing_redundant_prediction_via_projection': pp.suppressing_redundant_prediction_via_projection,
         'remove_outlier': pp.remove_outlier}
    exec(compile(mod, path, 'exec'), g)
    return g['process_long_image'], sp, ref['utils']


def synth(H, W, ov, seed, trailing_empty, sp):
    """Per-crop detections of a few full-frame persons seen by every crop that covers them, plus a near-duplicate inside one
    crop, a remote tiny person (crop-stage outlier) and a remote person in a crop with only two (full-frame outlier)."""
    rs = np.random.RandomState(seed)
    pad_length = int(H * ov)
    crops = sp.get_image_split_plan(np.zeros((H, W + 2 * pad_length, 3), np.uint8), overlap_ratio=ov)
    K = len(crops)
    fb = crops.astype(np.float64).copy()
    fb[:, :2] -= pad_length
    scale = np.maximum(fb[:, 1] - fb[:, 0], fb[:, 3] - fb[:, 2]) / max(H, W)
    shift = fb[:, :2].mean(1) / (W / 2) - 1
    M = max(6, int(round(1.2 * W / H * 2)))
    persons = []
    for p in range(M):
        persons.append({'s': rs.uniform(0.45, 0.85) * H / W * 1.0, 'ty': rs.uniform(-0.3, 0.3) * H / W,
                        'tx': -0.95 + 1.9 * (p + rs.uniform(0.2, 0.8)) / M,
                        'j': (rs.randn(71, 3) * np.array([0.25, 0.45, 0.1])).astype(np.float32)})
    dets = [[] for _ in range(K)]
    for p in persons:
        for c in range(K):
            txc = (p['tx'] - shift[c]) / scale[c]
            if abs(txc) < 1.05:
                cam = np.array([p['s'] / scale[c], p['ty'] / scale[c], txc]) + rs.randn(3) * [0.002, 0.002, 0.004]
                dets[c].append((cam, p['j'] + rs.randn(71, 3).astype(np.float32) * 0.01, rs.uniform(0.1, 0.9)))
    c = K // 2                                                          # near-duplicate inside one crop
    cam, j, _ = dets[c][0]
    dets[c].append((cam + [0.01, 0.001, 0.002], j + 0.005, rs.uniform(0.1, 0.9)))
    c = K // 3                                                          # remote tiny person: crop-stage outlier
    dets[c].append((np.array([0.04, 0.1, 0.0]), persons[0]['j'], 0.5))
    if trailing_empty:
        dets[K - 1] = []
    else:                                                               # last crop: two persons, one remote (crop stage skips N < 3)
        dets[K - 1] = dets[K - 1][:1] + [(np.array([0.05, -0.2, 0.1]), persons[1]['j'], 0.6)]
    for c in range(K - (1 if trailing_empty else 0)):                   # (the reference raises on an empty crop before a full one)
        if not dets[c]:
            dets[c].append((np.array([0.5, 0.05, rs.uniform(-0.2, 0.2)]), persons[2]['j'], rs.uniform(0.1, 0.9)))
    rows = []
    for c in range(K):
        for cam, j, conf in dets[c]:
            rows.append((c, np.asarray(cam, np.float32), j.astype(np.float32), np.float32(conf)))
    return crops, rows


def run_case(H, W, ov, seed, trailing_empty, process_long_image, sp, utils):
    crops_plan, rows = synth(H, W, ov, seed, trailing_empty, sp)
    N = len(rows)
    rs = np.random.RandomState(100 + seed)
    crop_id = np.array([r[0] for r in rows], np.int32)
    cam = np.stack([r[1] for r in rows])
    joints = np.stack([r[2] for r in rows])
    conf = np.array([r[3] for r in rows], np.float32)
    verts = (rs.randn(N, NV, 3) * 0.3).astype(np.float32)
    params = rs.randn(N, 146).astype(np.float32)
    thetas, betas = rs.randn(N, 72).astype(np.float32), rs.randn(N, 11).astype(np.float32)
    rec = {'crops': [], 'pads': [], 'shapes': []}

    class Stub:
        pass

    self = Stub()
    self.settings = argparse.Namespace(overlap_ratio=ov, nms_thresh=20, relative_scale_thresh=1.6, center_thresh=0.08,
                                       render_mesh=False, renderer='sim3dr')
    state = {'cid': 0}

    def single_image_forward(img):
        c = state['cid']
        state['cid'] += 1
        rec['shapes'].append(img.shape[:2])
        rec['pads'].append(utils.padding_image(img)[1].numpy())
        sel = np.nonzero(crop_id == c)[0]
        if len(sel) == 0:
            return None, None
        t = lambda a: torch.from_numpy(a[sel].copy())
        out = {'smpl_thetas': t(thetas), 'smpl_betas': t(betas), 'cam': t(cam), 'params_pred': t(params),
               'center_confs': t(conf), 'pred_batch_ids': torch.zeros(len(sel), dtype=torch.long),
               'idx': torch.from_numpy(sel.astype(np.int64))}
        out['cam_trans'] = sys.modules['bev.post_parser'].denormalize_cam_params_to_trans(out['cam'])
        state['last'] = sel
        return out, None

    def smpl_parser(b, th):
        sel = state['last']
        return torch.from_numpy(verts[sel].copy()), torch.from_numpy(joints[sel].copy()), torch.zeros(1, 3)

    self.single_image_forward = single_image_forward
    self.smpl_parser = smpl_parser
    orig_plan = sp.get_image_split_plan

    def plan(image, overlap_ratio=0.46):
        boxes = orig_plan(image, overlap_ratio=overlap_ratio)
        rec['crops'] = boxes.copy()
        return boxes

    sp.get_image_split_plan = plan
    try:
        out = process_long_image(self, np.zeros((H, W, 3), np.uint8))
    finally:
        sp.get_image_split_plan = orig_plan
    assert np.array_equal(rec['crops'], crops_plan)
    _, pad_info, pad_length = sp.padding_image_overlap(np.zeros((H, W, 3), np.uint8), overlap_ratio=ov)
    kept = out['idx'].numpy()
    print('%dx%d ov %.2f: K %d, rows %d, kept %d' % (H, W, ov, len(crops_plan), N, len(kept)))
    return {'H': H, 'W': W, 'overlap': ov, 'pad_length': pad_length, 'crops': rec['crops'].astype(np.int32),
            'crop_shapes': np.array(rec['shapes'], np.int32), 'crop_pads': np.stack(rec['pads']).astype(np.float32),
            'pad_info': pad_info.numpy().astype(np.float32), 'crop_id': crop_id, 'cam': cam, 'joints': joints,
            'center_confs': conf, 'kept': kept.astype(np.int64), 'cam_full': out['cam'].numpy(),
            'cam_trans': out['cam_trans'].numpy(), 'pj2d_org': out['pj2d_org'].numpy()}


if __name__ == '__main__':
    process_long_image, sp, utils = load_process_long_image()
    arrays = {}
    for i, case in enumerate(CASES):
        for k, v in run_case(*case, process_long_image, sp, utils).items():
            arrays['c%d_%s' % (i, k)] = np.asarray(v)
    arrays['n_cases'] = np.array(len(CASES))
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'bev_crowd.npz'), **arrays)
