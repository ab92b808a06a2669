"""Golden fixture for the per-person kernels' edge cases, produced by the reference's own functions: SMPL.forward
(smpl.py:62-108), batch_orth_proj (utils.py:309-315), convert_cam_to_3d_trans (utils.py:303-307), estimate_translation with
cv2 absent (utils.py:391-434), convert_proejection_from_input_to_orgimg (post_parser.py:81-88) and BEV's
perspective_projection (bev/post_parser.py:68-107).  Inputs come from oracle/body_kernels_ref.py and are not stored: the
tests draw them again from the same seeds.  Of every mesh only the vertex subset K.fixture_vertices is kept, and all 71
joints.  Build container only; does nothing where the reference is absent.   python oracle/make_golden_body_edges.py"""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location('mg', os.path.join(ROOT, 'oracle', 'make_golden.py'))
mg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mg)


if __name__ == '__main__':
    if not os.path.isdir(os.path.join(mg.REF, 'romp')):
        print('reference not present: nothing written')
        sys.exit(0)
    from oracle import body_kernels_ref as K
    from oracle import romp_oracle as O
    ref = mg._load_reference()
    bev = mg._load_reference_bev()
    U, PP = ref['utils'], ref['post_parser']
    out = {}
    T = torch.from_numpy
    # ---- SMPL, its own tree, both model types, with and without root alignment
    for nb, tag in ((10, 'smpl'), (11, 'smpla')):
        model = O.make_synthetic_smpl(seed=0, n_betas=nb)
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, 'm.pth')
            torch.save(model, path)
            smpl = ref['smpl'].SMPL(path, model_type=tag)
        be, po, _ = K.smpl_edge_batch(nb)
        vi = K.fixture_vertices(model)
        for ra in (False, True):
            v, j, _ = smpl(T(be), T(po), root_align=ra)
            out[f'{tag}_verts_ra{int(ra)}'] = v.numpy()[:, vi]
            out[f'{tag}_joints_ra{int(ra)}'] = j.numpy()
            assert np.isfinite(v.numpy()).all() and np.isfinite(j.numpy()).all()
        out[f'{tag}_vertex_index'] = vi
    # ---- projection: joints / vertices, every pad layout
    rs = np.random.RandomState(6000)
    joints = rs.randn(5, 71, 3).astype(np.float32)
    verts = rs.randn(5, 301, 3).astype(np.float32)
    cams = K.edge_cams(5)
    out['cam_trans'] = U.convert_cam_to_3d_trans(T(cams)).numpy()
    for name, pad in K.PADS.items():
        padt = torch.Tensor(list(pad))
        pj = U.batch_orth_proj(T(joints), T(cams), mode='2d')
        out[f'pj2d_{name}'] = pj.numpy().copy()
        out[f'pj2d_org_{name}'] = PP.convert_proejection_from_input_to_orgimg(pj.clone(), padt).numpy()
        vc = U.batch_orth_proj(T(verts), T(cams), mode='3d', keep_dim=True)
        out[f'verts_camed_{name}'] = vc.numpy().copy()
        out[f'verts_camed_org_{name}'] = PP.convert_proejection_from_input_to_orgimg(vc.clone(), padt).numpy()
        tr = K.bev_trans(5)
        pv = bev['post_parser'].perspective_projection(T(verts).clone(), translation=T(tr), focal_length=443.4, normalize=True)
        pv = torch.cat([pv, T(verts)[:, :, [2]]], -1)
        out[f'bev_verts_camed_org_{name}'] = bev['post_parser'].convert_proejection_from_input_to_orgimg(pv, padt).numpy()
    # ---- convert_cam_to_3d_trans on the scale edges (weight 2 and 1)
    c = K.cam_to_trans_cams(257)
    out['cam_to_trans_w2'] = U.convert_cam_to_3d_trans(T(c), 2.).numpy()
    out['cam_to_trans_w1'] = U.convert_cam_to_3d_trans(T(c), 1.).numpy()
    # ---- estimate_translation (cv2 is a stub: the reference falls through to its own least squares)
    X, pj = K.lsq_recovery_case(9)
    for Kj in (2, 4, 24, 64, 65, 71):
        out[f'lsq_recovery_K{Kj}'] = U.estimate_translation(X[:, :Kj], K.px(pj, Kj), focal_length=443.4, img_size=np.array([512, 512])).numpy()
    X, pj = K.lsq_edge_cases()
    res, raised = np.zeros((len(X), 3), np.float32), np.zeros(len(X), np.int64)
    for i, name in enumerate(K.LSQ_EDGE_NAMES):
        try:
            res[i] = U.estimate_translation(X[i:i + 1, :24], K.px(pj[i:i + 1], 24), focal_length=443.4, img_size=np.array([512, 512])).numpy()[0]
        except Exception as e:                                   # the singular system: np.linalg.solve raises
            raised[i], res[i] = 1, np.nan
            print(name, 'raised', type(e).__name__, e)
    out['lsq_edges'], out['lsq_edges_raised'] = res, raised
    path = os.path.join(ROOT, 'tests', 'golden', 'body_edges.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')
