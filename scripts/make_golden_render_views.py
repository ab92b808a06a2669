"""Golden fixture for the bird / side mesh views (tests/golden/render_views.npz), produced by the reference's own
simple_romp/vis_human/main.py:rendering_romp_bev_results with items mesh,mesh_bird_view,mesh_side_view and its own
vis_utils.rotate_view_weak_perspective, driving the reference Sim3DR (renderer.py + its C++ rasterizer compiled into
oracle/_ref, through oracle/make_golden_sim3dr.load_reference_renderer).  cv2 is replaced by an empty stub module: the
sim3dr branch never calls it.

Build container only (needs the reference checkout):

    make -C oracle && python scripts/make_golden_render_views.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sim3dr_oracle as SO  # noqa: E402
from oracle.make_golden_sim3dr import load_reference_renderer  # noqa: E402

VIS = '/root/reference/simple_romp/vis_human'
# (name, h, w, persons, seed)
CASES = [('wide', 120, 260, 4, 1), ('tall', 150, 96, 3, 2)]


def load_reference_vis():
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    pkg = types.ModuleType('vis_human')
    pkg.__path__ = [VIS]
    sys.modules['vis_human'] = pkg
    mods = {}
    for name in ('vis_utils', 'main'):
        spec = importlib.util.spec_from_file_location('vis_human.' + name, os.path.join(VIS, name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules['vis_human.' + name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods['main'], mods['vis_utils']


def make_case(h, w, n, seed):
    """n ellipsoid 'persons' in camera space (verts + cam_trans) whose bird / side footprints overlap, plus their
    image-space meshes (verts_camed_org) for the frame panel."""
    rs = np.random.RandomState(seed)
    base, tri = SO.ellipsoid_mesh(10, 14, [0, 0, 0], [1, 1, 1])
    verts, org = [], []
    trans = np.stack([rs.uniform(-0.6, 0.6, n), rs.uniform(-0.2, 0.2, n), rs.uniform(4.0, 6.0, n)], 1)
    for i in range(n):
        r = np.array([rs.uniform(0.2, 0.35), rs.uniform(0.7, 0.9), rs.uniform(0.15, 0.3)])
        v = base * r[None] + rs.normal(0, 0.01, base.shape)
        verts.append(v.astype(np.float32))
        c = [rs.uniform(0.25, 0.75) * w, rs.uniform(0.3, 0.7) * h, rs.uniform(-20, 20)]
        org.append((base * np.array([0.15 * w, 0.3 * h, 20])[None] + np.array(c)[None]).astype(np.float32))
    frame = np.full((h, w, 3), 96, np.uint8)                 # flat with two blocks: the fixture stays small
    frame[h // 4:h // 2, w // 5:w // 2] = (30, 200, 120)
    frame[h // 2:, w // 2:] = (220, 60, 10)
    return np.stack(verts), trans.astype(np.float32), np.stack(org), tri, frame


def main():
    ref_main, ref_vu = load_reference_vis()
    renderer = load_reference_renderer().Sim3DR()
    data = {}
    for name, h, w, n, seed in CASES:
        verts, trans, org, tri, frame = make_case(h, w, n, seed)
        outputs = {'smpl_face': torch.from_numpy(tri.astype(np.int64)), 'cam_trans': torch.from_numpy(trans),
                   'verts': torch.from_numpy(verts), 'verts_camed_org': torch.from_numpy(org)}
        cfgs = {'mesh_color': 'identity', 'items': ['mesh', 'mesh_bird_view', 'mesh_side_view'], 'renderer': 'sim3dr'}
        res = ref_main.rendering_romp_bev_results(renderer, dict(outputs), frame.copy(), cfgs)
        img = res['rendered_image']
        assert img.shape == (h, w + w + 2 * h, 3), img.shape
        # the transformed vertices / centre / scale of both views, from the reference's own function on the same input
        order = torch.sort(torch.from_numpy(trans)[:, 2], descending=True).indices.numpy()
        vt = (torch.from_numpy(verts) + torch.from_numpy(trans).unsqueeze(1))[order]
        vt[:, :, 2] = vt[:, :, 2] * -1
        bird, bc, bs = ref_vu.rotate_view_weak_perspective(vt, rx=-90, ry=0, img_shape=(h, h), expand_ratio=1.2)
        side, sc, ss = ref_vu.rotate_view_weak_perspective(vt, rx=0, ry=-90, img_shape=(h, w), expand_ratio=1.2)
        for k, v in dict(verts=verts, cam_trans=trans, verts_camed_org=org, frame=frame, verts_tran=vt.numpy(),
                         bird_verts=bird.numpy(), bird_center=bc.reshape(3).numpy(), bird_scale=np.float32(bs.item()),
                         side_verts=side.numpy(), side_center=sc.reshape(3).numpy(), side_scale=np.float32(ss.item()),
                         rendered_image=img).items():
            data['%s_%s' % (name, k)] = v
        painted = [int((img[:, w + w + i * h:w + w + (i + 1) * h] != 255).any(2).sum()) for i in range(2)]
        print(name, h, w, 'persons', n, 'bird / side painted px', painted)
    data['triangles'] = tri.astype(np.int32)
    out = os.path.join(ROOT, 'tests', 'golden', 'render_views.npz')
    np.savez_compressed(out, **data)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
