"""Latency of rendering one 720x1280 frame (rendering_romp_bev_results) with items `mesh` and
`mesh,mesh_bird_view,mesh_side_view`, N SMPL-sized meshes (6890 vertices, 13776 faces): the batched renderer
(romp_sim3dr_render_batch, one set of launches per panel) against the per-person loop it replaced (per mesh:
normals, light, key memset, raster, resolve through romp_sim3dr_normals / _light / _rasterize).  Median of --calls
calls after --warmup, wall clock, each call ending with the panels downloaded.

    python scripts/render_views_latency.py [--out profiles/render_views_latency.txt]
    python scripts/render_views_latency.py --trace N     # one batched render of all three panels (for rocprofv3)
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sim3dr_oracle as SO  # noqa: E402
from romp_amd import renderer as R  # noqa: E402
from romp_amd.vis import rendering_romp_bev_results  # noqa: E402

H, W = 720, 1280
ITEMS = {'mesh': ['mesh'], 'mesh,bird,side': ['mesh', 'mesh_bird_view', 'mesh_side_view']}


class PerPersonSim3DR(R.Sim3DR):
    """The previous Sim3DR.__call__: one normals / light / rasterize sequence per mesh."""

    def __call__(self, verts_list, triangles, bg, mesh_colors=np.array([[1, 0.6, 0.4]])):
        dev = R._device(self.device)
        img = bg.to(dev).clone() if torch.is_tensor(bg) else torch.from_numpy(np.ascontiguousarray(bg)).to(dev)
        keys = torch.empty(img.shape[0] * img.shape[1], dtype=torch.int64, device=dev)
        verts_dev = verts_list.to(dev, torch.float32).contiguous()
        light = torch.empty_like(verts_dev[0])
        topo = R._topology(triangles, verts_dev.shape[1], dev)
        for ind in range(len(verts_dev)):
            self._render_dev(img, verts_dev[ind], topo, np.asarray(mesh_colors)[[ind % len(mesh_colors)]], keys, light)
        return img.cpu().numpy()


def make_outputs(n, dev, seed=0):
    rs = np.random.RandomState(seed)
    base, tri = SO.ellipsoid_mesh(84, 82, [0, 0, 0], [1, 1, 1])
    faces = np.concatenate([tri, tri[:13776 - len(tri)]]).astype(np.int64)   # SMPL's face count; no vertex of huge valence
    verts = np.zeros((n, 6890, 3), np.float32)
    verts[:, :len(base)] = base[None] * np.stack([rs.uniform(0.2, 0.35, n), rs.uniform(0.7, 0.9, n), rs.uniform(0.15, 0.3, n)], 1)[:, None]
    trans = np.stack([rs.uniform(-2, 2, n), rs.uniform(-0.5, 0.5, n), rs.uniform(4, 12, n)], 1).astype(np.float32)
    p = verts + trans[:, None]
    org = np.stack([p[..., 0] / p[..., 2] * 443.4 + W / 2, p[..., 1] / p[..., 2] * 443.4 + H / 2, verts[..., 2] * 300], -1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {'smpl_face': t(faces), 'cam_trans': t(trans), 'verts': t(verts), 'verts_camed_org': t(org.astype(np.float32))}


def time_calls(renderer, outputs, frame, items, warmup, calls):
    cfgs = {'mesh_color': 'identity', 'items': items, 'renderer': 'sim3dr'}
    for _ in range(warmup):
        rendering_romp_bev_results(renderer, dict(outputs), frame, cfgs)
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rendering_romp_bev_results(renderer, dict(outputs), frame, cfgs)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--trace', type=int, default=0, help='render N meshes once, all items, batched only')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    frame = np.random.RandomState(1).randint(0, 256, (H, W, 3)).astype(np.uint8)
    if a.trace:
        out = make_outputs(a.trace, dev)
        cfgs = {'mesh_color': 'identity', 'items': ITEMS['mesh,bird,side'], 'renderer': 'sim3dr'}
        img = rendering_romp_bev_results(R.Sim3DR(), out, frame, cfgs)['rendered_image']
        torch.cuda.synchronize()
        print('traced N=%d, rendered_image %s' % (a.trace, img.shape))
        return
    lines = ['# rendering_romp_bev_results, one %dx%d frame, median of %d calls after %d warm-up, ms (%s)'
             % (H, W, a.calls, a.warmup, torch.cuda.get_device_name(0)),
             '# batched: romp_sim3dr_render_batch per panel; per-person: the previous loop (5 launches + host light config per mesh)',
             '%-16s %4s %12s %14s %8s' % ('items', 'N', 'batched_ms', 'per_person_ms', 'speedup')]
    for n in (1, 8, 32, 64):
        out = make_outputs(n, dev)
        for name, items in ITEMS.items():
            b = time_calls(R.Sim3DR(), out, frame, items, a.warmup, a.calls)
            p = time_calls(PerPersonSim3DR(), out, frame, items, a.warmup, a.calls)
            lines.append('%-16s %4d %12.3f %14.3f %7.2fx' % (name, n, b, p, p / b))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
