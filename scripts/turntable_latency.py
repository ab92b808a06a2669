"""Latency of the 96-view mesh turntable (--show_items rotate_mesh) of N SMPL-sized meshes (6890 vertices, 13776 faces) on
512x512 canvases: `vis.rendering_mesh_rotating_view` (one romp_view_turntable + romp_sim3dr_render_canvases per chunk of
canvases, one download) against what the single-canvas API could already do: per view `view_weak_perspective` +
`Sim3DR.__call__` onto a device canvas (one download per view).  The two transforms differ (the baseline tilts first and
fits every view on its own), so this compares cost, not pixels.  Per side the lower of two alternated medians of --calls calls after
--warmup, wall clock, both sides synchronised and ending with the frames on the host.

    python scripts/turntable_latency.py [--out profiles/turntable_latency.txt]
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
from romp_amd.vis import mesh_color_left2right, rendering_mesh_rotating_view, turntable_angles  # noqa: E402

SIZE, TILT = 512, -20.


def make_scene(n, dev, seed=0):
    rs = np.random.RandomState(seed)
    base, tri = SO.ellipsoid_mesh(84, 82, [0, 0, 0], [1, 1, 1])
    faces = np.concatenate([tri, tri[:13776 - len(tri)]]).astype(np.int32)   # SMPL's face count; no vertex of huge valence
    verts = np.zeros((n, 6890, 3), np.float32)
    verts[:, :len(base)] = base[None] * np.stack([rs.uniform(0.2, 0.35, n), rs.uniform(0.7, 0.9, n), rs.uniform(0.15, 0.3, n)], 1)[:, None]
    trans = np.stack([rs.uniform(-2, 2, n), rs.uniform(-0.5, 0.5, n), rs.uniform(4, 12, n)], 1).astype(np.float32)
    vt = verts + trans[:, None]
    vt[:, :, 2] *= -1
    return torch.from_numpy(vt).to(dev), faces, mesh_color_left2right(torch.from_numpy(trans))


def turntable(renderer, verts, faces, colors, azimuths):
    return rendering_mesh_rotating_view(renderer, verts, faces, (SIZE, SIZE), colors, azimuths=azimuths, tilt=TILT)


def per_view(renderer, verts, faces, colors, azimuths):
    white = torch.full((SIZE, SIZE, 3), 255, dtype=torch.uint8, device=verts.device)
    return np.stack([renderer(R.view_weak_perspective(verts, TILT, az, (SIZE, SIZE))[0], faces, white, mesh_colors=colors)
                     for az in azimuths])


def time_calls(fn, args, warmup, calls):
    for _ in range(warmup):
        fn(*args)
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(*args)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--calls', type=int, default=7)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    az = turntable_angles()
    K = len(az)
    renderer = R.Sim3DR()
    chunks = -(-K // renderer.max_canvases)
    # launches incl. the memsets: the transform is 1 + 3, a render 5 (normals, light, key clear, raster, resolve)
    lines = ['# %d-view turntable on %dx%d canvases, per side the lower of two alternated medians of %d calls after %d warm-up, ms (%s)'
             % (K, SIZE, SIZE, a.calls, a.warmup, torch.cuda.get_device_name(0)),
             '# turntable: 1 transform + %d chunks of <= %d canvases = %d launches, 1 download; per-view: %d x (transform + render) = %d '
             'launches, %d downloads' % (chunks, renderer.max_canvases, 4 + 5 * chunks, K, 9 * K, K),
             '%4s %14s %12s %8s' % ('N', 'turntable_ms', 'per_view_ms', 'speedup')]
    print('\n'.join(lines), flush=True)
    for n in (1, 8, 64):
        verts, faces, colors = make_scene(n, dev)
        assert turntable(renderer, verts, faces, colors, az).shape == per_view(renderer, verts, faces, colors, az).shape == (K, SIZE, SIZE, 3)
        rounds = [(time_calls(turntable, (renderer, verts, faces, colors, az), a.warmup, a.calls),
                   time_calls(per_view, (renderer, verts, faces, colors, az), a.warmup, a.calls)) for _ in range(2)]   # alternated
        t, p = min(r[0] for r in rounds), min(r[1] for r in rounds)
        lines.append('%4d %14.3f %12.3f %7.2fx' % (n, t, p, p / t))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
