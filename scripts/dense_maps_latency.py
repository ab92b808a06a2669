"""Latency of the dense maps (vis.dense_maps) next to the 'mesh' panel (rendering_romp_bev_results, items mesh) on one
720x1280 frame with N SMPL-sized meshes (6890 vertices, 13776 faces):

    maps alone | mesh panel alone | both, the panel's keys handed to the maps | both, each with its own raster pass

Median of --calls calls after --warmup, wall clock, each call ending with a device synchronisation (the panel is
downloaded by the renderer as always; the maps stay on the device).  The raster passes and launches of each arrangement
are counted from the C entries the call makes and their keys_ready argument (romp_sim3dr_render_batch: normals, light,
raster, resolve + 1 memset; romp_sim3dr_maps: the maps kernel + 2 memsets, and raster + 1 memset unless keys_ready); the
script fails unless sharing the keys saves exactly one raster launch.

    python scripts/dense_maps_latency.py [--out profiles/dense_maps_latency.txt]
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
from romp_amd import lib as L  # noqa: E402
from romp_amd import renderer as R  # noqa: E402
from romp_amd.vis import dense_maps, mesh_panel_keys, rendering_romp_bev_results  # noqa: E402
from render_views_latency import H, W, make_outputs  # noqa: E402

CFGS = {'mesh_color': 'identity', 'items': ['mesh'], 'renderer': 'sim3dr'}


class Counter(object):
    """Counts kernel launches, memsets and raster passes of the render / maps entries called through the library handle."""

    def __init__(self, lib):
        self.kernels = self.memsets = self.raster = 0
        self._lib, self._batch, self._maps = lib, lib.romp_sim3dr_render_batch, lib.romp_sim3dr_maps

    def __enter__(self):
        def batch(*args):
            self.kernels, self.memsets, self.raster = self.kernels + 4, self.memsets + 1, self.raster + 1
            return self._batch(*args)

        def maps(*args):
            ready = int(args[-2])
            vis, pix = args[-5], args[-4]
            self.kernels += 1 if ready else 2
            self.raster += 0 if ready else 1
            self.memsets += (0 if ready else 1) + int(bool(vis.value)) + int(bool(pix.value))
            return self._maps(*args)

        self._lib.romp_sim3dr_render_batch, self._lib.romp_sim3dr_maps = batch, maps
        return self

    def __exit__(self, *exc):
        self._lib.romp_sim3dr_render_batch, self._lib.romp_sim3dr_maps = self._batch, self._maps


def arrangements(renderer, frame, labels, dev):
    def maps_alone(out):
        dense_maps(renderer, out, frame.shape, labels)

    def panel_alone(out):
        rendering_romp_bev_results(renderer, out, frame, CFGS)

    def both_shared(out):
        keys = mesh_panel_keys(frame.shape, dev)
        rendering_romp_bev_results(renderer, out, frame, CFGS, keys=keys)
        dense_maps(renderer, out, frame.shape, labels, keys=keys)

    def both_separate(out):
        rendering_romp_bev_results(renderer, out, frame, CFGS)
        dense_maps(renderer, out, frame.shape, labels)

    return [('maps', maps_alone), ('panel', panel_alone), ('both_shared_keys', both_shared), ('both_own_keys', both_separate)]


def time_calls(fn, outputs, warmup, calls):
    for _ in range(warmup):
        fn(dict(outputs))
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn(dict(outputs))
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    lib = L.load()
    frame = np.random.RandomState(1).randint(0, 256, (H, W, 3)).astype(np.uint8)
    labels = torch.from_numpy(np.random.RandomState(2).randint(0, 24, 6890).astype(np.uint8)).to(dev)
    renderer = R.Sim3DR()
    lines = ['# one %dx%d frame, median of %d calls after %d warm-up, ms (%s)' % (H, W, a.calls, a.warmup, torch.cuda.get_device_name(0)),
             '# raster / kernels / memsets: per call, counted from the C entries called and their keys_ready argument',
             '%-18s %4s %10s %7s %8s %8s' % ('arrangement', 'N', 'median_ms', 'raster', 'kernels', 'memsets')]
    for n in (1, 64):
        outputs = make_outputs(n, dev)
        counts = {}
        for name, fn in arrangements(renderer, frame, labels, dev):
            with Counter(lib) as c:
                fn(dict(outputs))
            counts[name] = c
            ms = time_calls(fn, outputs, a.warmup, a.calls)
            lines.append('%-18s %4d %10.3f %7d %8d %8d' % (name, n, ms, c.raster, c.kernels, c.memsets))
            print(lines[-1], flush=True)
        shared, own = counts['both_shared_keys'], counts['both_own_keys']
        assert shared.raster == 1 and own.raster == 2 and own.kernels - shared.kernels == 1, 'shared keys must save one raster launch'
        assert shared.kernels == counts['panel'].kernels + 1 and counts['maps'].kernels == 2
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
