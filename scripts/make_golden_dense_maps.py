"""Golden fixture for the dense maps (tests/golden/dense_maps.npz), produced by the reference's own C++ `_rasterize`
(simple_romp/vis_human/sim3drender/lib/rasterize_kernel.cpp, compiled in place into oracle/_ref by oracle/Makefile)
driven the way the reference's Sim3DR.__call__ drives it (renderer.py:128-135): the meshes of
oracle.sim3dr_oracle.make_scene(seed=0, h=160, w=208, n=3) one after the other onto one image, each with a fresh
depth buffer at -1e8.  Stored: the inputs, every mesh's depth buffer after its own pass, the final image.  The
per-vertex colours are the reference's `_get_normal` normals lit by oracle.sim3dr_oracle.vertex_light.

Build container only (needs the reference checkout):

    make -C oracle && python scripts/make_golden_dense_maps.py
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sim3dr_oracle as SO  # noqa: E402

F = np.float32


def main():
    lib = SO.load_ref()
    assert lib is not None, 'oracle/_ref/libsim3dr_ref.so is missing: make -C oracle'
    h, w, n = 160, 208, 3
    verts, tri, bg, colors = SO.make_scene(seed=0, h=h, w=w, n=n)
    tri = np.ascontiguousarray(tri, np.int32)
    image = bg.copy()
    depths, lights = [], []
    for i in range(n):
        v = np.ascontiguousarray(verts[i], F)
        light = np.ascontiguousarray(SO.vertex_light(v, SO.ref_get_normal(v, tri), colors[[i]]), F)
        depth = np.zeros((h, w), F) - F(1e8)
        lib.ref_rasterize(SO._p(image, C.c_ubyte), SO._p(v, C.c_float), SO._p(tri, C.c_int), SO._p(light, C.c_float),
                          SO._p(depth, C.c_float), tri.shape[0], h, w, 3, 1.0, 0)
        depths.append(depth)
        lights.append(light)
        print('mesh', i, 'covers', int((depth > F(-1e8)).sum()), 'px')
    out = os.path.join(ROOT, 'tests', 'golden', 'dense_maps.npz')
    np.savez_compressed(out, verts=verts.astype(F), triangles=tri, bg=bg, colors=colors, light=np.stack(lights),
                        depth_buffers=np.stack(depths), image=image)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
