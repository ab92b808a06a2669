"""Golden fixture for per-vertex colours and the specular exponent (tests/golden/render_texture.npz), produced by the
reference's own Sim3DR.render(texture=...) (simple_romp/vis_human/sim3drender/renderer.py driving its C++ rasterizer
compiled into oracle/_ref, through oracle/make_golden_sim3dr.load_reference_renderer) and its own
vis_utils.mesh_color_trackID.  The reference's __call__ takes no textures, so the meshes of a case are painted by its
render() one after the other onto the running image, each with its own colour and texture -- what __call__ does with
render(texture=None).

Per case NAME in CASES: NAME_verts (n,V,3), NAME_triangles, NAME_colors (n,3), NAME_textures (n,V,3) float32, NAME_bg and
NAME_image_eE, the uint8 picture for specular_exp E in EXPONENTS.  light: the Sim3DR settings of every picture.

Build container only (needs the reference checkout):

    make -C oracle && python scripts/make_golden_render_texture.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sim3dr_oracle as SO  # noqa: E402
from oracle.make_golden_sim3dr import load_reference_renderer  # noqa: E402
from scripts.make_golden_render_views import load_reference_vis  # noqa: E402

F = np.float32
EXPONENTS = (1, 2, 5)
# light and eye on the same side of the meshes, so that the reflection meets the eye and the specular term is not clipped away
LIGHT = dict(light_pos=(1, -2, -4), view_pos=(0.5, -1, -5), intensity_specular=0.3)
TRACK_IDS = [0, 1, 15, 16, 17, 3, 3]
TRACK_IDS_WRAP = [78, 79, 80, 160]


def quad():
    """4 vertices, 2 triangles, not planar: the two faces and the four vertex normals differ."""
    v = np.array([[0.6, 0.7, 0.4], [6.6, 1.2, -0.5], [6.2, 6.8, 0.7], [1.1, 6.3, -0.3]], F)
    tri = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    tex = np.array([[1.0, 0.1, 0.2], [0.2, 0.9, 0.3], [0.3, 0.2, 1.0], [0.9, 0.8, 0.1]], F)
    return v, tri, tex


def case_quad():
    v, tri, tex = quad()
    bg = np.full((8, 8, 3), 40, np.uint8)
    return v[None], tri, np.array([[1.0, 0.6, 0.4]]), tex[None], bg


def case_three(n=3):
    """Three copies of the quad at different offsets and depths, each with its own texture and ambient colour."""
    v, tri, tex = quad()
    offs = np.array([[0, 0, 0], [1.3, -0.8, -3.0], [-0.9, 1.1, 2.0]], F)
    scale = np.array([1.0, 0.85, 0.9], F)
    verts = np.stack([(v * F(s) + o).astype(F) for s, o in zip(scale, offs)])
    texs = np.stack([tex, tex[::-1] * F(0.8), np.roll(tex, 1, axis=1)]).astype(F)
    colors = np.array([[1.0, 0.6, 0.4], [0.4, 0.6, 1.0], [0.7, 1.0, 0.6]])
    bg = np.full((8, 8, 3), 40, np.uint8)
    bg[::2] = 200
    return verts[:n], tri, colors[:n], texs[:n], bg


def case_smpl_sized():
    """One mesh of SMPL's size, 6890 vertices, on a 64 x 64 canvas: an ellipsoid (6808 vertices) and a band of the last
    82 in a corner, so that the vertices of the last, ragged pass of a 1024-wide stride loop show.  The texture is a
    function of the vertex index."""
    body, tri = SO.ellipsoid_mesh(84, 82, [30, 33, 0], [21, 27, 15])
    k = np.arange(41)
    band = np.stack([np.stack([44 + 0.45 * k, np.full(41, 2.3), 3 * np.sin(k / 6.0)], 1),
                     np.stack([44.2 + 0.45 * k, np.full(41, 9.6), 3 * np.cos(k / 6.0)], 1)], 1).reshape(82, 3)
    base = len(body)
    btri = [[base + 2 * i, base + 2 * i + 1, base + 2 * i + 2] for i in range(40)] + \
           [[base + 2 * i + 1, base + 2 * i + 3, base + 2 * i + 2] for i in range(40)]
    v = np.concatenate([body, band.astype(F)])
    tri = np.concatenate([tri, np.array(btri, np.int32)])
    assert v.shape == (6890, 3) and 6890 % 1024 != 0
    i = np.arange(6890)
    tex = (np.stack([(i * 7) % 256, (i * 13 + 5) % 256, (i * 29 + 11) % 256], 1) / 255.0).astype(F)
    rs = np.random.RandomState(4)
    bg = rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    return v[None], tri, np.array([[0.9, 0.9, 0.8]]), tex[None], bg


CASES = [('quad', case_quad), ('three', case_three), ('three_first', lambda: case_three(1)), ('smpl', case_smpl_sized)]


def main():
    ref = load_reference_renderer()
    _, ref_vu = load_reference_vis()
    data = {'light_' + k: np.array(v, F) for k, v in LIGHT.items()}
    data['exponents'] = np.array(EXPONENTS, np.int32)
    for name, make in CASES:
        verts, tri, colors, texs, bg = make()
        for k, v in dict(verts=verts, triangles=tri, colors=colors, textures=texs, bg=bg).items():
            data['%s_%s' % (name, k)] = v
        for e in EXPONENTS:
            r = ref.Sim3DR(specular_exp=e, **LIGHT)
            img = bg.copy()
            for i in range(len(verts)):
                img = r.render(np.ascontiguousarray(verts[i]), tri, img, colors[[i]], texture=texs[i].copy())
            data['%s_image_e%d' % (name, e)] = img
            # the specular term must show, or the exponent is not tested: the picture without it differs in enough pixels
            dull = bg.copy()
            r0 = ref.Sim3DR(specular_exp=e, **dict(LIGHT, intensity_specular=0))
            for i in range(len(verts)):
                dull = r0.render(np.ascontiguousarray(verts[i]), tri, dull, colors[[i]], texture=texs[i].copy())
            covered = (img != bg).any(2) | (dull != bg).any(2)
            share = (img != dull).any(2).sum() / max(int(covered.sum()), 1)
            print('%-12s e=%d covered px %5d, specular shows in %.1f %%' % (name, e, int(covered.sum()), 100 * share))
            assert share >= 0.10, (name, e, share)
    for key, ids in (('track_ids', TRACK_IDS), ('track_ids_wrap', TRACK_IDS_WRAP)):
        data[key] = np.array(ids, np.int64)
        data[key.replace('ids', 'colors')] = ref_vu.mesh_color_trackID(ids)
    out = os.path.join(ROOT, 'tests', 'golden', 'render_texture.npz')
    np.savez_compressed(out, **data)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
