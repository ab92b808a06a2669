"""Per-vertex colours in the Sim3DR renderer: textured meshes, the specular exponent, part and track-id colouring.  CPU
part: a numpy restatement of "light, then texture times light" against tests/golden/render_texture.npz, which the
reference's own Sim3DR.render(texture=...) rendered (scripts/make_golden_render_texture.py); the colour tables and the
--mesh_color flag.  The GPU part is tests/test_gpu_render_texture.py, which shares the helpers below."""
import os

import numpy as np
import pytest

from oracle import sim3dr_oracle as SO

F = np.float32
CASES = ('quad', 'three', 'three_first', 'smpl')
EXPONENTS = (1, 2, 5)
_cache = {}


def golden(golden_dir):
    if 'g' not in _cache:
        with np.load(os.path.join(golden_dir, 'render_texture.npz')) as g:
            _cache['g'] = {k: g[k] for k in g.files}
        for v in _cache['g'].values():
            v.setflags(write=False)
    return _cache['g']


def light_cfg(g, e, **over):
    cfg = dict(light_pos=tuple(g['light_light_pos']), view_pos=tuple(g['light_view_pos']),
               intensity_specular=float(g['light_intensity_specular']), specular_exp=int(e))
    cfg.update(over)
    return cfg


def render_textured_np(verts, tri, bg, colors, textures, cfg):
    """Sim3DR.render(color=colors[i], texture=textures[i]) for each mesh in turn (renderer.py:84-126): the clipped light,
    then ONE float32 multiply by the texture, then the rasterizer.  textures None: the light alone."""
    out = bg.copy()
    for i in range(len(verts)):
        v = np.ascontiguousarray(verts[i], F)
        light = SO.vertex_light(v, SO.get_normal(v, tri), np.asarray(colors)[[i]], cfg).astype(F)
        SO.rasterize(out, v, tri, light if textures is None else np.asarray(textures[i], F) * light)
    return out


def covered(verts, tri, shape):
    """Pixels some mesh paints."""
    mask = np.zeros(shape[:2], bool)
    for v in verts:
        mask |= SO.rasterize(np.zeros(tuple(shape[:2]) + (1,), np.uint8), v, tri, np.ones((len(v), 1), F))[:, :, 0] == 255
    return mask


def case(g, name):
    """Copies: the cached fixture stays as it was read."""
    return [g['%s_%s' % (name, k)].copy() for k in ('verts', 'triangles', 'colors', 'textures', 'bg')]


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_shapes(golden_dir):
    g = golden(golden_dir)
    assert tuple(g['exponents']) == EXPONENTS
    assert g['quad_verts'].shape == (1, 4, 3) and g['quad_triangles'].shape == (2, 3) and g['quad_bg'].shape == (8, 8, 3)
    assert g['three_verts'].shape == (3, 4, 3) and g['three_first_verts'].shape == (1, 4, 3)
    assert np.array_equal(g['three_first_verts'][0], g['three_verts'][0])
    assert g['smpl_verts'].shape == (1, 6890, 3) and g['smpl_bg'].shape == (64, 64, 3) and 6890 % 1024 != 0
    assert int(g['smpl_triangles'].max()) == 6889                   # the last, ragged pass of a 1024-wide stride loop is drawn
    i = np.arange(6890)
    assert np.array_equal(g['smpl_textures'][0], (np.stack([(i * 7) % 256, (i * 13 + 5) % 256, (i * 29 + 11) % 256], 1) / 255.0).astype(F))
    for name in CASES:
        tex = g[name + '_textures']
        assert tex.dtype == F and tex.shape == g[name + '_verts'].shape and 0 <= tex.min() and tex.max() <= 1
    assert len({tuple(r) for r in g['quad_textures'][0].tolist()}) == 4          # a different colour at each vertex
    assert not np.array_equal(g['three_textures'][0], g['three_textures'][1])


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_reference_fixture(golden_dir, name):
    """Exponents 1 and 2: bit for bit.  Exponent 5 goes through numpy's powf, whose last bit may differ between numpy
    builds; an ulp of a [0, 1] light value moves a truncated 255 * x by at most one level."""
    g = golden(golden_dir)
    verts, tri, colors, texs, bg = case(g, name)
    for e in EXPONENTS:
        img = render_textured_np(verts, tri, bg, colors, texs, light_cfg(g, e))
        want = g['%s_image_e%d' % (name, e)]
        diff = np.abs(img.astype(int) - want.astype(int))
        print(name, 'e', e, 'differing bytes', int((diff > 0).sum()), 'max', int(diff.max()))
        assert diff.max() <= (0 if e in (1, 2) else 1)
        assert (want != bg).any()


@pytest.mark.parametrize('name', CASES)
def test_fixture_texture_and_specular_show(golden_dir, name):
    """Neither part of the fixture is vacuous: the texture changes the picture, the exponents give different pictures, and
    with exponent 5 the specular term shows in at least 10 % of the covered pixels."""
    g = golden(golden_dir)
    verts, tri, colors, texs, bg = case(g, name)
    cov = covered(verts, tri, bg.shape)
    assert cov.sum() >= 20
    plain = render_textured_np(verts, tri, bg, colors, None, light_cfg(g, 1))
    assert ((plain != g[name + '_image_e1']).any(2) & cov).sum() >= 0.5 * cov.sum()
    assert not np.array_equal(g[name + '_image_e1'], g[name + '_image_e2'])
    assert not np.array_equal(g[name + '_image_e2'], g[name + '_image_e5'])
    dull = render_textured_np(verts, tri, bg, colors, texs, light_cfg(g, 5, intensity_specular=0))
    shows = ((dull != g[name + '_image_e5']).any(2) & cov).sum() / cov.sum()
    print(name, 'covered', int(cov.sum()), 'specular shows in', shows)
    assert shows >= 0.10


def test_three_meshes_overlap(golden_dir):
    """Case 'three' has pixels where a later mesh hides an earlier one, so a texture indexed by the wrong mesh shows."""
    g = golden(golden_dir)
    verts, tri, colors, texs, bg = case(g, 'three')
    cov = [covered(verts[i:i + 1], tri, bg.shape) for i in range(3)]
    assert (cov[0] & cov[1]).any() and (cov[1] & cov[2]).any() and (cov[0] & cov[2]).any()
    swapped = render_textured_np(verts, tri, bg, colors, texs[[1, 2, 0]], light_cfg(g, 1))
    assert not np.array_equal(swapped, g['three_image_e1'])


# ------------------------------------------------------------------------------------------------ colour tables
def test_mesh_color_trackID_matches_reference(golden_dir):
    from romp_amd.vis import mesh_color_trackID, tracking_color_list
    g = golden(golden_dir)
    assert list(g['track_ids']) == [0, 1, 15, 16, 17, 3, 3]
    for ids, want in ((g['track_ids'], g['track_colors']), (g['track_ids_wrap'], g['track_colors_wrap'])):
        got = mesh_color_trackID(ids)
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert list(g['track_ids_wrap']) == [78, 79, 80, 160]                        # the table holds 79 rows: these wrap
    n = len(tracking_color_list)
    assert np.array_equal(mesh_color_trackID([n, n + 1]), tracking_color_list[:2])
    assert np.array_equal(mesh_color_trackID(np.array([3, 3], np.int32))[0], tracking_color_list[3])
    table = np.arange(12.).reshape(4, 3)
    assert np.array_equal(mesh_color_trackID([5, 0], table), table[[1, 0]])


def test_part_palette():
    from romp_amd.vis import part_palette
    assert part_palette.shape == (24, 3) and part_palette.dtype == F
    assert part_palette.min() >= 0 and part_palette.max() <= 1
    assert len({tuple(r) for r in part_palette.tolist()}) == 24


# ------------------------------------------------------------------------------------------------ flags
@pytest.mark.parametrize('settings', ['romp', 'bev'])
def test_mesh_color_flag(settings):
    if settings == 'romp':
        from romp_amd.main import romp_settings as parse
    else:
        from romp_amd.bev import bev_settings as parse
    assert parse([]).mesh_color == 'identity'
    for mode in ('identity', 'same', 'track_id', 'part'):
        assert parse(['--mesh_color', mode]).mesh_color == mode
    with pytest.raises(SystemExit):
        parse(['--mesh_color', 'rainbow'])


def test_specular_exp_validation():
    """An integer >= 1 is taken; anything else keeps raising, before a device is looked for."""
    from romp_amd.renderer import Sim3DR
    for e in (1, 2, 5, np.int64(3)):
        assert Sim3DR(specular_exp=e).specular_exp == int(e)
    for e in (0, -1, 1.5, 2.0, True, None):
        with pytest.raises(NotImplementedError, match='integer >= 1'):
            Sim3DR(specular_exp=e)


def test_new_symbols_exported():
    from romp_amd import lib
    assert lib.TEXTURE_EXPORTS == ['romp_sim3dr_light_tex', 'romp_sim3dr_render_batch_tex']
    assert not set(lib.TEXTURE_EXPORTS) & (set(lib.EXPORTS) | set(lib.VIEW_EXPORTS) | set(lib.MAP_EXPORTS))
    h = lib.load()
    assert all(hasattr(h, n) for n in lib.TEXTURE_EXPORTS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'romp_hip_views.h')).read()
    assert all(n + '(' in header for n in lib.TEXTURE_EXPORTS)
