"""GPU tests of the rasterizer's depth test at the values where the device's order-free rule (a 64-bit atomicMax key that holds the
depth's bits, `raster_key` in romp_amd/csrc/render.hip) and the reference's sequential IEEE `>` could part ways: -0.0 against +0.0,
a depth that underflows to -0.0, the -1e8 floor of the z-buffer, infinities and NaN.  The scenes are the crafted ones of
tests/test_dense_maps.py ('zero_signs', 'zero_underflow', 'depth_floor', 'zero_meshes'), which says what each is built for, checks
them against the compiled reference rasterizer on the CPU and, in test_abi_crafted_scenes, runs them through romp_sim3dr_maps.  Here
every picture entry paints them: renderer.rasterize (both row orders), Sim3DR.__call__ plain and with per-vertex colours, and
Sim3DR.render_canvases.  Bar: uint8 images BIT FOR BIT against the sequential restatement (the reference's compiled C++ when
oracle/_ref is built), over a random background so that an unpainted pixel cannot pass for a black one.  The lit entries take the
scenes whose depths are zeros and denormals: the lighting of a NaN or infinite vertex is no part of this."""
import numpy as np
import pytest
import torch

from oracle import sim3dr_oracle as SO
from test_dense_maps import _image_from_maps, crafted, maps_np
from test_render_texture import render_textured_np

pytestmark = pytest.mark.gpu

F = np.float32
H = W = 16
SCENES = ['zero_signs', 'zero_underflow', 'depth_floor', 'zero_meshes']
LIT = ['zero_signs', 'zero_underflow', 'zero_meshes']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def _paint(seed, verts):
    """A random background, one colour per vertex in (0.1, 0.9), one ambient colour per mesh."""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (H, W, 3)).astype(np.uint8), rs.uniform(0.1, 0.9, verts.shape).astype(F), rs.uniform(0.2, 1.0, (len(verts), 3))


def _same_image(got, want, what):
    nd = int((got != want).sum())
    print('%s: differing bytes %d of %d' % (what, nd, want.size))
    assert got.shape == want.shape and got.dtype == np.uint8 and nd == 0, what


@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('name', SCENES)
def test_rasterize_entry(dev, name, reverse):
    """renderer.rasterize with given colours, mesh after mesh onto the same picture.  With the rows in order the picture is also the
    one the scene's maps (the winners its self-check asserts) paint."""
    from romp_amd.renderer import rasterize
    sc = crafted(name)
    verts, tri = sc['verts'], sc['tri']
    bg, cols, _ = _paint(1, verts)
    ref = SO.ref_rasterize if SO.load_ref() is not None else SO.rasterize
    got, want = bg.copy(), bg.copy()
    for m in range(len(verts)):
        got = rasterize(verts[m], tri, cols[m], bg=got, reverse=reverse)
        want = ref(want, verts[m], tri, cols[m], reverse=reverse)
    assert (want != bg).any() and (want == bg).all(2).any()
    _same_image(got, want, '%s reverse=%s' % (name, reverse))
    if not reverse:
        assert np.array_equal(want, _image_from_maps(sc['ref'], verts, tri, bg, cols))


@pytest.mark.parametrize('n', [3, 2])
def test_call_on_meshes_of_signed_zeros(dev, n):
    """Sim3DR.__call__ on the first n meshes of 'zero_meshes' (+0.0, -0.0, +0.0 over the same pixels; 2 and 1 mesh bits in the key): the
    last mesh owns the pixels whatever the signs, in the picture and in the keys it leaves."""
    from romp_amd.renderer import Sim3DR
    sc = crafted('zero_meshes')
    verts, tri = sc['verts'][:n], sc['tri']
    bg, _, colors = _paint(2, verts)
    before = bg.copy()
    keys = torch.full((H * W,), -1, dtype=torch.int64, device=dev)
    got = Sim3DR()(verts, tri, bg, mesh_colors=colors, keys=keys)
    assert np.array_equal(bg, before)
    _same_image(got, SO.render_meshes(verts, tri, bg, colors, use_ref=SO.load_ref() is not None), 'zero_meshes n=%d' % n)
    owner = Sim3DR().maps(verts, tri, (H, W), keys=keys)['person_map'].cpu().numpy()
    assert np.array_equal(owner, maps_np(verts, tri, H, W)['mesh_map']) and (owner == n - 1).sum() == 36 and set(np.unique(owner)) == {-1, n - 1}
    assert ((got != bg).any(2) <= (owner >= 0)).all() and (got != bg).any()                    # painted where the owner is, nowhere else


@pytest.mark.parametrize('textured', [False, True])
@pytest.mark.parametrize('name', LIT)
def test_lit_batch_entry(dev, name, textured):
    """Sim3DR.__call__ (romp_sim3dr_render_batch, and with per-vertex colours romp_sim3dr_render_batch_tex): lit, then painted."""
    from romp_amd.renderer import Sim3DR
    sc = crafted(name)
    verts, tri = sc['verts'], sc['tri']
    bg, texs, colors = _paint(3, verts)
    keys = torch.full((H * W,), -1, dtype=torch.int64, device=dev)
    got = Sim3DR()(verts, tri, bg, mesh_colors=colors, vert_colors=texs if textured else None, keys=keys)
    want = render_textured_np(verts, tri, bg, colors, texs if textured else None, None)
    assert (want != bg).any()
    _same_image(got, want, '%s textured=%s' % (name, textured))
    tri_map = Sim3DR().maps(verts, tri, (H, W), keys=keys)['tri_map'].cpu().numpy()        # the keys it left name the reference's winners
    assert np.array_equal(tri_map, sc['ref']['tri_map'])


@pytest.mark.parametrize('textured', [False, True])
@pytest.mark.parametrize('name', LIT)
def test_canvases_entry(dev, name, textured):
    """Sim3DR.render_canvases: two canvases over slices of one slot array.  The scene's meshes are laid out twice; canvas 0 takes the
    first copy whole, canvas 1 the second copy without its last mesh, or with a repeat of it where the scene has one mesh -- so the two
    canvases differ in their number of mesh bits (zero_meshes: 2 and 1; the others: 0 and 1)."""
    from romp_amd.renderer import Sim3DR
    sc = crafted(name)
    tri = sc['tri']
    n = len(sc['verts'])
    verts = np.concatenate([sc['verts'], sc['verts'], sc['verts'][:1]])[:2 * n + (1 if n == 1 else -1)]
    offsets = np.array([0, n, len(verts)])
    assert len(verts) - n == max(n - 1, 2)
    rs = np.random.RandomState(4)
    bgs = rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    texs, colors = rs.uniform(0.1, 0.9, verts.shape).astype(F), rs.uniform(0.2, 1.0, (len(verts), 3))
    keys = torch.full((2, H, W), -1, dtype=torch.int64, device=dev)
    got = Sim3DR().render_canvases(verts, tri, bgs, offsets, mesh_colors=colors, vert_colors=texs if textured else None, keys=keys)
    for c in range(2):
        sl = slice(offsets[c], offsets[c + 1])
        want = render_textured_np(verts[sl], tri, bgs[c], colors[sl], texs[sl] if textured else None, None)
        assert (want != bgs[c]).any()
        _same_image(got[c], want, '%s textured=%s canvas %d' % (name, textured, c))
        ref = maps_np(verts[sl], tri, H, W)
        got_maps = Sim3DR().maps(verts[sl], tri, (H, W), keys=keys[c].reshape(-1))
        assert np.array_equal(got_maps['tri_map'].cpu().numpy(), ref['tri_map']) and np.array_equal(got_maps['person_map'].cpu().numpy(), ref['mesh_map'])
