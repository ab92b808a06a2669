"""Dense per-pixel maps of the Sim3DR rasterizer (romp_sim3dr_maps, Sim3DR.maps, vis.dense_maps, --dense_maps).
Fixture: tests/golden/dense_maps.npz, written by the reference's own compiled `_rasterize` (scripts/make_golden_dense_maps.py).
CPU part: `maps_np`, a numpy restatement of the semantics (the reference's sequential z-buffer, kept per pixel instead of
painted), against the fixture's depth buffers and image and against the compiled reference rasterizer.  GPU part: the C
ABI and the Python layers against the restatement.  Bar: integer maps EXACT, float maps BIT FOR BIT."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import sim3dr_oracle as SO

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = ('person_map', 'tri_map', 'bary_map', 'attr_map', 'label_map', 'vert_visible', 'person_pixels')


# ------------------------------------------------------------------------------------------------ restatement
def raster_np(verts, tri, h, w):
    """rasterize_kernel.cpp:233-300 for one mesh, keeping per pixel what the reference overwrites: triangles in index
    order, strict `>` against a -1e8 buffer -> (depth buffer, winning triangle or -1, its weights)."""
    v = np.asarray(verts, F)
    depth = np.zeros((h, w), F) - F(1e8)
    win = np.full((h, w), -1, np.int32)
    bary = np.zeros((h, w, 3), F)
    with np.errstate(all='ignore'):
        for t, (i0, i1, i2) in enumerate(np.asarray(tri, np.int64)):
            p0, p1, p2 = v[i0], v[i1], v[i2]
            x_min = max(int(np.ceil(min(p0[0], p1[0], p2[0]))), 0)
            x_max = min(int(np.floor(max(p0[0], p1[0], p2[0]))), w - 1)
            y_min = max(int(np.ceil(min(p0[1], p1[1], p2[1]))), 0)
            y_max = min(int(np.floor(max(p0[1], p1[1], p2[1]))), h - 1)
            if x_max < x_min or y_max < y_min:
                continue
            ys, xs = np.mgrid[y_min:y_max + 1, x_min:x_max + 1]
            w0, w1, w2 = SO._weights(xs.astype(F), ys.astype(F), p0, p1, p2)
            w0, w1, w2 = (np.broadcast_to(np.asarray(a, F), xs.shape) for a in (w0, w1, w2))
            pd = (w0 * p0[2] + w1 * p1[2]) + w2 * p2[2]
            hit = (w2 >= 0) & (w1 >= 0) & (w0 > 0) & (pd > depth[ys, xs])
            yy, xx = ys[hit], xs[hit]
            depth[yy, xx] = pd[hit]
            win[yy, xx] = t
            bary[yy, xx] = np.stack([w0[hit], w1[hit], w2[hit]], -1)
    return depth, win, bary


def maps_np(verts, tri, h, w, mesh_ids=None, attrs=None, attr_bg=0., vert_labels=None):
    """The table of include/romp_hip_maps.h in numpy: meshes painted in index order, each with a fresh z-buffer, so the
    highest mesh that covers a pixel owns it.  Also returns 'mesh_map' (the mesh index) and 'depth_buffers' (n,h,w)."""
    verts = np.asarray(verts, F)
    tri = np.asarray(tri, np.int32)
    n, nver = verts.shape[:2]
    mesh = np.full((h, w), -1, np.int32)
    tri_map = np.full((h, w), -1, np.int32)
    bary = np.zeros((h, w, 3), F)
    depths = np.zeros((n, h, w), F)
    for m in range(n):
        depths[m], win, b = raster_np(verts[m], tri, h, w)
        cover = win >= 0
        mesh[cover], tri_map[cover], bary[cover] = m, win[cover], b[cover]
    fg = mesh >= 0
    out = {'mesh_map': mesh, 'depth_buffers': depths, 'tri_map': tri_map, 'bary_map': bary}
    ids = np.arange(n, dtype=np.int32) if mesh_ids is None else np.asarray(mesh_ids, np.int32)
    out['person_map'] = np.where(fg, ids[np.maximum(mesh, 0)] if n else -1, -1).astype(np.int32)
    corners = tri[tri_map[fg]] if n else np.zeros((0, 3), np.int32)            # (P,3) vertex indices of the winners
    if attrs is not None:
        a = np.asarray(attrs, F).reshape(n, nver, -1)
        am = np.full((h, w, a.shape[2]), attr_bg, F)
        if n:
            a0, a1, a2 = (a[mesh[fg], corners[:, k]] for k in range(3))
            b = bary[fg]
            am[fg] = (b[:, :1] * a0 + b[:, 1:2] * a1) + b[:, 2:] * a2
        out['attr_map'] = am
    if vert_labels is not None:
        lm = np.full((h, w), 255, np.uint8)
        if n:
            lm[fg] = np.asarray(vert_labels, np.uint8)[corners[np.arange(len(corners)), np.argmax(bary[fg], 1)]]   # first maximum
        out['label_map'] = lm
    vis = np.zeros((n, nver), np.uint8)
    if n:
        vis[np.repeat(mesh[fg], 3), corners.reshape(-1)] = 1
    out['vert_visible'] = vis
    out['person_pixels'] = np.bincount(mesh[fg], minlength=n).astype(np.int32)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ scenes
def _golden(golden_dir=os.path.join(ROOT, 'tests', 'golden')):
    return np.load(os.path.join(golden_dir, 'dense_maps.npz'))


def _extras(verts, seed, c):
    """mesh ids, a c-channel attribute (channel 0: the rasterized z) and vertex labels for a scene."""
    rs = np.random.RandomState(seed)
    n, nver = verts.shape[:2]
    attrs = np.concatenate([verts[:, :, 2:], rs.normal(0, 3, (n, nver, c - 1)).astype(F)], 2).astype(F)
    return dict(mesh_ids=rs.permutation(n).astype(np.int32) + 10, attrs=np.ascontiguousarray(attrs), attr_bg=-7.5,
                vert_labels=rs.randint(0, 24, nver).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def fixture_scene(n, c):
    """The fixture's meshes: the first n of its 3; n = 5: mesh 3 repeats mesh 0 verbatim (a tie between meshes: the later
    one wins), mesh 4 is mesh 1 moved."""
    g = _golden()
    verts = g['verts']
    if n > 3:
        verts = np.concatenate([verts, verts[:1], verts[1:2] + np.array([17.25, -9.5, 3.0], F)]).astype(F)
    verts = np.ascontiguousarray(verts[:n])
    h, w = g['bg'].shape[:2]
    sc = dict(verts=verts, tri=g['triangles'], h=h, w=w, **_extras(verts, n, c))
    sc['ref'] = maps_np(verts, sc['tri'], h, w, sc['mesh_ids'], sc['attrs'], sc['attr_bg'], sc['vert_labels'])
    return sc


def _scene(verts, tri, h=16, w=16, c=2, seed=0):
    verts = np.ascontiguousarray(np.asarray(verts, F).reshape((-1,) + np.shape(verts)[-2:]))
    tri = np.ascontiguousarray(tri, np.int32)
    sc = dict(verts=verts, tri=tri, h=h, w=w, **_extras(verts, seed, c))
    sc['ref'] = maps_np(verts, tri, h, w, sc['mesh_ids'], sc['attrs'], sc['attr_bg'], sc['vert_labels'])
    return sc


@functools.lru_cache(maxsize=None)
def crafted(name):
    if name == 'coplanar_tie':          # two overlapping triangles in the plane z = 0: equal depth, the lowest index wins
        return _scene([[2, 2, 0], [13, 3, 0], [4, 12, 0], [1, 6, 0], [12, 1, 0], [11, 13, 0]], [[0, 1, 2], [3, 4, 5]])
    if name == 'edge_vertex':           # integer vertices, legs of 8 (every weight exact); the two share the edge (10,2)-(2,10)
        return _scene([[2, 2, 1], [10, 2, 2], [2, 10, 3], [10, 10, 4]], [[0, 1, 2], [1, 3, 2]])
    if name == 'zero_area':             # collinear corners: the denominator is 0, weights (1,0,0) all over the bounding box
        return _scene([[3, 3, 2], [7, 7, 9], [5, 5, -4], [9, 1, 0], [14, 2, 0], [12, 6, 0]], [[0, 1, 2], [3, 4, 5]])
    if name == 'off_canvas':            # one triangle partly on the canvas, two wholly off it, one across a corner
        return _scene([[-5, -5, 1], [8, 3, 2], [3, 9, 3], [20, 20, 1], [30, 20, 1], [20, 30, 1], [-10, -3, 1], [-2, -8, 1], [-4, -1, 1],
                       [12.5, 12.5, 0], [22, 13, 1], [13, 25, 2]], [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]])
    if name == 'paint_order':           # mesh 0 nearer (greater depth) but painted first and fully covered by mesh 1
        return _scene([[[5, 5, 10], [9, 5, 10], [5, 9, 10]], [[1, 1, -10], [15, 1, -10], [1, 15, -10]]], [[0, 1, 2]])
    if name == 'canvas_37x53':          # h * w = 1961: no multiple of the block of 256, eight blocks
        verts, tri, _, _ = SO.make_scene(seed=1, h=37, w=53, n=3, n_lat=6, n_lon=8)
        return _scene(verts, tri, 37, 53, c=3, seed=5)
    # Depth edges: where an IEEE `>` and an integer key of the depth's bits could part ways.  Right triangles with integer corners
    # and legs of 8 or 4 (a power of two: every weight is an exact multiple of 1/8 or 1/4).
    nz, pz = -0.0, 0.0
    if name == 'zero_signs':            # -0.0 == +0.0 for the z-test: the first one drawn stays, whichever sign it has
        return _scene([[1, 1, nz], [9, 1, nz], [1, 9, nz], [3, 1, pz], [11, 1, pz], [3, 9, pz],
                       [14, 14, pz], [6, 14, pz], [14, 6, pz], [12, 14, nz], [4, 14, nz], [12, 6, nz]],
                      [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]])
    if name == 'zero_underflow':        # z = the smallest denormal: w * z rounds to -0.0 for w <= 1/2, stays the denormal above
        d = float(np.float32(-1.4e-45))
        return _scene([[2, 2, d], [10, 2, d], [2, 10, d], [2, 2, pz], [10, 2, pz], [2, 10, pz]], [[0, 1, 2], [3, 4, 5]])
    if name == 'depth_floor':           # the -1e8 floor of the z-buffer, infinities and NaN; six disjoint footprints
        lo, inf, nan = float(F(-1e8)), float('inf'), float('nan')
        up = float(np.nextafter(F(-1e8), F(0)))
        return _scene([[0, 0, lo], [8, 0, lo], [0, 8, lo],                     # 0: exactly the floor: never above it
                       [8, 8, up], [0, 8, up], [8, 0, up],                     # 1: one ulp above the floor
                       [10, 0, -inf], [14, 0, -inf], [10, 4, -inf],            # 2
                       [14, 4, 1], [10, 4, nan], [14, 0, 1],                   # 3: NaN at p1 only; 0 * NaN is NaN at every pixel
                       [10, 6, inf], [14, 6, inf], [10, 10, inf],              # 4, 5: +inf twice over the same pixels
                       [10, 6, inf], [14, 6, inf], [10, 10, inf],
                       [1, 10, 5], [5, 10, 5], [1, 14, 5],                     # 6: finite, 7: +inf over it
                       [1, 10, inf], [5, 10, inf], [1, 14, inf]],
                      [[3 * t, 3 * t + 1, 3 * t + 2] for t in range(8)])
    if name == 'zero_meshes':           # three meshes over the same pixels at z = +0, -0, +0: a later mesh wins whatever the signs
        return _scene([[[3, 3, z], [11, 3, z], [3, 11, z]] for z in (pz, nz, pz)], [[0, 1, 2]])
    raise KeyError(name)


CRAFTED = ['coplanar_tie', 'edge_vertex', 'zero_area', 'off_canvas', 'paint_order', 'canvas_37x53',
           'zero_signs', 'zero_underflow', 'depth_floor', 'zero_meshes']


# ------------------------------------------------------------------------------------------------ CPU
def test_restatement_depth_equals_reference_depth_buffers(golden_dir):
    g = _golden(golden_dir)
    sc = fixture_scene(3, 1)
    ref, buf = sc['ref'], g['depth_buffers']
    assert same(ref['depth_buffers'], buf)
    attr = maps_np(sc['verts'], sc['tri'], sc['h'], sc['w'], attrs=sc['verts'][:, :, 2:], attr_bg=-1e8)['attr_map'][:, :, 0]
    for m in range(3):
        wins = ref['mesh_map'] == m
        assert wins.any() and same(attr[wins], buf[m][wins]), m
    assert np.array_equal(ref['mesh_map'] >= 0, (buf > F(-1e8)).any(0))
    assert np.array_equal(ref['mesh_map'], np.where((buf > F(-1e8)).any(0), 2 - np.argmax((buf > F(-1e8))[::-1], 0), -1))
    assert np.array_equal(ref['person_map'] >= 0, ref['mesh_map'] >= 0)


def _image_from_maps(ref, verts, tri, bg, lights):
    """The picture from tri_map / bary_map and per-vertex colours: (w0*c0 + w1*c1) + w2*c2, times 255, truncated."""
    img = bg.copy()
    fg = ref['mesh_map'] >= 0
    corners, m, b = tri[ref['tri_map'][fg]], ref['mesh_map'][fg], ref['bary_map'][fg]
    c0, c1, c2 = (lights[m, corners[:, k]] for k in range(3))
    pc = (b[:, :1] * c0 + b[:, 1:2] * c1) + b[:, 2:] * c2
    img[fg] = (F(255) * pc).astype(np.int64).astype(np.uint8)
    return img


def _lights(verts, tri, colors):
    return np.stack([SO.vertex_light(v, SO.get_normal(v, tri), colors[[i % len(colors)]]).astype(F) for i, v in enumerate(verts)])


def test_image_rebuilt_from_maps_equals_reference_image(golden_dir):
    g = _golden(golden_dir)
    sc = fixture_scene(3, 1)
    lights = _lights(sc['verts'], sc['tri'], g['colors'])
    assert same(lights, g['light'])
    img = _image_from_maps(sc['ref'], sc['verts'], sc['tri'], g['bg'], lights)
    assert np.array_equal(img, g['image']) and (img != g['bg']).any()


def _ref_lib_pass(lib, image, verts, tri, colors, depth):
    h, w, c = image.shape
    lib.ref_rasterize(SO._p(image, C.c_ubyte), SO._p(verts, C.c_float), SO._p(tri, C.c_int), SO._p(colors, C.c_float),
                      SO._p(depth, C.c_float), tri.shape[0], h, w, c, 1.0, 0)


@pytest.mark.parametrize('name', ['fixture'] + CRAFTED)
def test_restatement_vs_compiled_reference_rasterizer(name):
    lib = SO.load_ref()
    if lib is None:
        pytest.skip('oracle/_ref/libsim3dr_ref.so has not been built')
    sc = fixture_scene(3, 1) if name == 'fixture' else crafted(name)
    verts, tri, h, w, ref = sc['verts'], np.ascontiguousarray(sc['tri'], np.int32), sc['h'], sc['w'], sc['ref']
    rs = np.random.RandomState(3)
    bg = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    lights = rs.uniform(0.1, 0.9, verts.shape).astype(F)
    image = bg.copy()
    for m in range(len(verts)):
        depth = np.zeros((h, w), F) - F(1e8)                                  # the test's own depth array
        _ref_lib_pass(lib, image, np.ascontiguousarray(verts[m]), tri, np.ascontiguousarray(lights[m]), depth)
        assert same(depth, ref['depth_buffers'][m]), (name, m)
        wins = ref['mesh_map'] == m
        zattr = maps_np(verts, tri, h, w, attrs=verts[:, :, 2:], attr_bg=-1e8)['attr_map'][:, :, 0]
        assert same(zattr[wins], depth[wins])
    assert np.array_equal(_image_from_maps(ref, verts, tri, bg, lights), image), name


def test_crafted_scenes_say_what_they_are_built_for():
    r = crafted('coplanar_tie')['ref']
    both = (raster_np(crafted('coplanar_tie')['verts'][0], [[0, 1, 2]], 16, 16)[1] >= 0) & \
           (raster_np(crafted('coplanar_tie')['verts'][0], [[3, 4, 5]], 16, 16)[1] >= 0)
    assert both.sum() > 10 and (r['tri_map'][both] == 0).all() and (r['tri_map'] == 1).any()
    r = crafted('edge_vertex')['ref']
    assert r['tri_map'][6, 6] == 1 and same(r['bary_map'][6, 6], np.array([0.5, 0, 0.5], F))     # on the shared edge: w0 == 0 shuts 0 out
    assert r['tri_map'][2, 2] == 0 and same(r['bary_map'][2, 2], np.array([1, 0, 0], F))         # on a vertex: p0 of triangle 0
    assert r['tri_map'][2, 10] == 1 and r['tri_map'][10, 2] == -1 and r['tri_map'][10, 10] == -1  # p2 of both, p1 of 1: w0 == 0
    assert r['tri_map'][2, 6] == 0 and r['bary_map'][2, 6, 2] == 0                               # on triangle 0's edge p0-p1: w2 == 0 stays in
    r = crafted('zero_area')['ref']
    assert (r['tri_map'] == 0).sum() == 25 and (r['tri_map'][3:8, 3:8] == 0).all()
    assert same(r['bary_map'][5, 4], np.array([1, 0, 0], F)) and r['attr_map'][5, 4, 0] == 2
    assert r['vert_visible'][0, :3].all()
    r = crafted('off_canvas')['ref']
    assert set(np.unique(r['tri_map'])) == {-1, 0, 3} and not r['vert_visible'][0, 3:9].any() and r['vert_visible'][0, [0, 1, 2, 9, 10, 11]].all()
    r = crafted('paint_order')['ref']
    assert (r['depth_buffers'][0] > F(-1e8)).sum() > 0 and r['person_pixels'][0] == 0 and not r['vert_visible'][0].any()
    assert r['person_pixels'][1] == (r['mesh_map'] == 1).sum() > 50 and r['vert_visible'][1].all()
    alone = lambda sc, t: raster_np(sc['verts'][0], sc['tri'][t:t + 1], 16, 16)               # triangle t with nothing else drawn
    sc = crafted('zero_signs')
    r, z = sc['ref'], sc['verts'][0, :, 2]
    assert (z == 0).all() and np.signbit(z).tolist() == [True] * 3 + [False] * 6 + [True] * 3
    for first, second in ((0, 1), (2, 3)):                                                    # the overlaps go to 0 and to 2
        both = (alone(sc, first)[1] >= 0) & (alone(sc, second)[1] >= 0)
        assert both.sum() > 10 and (r['tri_map'][both] == first).all() and (r['tri_map'] == second).any()
    sc = crafted('zero_underflow')
    r, tiny = sc['ref'], F(-1.4e-45)
    d0, w0 = alone(sc, 0)[0], alone(sc, 0)[1] >= 0
    assert tiny < 0 and tiny == np.nextafter(F(0), F(-1)) and w0.sum() == 36 and np.array_equal(w0, alone(sc, 1)[1] >= 0)
    under, kept = w0 & (d0 == 0), w0 & (d0 == tiny)
    assert under.sum() > 0 and kept.sum() > 0 and under.sum() + kept.sum() == 36 and np.signbit(d0[under]).all()
    assert (r['tri_map'][kept] == 1).all() and (r['tri_map'][under] == 0).all()               # 0 > denormal, but not 0 > -0.0
    assert same(r['attr_map'][:, :, 0][under], np.full(int(under.sum()), -0.0, F))            # and the map keeps the sign
    r = crafted('depth_floor')['ref']
    painted = [int((r['tri_map'] == t).sum()) for t in range(8)]
    assert painted[:4] == [0, 36, 0, 0] and painted[4] > 0 and painted[5] == 0, painted
    assert painted[7] > 0 and painted[6] + painted[7] == 10, painted                          # 7's edges are 0 * inf = NaN: 6 stays there
    assert r['tri_map'][4, 14] == -1 and r['tri_map'][0, 0] == -1                             # the NaN triangle's p0, the floor's p0
    assert np.isposinf(r['attr_map'][:, :, 0][r['tri_map'] == 4]).all() and np.isfinite(r['attr_map'][:, :, 0][r['tri_map'] == 1]).all()
    sc = crafted('zero_meshes')
    r = sc['ref']
    assert np.signbit(sc['verts'][:, 0, 2]).tolist() == [False, True, False] and (sc['verts'][:, :, 2] == 0).all()
    assert r['person_pixels'].tolist() == [0, 0, 36] and (r['mesh_map'] == 2).sum() == 36
    two = maps_np(sc['verts'][:2], sc['tri'], 16, 16)
    assert two['person_pixels'].tolist() == [0, 36] and np.array_equal(two['mesh_map'] == 1, r['mesh_map'] == 2)
    for name in CRAFTED:
        r = crafted(name)['ref']
        assert r['person_pixels'].sum() == (r['mesh_map'] >= 0).sum()
        assert set(np.unique(r['label_map'][r['mesh_map'] >= 0])) <= set(range(24)) and (r['label_map'][r['mesh_map'] < 0] == 255).all()


def test_map_symbol_exported():
    from romp_amd import lib
    assert lib.MAP_EXPORTS == ['romp_sim3dr_maps']
    assert not set(lib.MAP_EXPORTS) & (set(lib.EXPORTS) | set(lib.VIEW_EXPORTS))
    assert len(lib.EXPORTS) == 52 and len(lib.VIEW_EXPORTS) == 2
    h = lib.load()
    assert hasattr(h, 'romp_sim3dr_maps') and h.romp_abi_version() == 7
    header = open(os.path.join(ROOT, 'include', 'romp_hip_maps.h')).read()
    assert 'romp_sim3dr_maps(' in header


def test_dense_maps_setting_is_off_by_default_and_implies_meshes():
    import romp_amd
    from romp_amd import bev
    assert romp_amd.romp_settings([]).dense_maps is False and bev.bev_settings([]).dense_maps is False
    for s in (romp_amd.romp_settings(['--dense_maps', '--calc_smpl']), bev.bev_settings(['--dense_maps', '--calc_smpl'])):
        assert s.dense_maps is True and s.calc_smpl is True


def test_part_labels_are_the_first_greatest_skinning_weight():
    from oracle import romp_oracle as O
    from romp_amd.smpl import SMPL
    info = dict(O.make_synthetic_smpl(0))
    wts = info['weights'].clone().float()
    wts[5] = 0
    wts[5, 3] = wts[5, 17] = 0.5                                               # a tie: the first index
    model = SMPL(dict(info, weights=wts))
    labels = model.part_labels
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (6890,) and int(labels.max()) <= 23 and labels[5] == 3
    assert np.array_equal(labels.numpy(), np.argmax(wts.numpy(), 1).astype(np.uint8))
    assert 'part_labels' not in model.state_dict()


# ------------------------------------------------------------------------------------------------ GPU: the C ABI
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


SENTINEL = {torch.int32: -77777, torch.float32: -12345.5, torch.uint8: 0xAB}
PAD_ROWS = 3


def abi_maps(dev, sc, which=MAPS, keys=None, keys_ready=0, n=None, ntri=None, expect_error=False):
    """romp_sim3dr_maps on scene `sc` into buffers PAD_ROWS rows larger than needed, filled with a sentinel -> the maps as
    numpy.  Asserts that the rows past the end still hold the sentinel."""
    from romp_amd import lib as L
    verts, tri, h, w = sc['verts'], sc['tri'], sc['h'], sc['w']
    nm, nver = verts.shape[:2]
    c = sc['attrs'].shape[2]
    shapes = {'person_map': ((h, w), torch.int32), 'tri_map': ((h, w), torch.int32), 'bary_map': ((h, w, 3), torch.float32),
              'attr_map': ((h, w, c), torch.float32), 'label_map': ((h, w), torch.uint8), 'vert_visible': ((nm, nver), torch.uint8),
              'person_pixels': ((nm,), torch.int32)}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    v_d, tri_d, ids_d, attrs_d, lab_d = t(verts), t(tri), t(sc['mesh_ids']), t(sc['attrs']), t(sc['vert_labels'])
    bufs = {}
    for m in which:
        shape, dtype = shapes[m]
        row = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        bufs[m] = torch.full((int(np.prod(shape)) + PAD_ROWS * max(row, 1),), SENTINEL[dtype], dtype=dtype, device=dev)
    if keys is None:
        keys = torch.full((h * w,), -1, dtype=torch.int64, device=dev)        # garbage: keys_ready = 0 must clear them
    rc = L.load().romp_sim3dr_maps(L.ptr(v_d), nm if n is None else n, nver, L.ptr(tri_d), tri.shape[0] if ntri is None else ntri, h, w,
                                   L.ptr(ids_d), L.ptr(attrs_d), c, float(sc['attr_bg']), L.ptr(lab_d),
                                   *[L.ptr(bufs.get(m)) for m in MAPS], L.ptr(keys), keys_ready, L.stream_ptr(dev))
    torch.cuda.current_stream(dev).synchronize()
    if expect_error:
        assert rc != 0
        for m in which:                                                       # nothing was written
            assert bool((bufs[m] == SENTINEL[bufs[m].dtype]).all()), m
        return L.load().romp_last_error()
    assert rc == 0, L.load().romp_last_error()
    out = {}
    for m in which:
        shape, dtype = shapes[m]
        size = int(np.prod(shape))
        host = bufs[m].cpu().numpy()
        assert (host[size:] == SENTINEL[dtype]).all(), 'write past the end of ' + m
        out[m] = host[:size].reshape(shape)
    return out


def check(got, ref, which=MAPS):
    for m in which:
        assert same(got[m], ref[m]), '%s: %d of %d elements differ' % (m, int((bits(got[m]) != bits(ref[m])).sum()), ref[m].size)


@pytest.mark.gpu
@pytest.mark.parametrize('n,c', [(1, 1), (2, 4), (3, 1), (3, 2), (3, 3), (3, 4), (5, 4)])
def test_abi_fixture_scene_all_outputs(dev, n, c):
    sc = fixture_scene(n, c)
    got = abi_maps(dev, sc)
    check(got, sc['ref'])
    assert (got['person_map'] >= 0).sum() > 1000 and got['person_pixels'].sum() == (got['person_map'] >= 0).sum()


@pytest.mark.gpu
def test_abi_each_output_alone(dev):
    sc = fixture_scene(3, 4)
    for m in MAPS:
        check(abi_maps(dev, sc, which=(m,)), sc['ref'], (m,))


@pytest.mark.gpu
@pytest.mark.parametrize('name', CRAFTED)
def test_abi_crafted_scenes(dev, name):
    sc = crafted(name)
    check(abi_maps(dev, sc), sc['ref'])


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 3, 5])
def test_abi_keys_ready_after_render_batch(dev, n, golden_dir):
    """The keys romp_sim3dr_render_batch leaves are the maps' own: keys_ready = 1 gives the same bits, and the maps say
    which pixels of the picture were painted."""
    from romp_amd.renderer import Sim3DR
    sc = fixture_scene(n, 4)
    g = _golden(golden_dir)
    keys = torch.full((sc['h'] * sc['w'],), -1, dtype=torch.int64, device=dev)
    img = Sim3DR()(sc['verts'], sc['tri'], g['bg'], mesh_colors=g['colors'], keys=keys)
    fresh = abi_maps(dev, sc)
    shared = abi_maps(dev, sc, keys=keys, keys_ready=1)
    check(shared, fresh)
    check(shared, sc['ref'])
    assert np.array_equal(img, _image_from_maps(sc['ref'], sc['verts'], sc['tri'], g['bg'], _lights(sc['verts'], sc['tri'], g['colors'])))


@pytest.mark.gpu
def test_abi_on_a_side_stream(dev):
    sc = fixture_scene(3, 2)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        got = abi_maps(dev, sc)
    check(got, sc['ref'])


@pytest.mark.gpu
def test_abi_rejects_what_the_key_cannot_hold(dev):
    """3 meshes take 2 key bits, 30 are left: 2^30 + 1 triangles do not fit.  Rejected before anything is launched or written."""
    sc = crafted('paint_order')
    msg = abi_maps(dev, sc, n=3, ntri=(1 << 30) + 1, expect_error=True)
    assert b'key bits' in msg and b'romp_sim3dr_maps' in msg
    from romp_amd import lib as L
    keys = torch.zeros(4, dtype=torch.int64, device=dev)
    buf = torch.zeros(64, dtype=torch.float32, device=dev)
    amap = torch.full((16,), 3.0, device=dev)
    lib = L.load()
    nul = C.c_void_p(0)
    args = lambda attrs, c, labels, attr_map, label_map: (L.ptr(buf), 1, 3, L.ptr(buf), 1, 2, 2, nul, attrs, c, 0.0, labels, nul, nul, nul,
                                                         attr_map, label_map, nul, nul, L.ptr(keys), 0, L.stream_ptr(dev))
    assert lib.romp_sim3dr_maps(*args(nul, 1, nul, L.ptr(amap), nul)) != 0 and b'attrs' in lib.romp_last_error()
    assert lib.romp_sim3dr_maps(*args(L.ptr(buf), 5, nul, L.ptr(amap), nul)) != 0 and b'attrs' in lib.romp_last_error()
    assert lib.romp_sim3dr_maps(*args(nul, 1, nul, nul, L.ptr(amap))) != 0 and b'vert_labels' in lib.romp_last_error()
    torch.cuda.synchronize()
    assert bool((amap == 3.0).all())


# ------------------------------------------------------------------------------------------------ GPU: Sim3DR.maps
def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.gpu
def test_sim3dr_maps_numpy_and_device_input(dev):
    from romp_amd.renderer import Sim3DR
    sc = fixture_scene(5, 4)
    r = Sim3DR()
    kw = dict(mesh_ids=sc['mesh_ids'], attrs=sc['attrs'], attr_bg=sc['attr_bg'], vert_labels=sc['vert_labels'])
    got = r.maps(list(sc['verts']), sc['tri'], (sc['h'], sc['w'], 3), **kw)
    assert set(got) == set(MAPS) and all(v.is_cuda for v in got.values())
    check(_np(got), sc['ref'])
    t = lambda a: torch.from_numpy(a).to(dev)
    got = r.maps(t(sc['verts']), sc['tri'], (sc['h'], sc['w']), mesh_ids=t(sc['mesh_ids']), attrs=t(sc['attrs']), attr_bg=sc['attr_bg'],
                 vert_labels=t(sc['vert_labels']), want=('tri_map', 'attr_map'))
    assert set(got) == {'tri_map', 'attr_map'}
    check(_np(got), sc['ref'], ('tri_map', 'attr_map'))
    plain = _np(r.maps(sc['verts'], sc['tri'], (sc['h'], sc['w'])))                          # no ids, attributes or labels
    assert set(plain) == set(MAPS) - {'attr_map', 'label_map'} and np.array_equal(plain['person_map'], sc['ref']['mesh_map'])
    depth = _np(r.maps(sc['verts'], sc['tri'], (sc['h'], sc['w']), attrs=sc['verts'][:, :, 2], attr_bg=-1e8, want=['attr_map']))['attr_map']
    assert depth.shape == (sc['h'], sc['w'], 1)
    for m in range(5):                                                                       # the reference's depth buffers
        wins = sc['ref']['mesh_map'] == m
        assert same(depth[:, :, 0][wins], sc['ref']['depth_buffers'][m][wins])


@pytest.mark.gpu
def test_sim3dr_maps_shared_keys(dev, golden_dir):
    from romp_amd.renderer import Sim3DR
    sc = fixture_scene(3, 1)
    g = _golden(golden_dir)
    r = Sim3DR()
    keys = torch.empty(sc['h'] * sc['w'], dtype=torch.int64, device=dev)
    img = r(sc['verts'], sc['tri'], g['bg'], mesh_colors=g['colors'], keys=keys)
    assert np.array_equal(img, g['image'])
    kw = dict(mesh_ids=sc['mesh_ids'], attrs=sc['attrs'], attr_bg=sc['attr_bg'], vert_labels=sc['vert_labels'])
    check(_np(r.maps(sc['verts'], sc['tri'], img.shape, keys=keys, **kw)), sc['ref'])
    with pytest.raises(ValueError, match='keys'):
        r.maps(sc['verts'], sc['tri'], img.shape, keys=keys[:-1])


@pytest.mark.gpu
def test_sim3dr_maps_nobody_and_bad_input(dev):
    from romp_amd.renderer import Sim3DR
    r = Sim3DR()
    empty = torch.zeros((0, 12, 3), device=dev)
    got = _np(r.maps(empty, np.zeros((4, 3), np.int32), (5, 7), attrs=torch.zeros((0, 12, 2), device=dev), attr_bg=float('inf'),
                     vert_labels=np.zeros(12, np.uint8)))
    assert (got['person_map'] == -1).all() and (got['tri_map'] == -1).all() and (got['bary_map'] == 0).all() and (got['label_map'] == 255).all()
    assert got['attr_map'].shape == (5, 7, 2) and np.isposinf(got['attr_map']).all() and got['person_map'].shape == (5, 7)
    assert got['vert_visible'].shape == (0, 12) and got['person_pixels'].shape == (0,) and got['bary_map'].shape == (5, 7, 3)
    assert got['person_map'].dtype == np.int32 and got['label_map'].dtype == np.uint8 and got['bary_map'].dtype == np.float32
    assert set(r.maps([], np.zeros((4, 3), np.int32), (5, 7))) == set(MAPS) - {'attr_map', 'label_map'}
    sc = crafted('paint_order')
    with pytest.raises(ValueError, match='one triangle table'):
        r.maps(sc['verts'], [sc['tri'], sc['tri']], (16, 16))
    with pytest.raises(ValueError, match='attr_map needs attrs'):
        r.maps(sc['verts'], sc['tri'], (16, 16), want=('attr_map',))
    with pytest.raises(ValueError, match='label_map needs vert_labels'):
        r.maps(sc['verts'], sc['tri'], (16, 16), want=('label_map',))
    with pytest.raises(ValueError, match='attrs must be'):
        r.maps(sc['verts'], sc['tri'], (16, 16), attrs=np.zeros((2, 3, 5), F))
    with pytest.raises(ValueError, match='unknown maps'):
        r.maps(sc['verts'], sc['tri'], (16, 16), want=('depth',))


# ------------------------------------------------------------------------------------------------ GPU: the public setting
NEW_KEYS = ('person_map', 'part_map', 'depth_map', 'verts_visible', 'person_pixels')


def _faces():
    _, base_tri = SO.ellipsoid_mesh(84, 82, [0, 0, 0], [1, 1, 1])
    faces = np.zeros((13776, 3), np.int64)                                   # a real closed surface over the first 6808 vertices
    faces[:len(base_tri)] = base_tri
    return faces


def _check_result(out, frame, org, labels, faces, dev, rendered):
    """The five keys of `out` against a direct Sim3DR.maps call on the geometry of the mesh panel, rebuilt here from the
    returned rows: `org` = verts_camed_org (N,6890,3) device tensor in result order."""
    from romp_amd.renderer import Sim3DR
    h, w = frame.shape[:2]
    N = len(out['cam_trans'])
    assert out['person_map'].shape == (h, w) and out['person_map'].dtype == np.int32
    assert out['part_map'].shape == (h, w) and out['part_map'].dtype == np.uint8
    assert out['depth_map'].shape == (h, w) and out['depth_map'].dtype == np.float32
    assert out['verts_visible'].shape == (N, 6890) and out['verts_visible'].dtype == np.bool_
    assert out['person_pixels'].shape == (N,) and out['person_pixels'].dtype == np.int32
    pm = out['person_map']
    assert pm.min() >= -1 and pm.max() < N and (pm >= 0).any()
    for i in range(N):
        assert (pm == i).sum() == out['person_pixels'][i], i
    order = torch.sort(torch.from_numpy(np.asarray(out['cam_trans'], F))[:, 2], descending=True).indices
    v = org[order.to(dev)].clone()
    v[:, :, 2] = v[:, :, 2] * -1
    cam_z = torch.from_numpy(np.asarray(out['verts'], F) + np.asarray(out['cam_trans'], F)[:, None])[order][:, :, 2:].contiguous()
    direct = _np(Sim3DR().maps(v, faces.astype(np.int32), (h, w), attrs=cam_z, attr_bg=float('inf'), vert_labels=labels))
    order = order.numpy()
    assert np.array_equal(pm, np.where(direct['person_map'] >= 0, order[np.maximum(direct['person_map'], 0)], -1))
    assert np.array_equal(out['part_map'], direct['label_map']) and same(out['depth_map'], direct['attr_map'][:, :, 0])
    assert np.array_equal(out['verts_visible'][order], direct['vert_visible'].astype(bool))
    assert np.array_equal(out['person_pixels'][order], direct['person_pixels'])
    assert np.isposinf(out['depth_map'][pm < 0]).all() and np.isfinite(out['depth_map'][pm >= 0]).all()
    assert (out['part_map'][pm < 0] == 255).all() and (out['part_map'][pm >= 0] <= 23).all()
    assert 'verts_camed_org' not in out
    if rendered:
        img = out['rendered_image']
        assert np.array_equal(img[:, :w], frame)
        painted = (img[:, w:2 * w] != frame).any(2)
        assert painted.any() and (pm >= 0)[painted].all()
    else:
        assert 'rendered_image' not in out


@pytest.mark.gpu
def test_romp_dense_maps_end_to_end(dev):
    import romp_amd
    from oracle import romp_oracle as O
    from romp_amd.post_parser import body_mesh_projection2image
    from romp_amd.utils import img_preprocess_device
    settings = romp_amd.romp_settings(['--dense_maps', '--render_mesh'])
    settings.GPU, settings.center_thresh, settings.max_batch = 0, 1.25, 2
    faces = _faces()
    smpl = dict(O.make_synthetic_smpl(0), f=torch.from_numpy(faces).float())
    model = romp_amd.ROMP(settings, state_dict=O.make_romp_state_dict(0, center_bias=2.0), smpl_model=smpl)
    frame = np.random.RandomState(3).randint(0, 256, (360, 640, 3)).astype(np.uint8)
    labels = model.smpl_parser.smpl_model.part_labels
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (6890,)
    fast_calls = []
    inner = model._forward_fast
    model._forward_fast = lambda image: fast_calls.append(1) or inner(image)
    for rendered in (True, False):
        settings.render_mesh = rendered
        out = model(frame)
        assert out is not None and not fast_calls
        pad = img_preprocess_device(frame, dev)[1]
        t = lambda a: torch.from_numpy(np.asarray(a, F)).to(dev)
        org = body_mesh_projection2image(t(out['joints']), t(out['cam']), vertices=t(out['verts']), input2org_offsets=pad)['verts_camed_org']
        _check_result(out, frame, org, labels, faces, dev, rendered)
    on_keys = set(out)
    # off: the latency path again, with exactly the keys it had
    settings.dense_maps = False
    off = model(frame)
    assert fast_calls == [1]
    assert set(off) == {'cam', 'global_orient', 'body_pose', 'smpl_betas', 'smpl_thetas', 'center_preds', 'center_confs', 'cam_trans',
                        'verts', 'joints', 'pj2d_org'}
    assert not set(NEW_KEYS) & set(off) and set(NEW_KEYS) <= on_keys
    assert np.array_equal(off['verts'], out['verts'])
    # nobody in the frame: None as before
    settings.dense_maps = True
    model.centermap_parser.conf_thresh = 1e9
    assert model(frame) is None


def _first_detection(model, frame):
    for thresh in (0.9995, 0.999, 0.99, 0.9, 0.5, 0.2):
        model.model.centermap_parser.conf_thresh = thresh
        out = model(frame)
        if out is not None:
            return out
    return None


@pytest.mark.gpu
def test_bev_dense_maps_single_temporal_and_crowd(dev):
    from oracle import bev_oracle as BO
    from oracle import romp_oracle as O
    from romp_amd import bev, tracker
    from romp_amd.utils import img_preprocess_device
    tracker.Track.last_id = 0
    s = bev.bev_settings(['--dense_maps', '--render_mesh', '-t'])
    s.GPU, s.max_batch = 0, 2
    faces = _faces()
    smpla = dict(O.make_synthetic_smpl(0, 11), f=torch.from_numpy(faces).float())
    smil = dict(O.make_synthetic_smpl(5, 10), f=torch.from_numpy(faces).float())
    model = bev.BEV(s, state_dict=BO.make_bev_state_dict(0), smpla_model=smpla, smil_model=smil)
    labels = model.smpl_parser.smpl_model.part_labels                          # the adult table for every person
    t = lambda a: torch.from_numpy(np.asarray(a, F)).to(dev)
    frame = np.random.RandomState(2).randint(0, 256, (360, 640, 3)).astype(np.uint8)
    for temporal, rendered in ((False, True), (False, False), (True, True)):
        s.temporal_optimize, s.render_mesh = temporal, rendered
        out = _first_detection(model, frame)
        assert out is not None and ('track_ids' in out) == temporal
        org = model._verts_camed_org(t(out['verts']), t(out['cam_trans']), img_preprocess_device(frame, dev)[1])
        _check_result(out, frame, org, labels, faces, dev, rendered)
    on_keys = set(out)
    s.temporal_optimize, s.render_mesh, s.crowd = False, False, True
    wide = np.random.RandomState(1).randint(0, 256, (160, 480, 3)).astype(np.uint8)
    out = _first_detection(model, wide)
    assert out is not None
    org = model._verts_camed_org(t(out['verts']), t(out['cam_trans']), bev.crowd_pad_info(160, 480))
    _check_result(out, wide, org, labels, faces, dev, False)
    # off: the keys the result had
    s.crowd, s.dense_maps = False, False
    off = _first_detection(model, frame)
    assert off is not None and not set(NEW_KEYS) & set(off) and set(NEW_KEYS) <= on_keys
    s.dense_maps = True
    model.model.centermap_parser.conf_thresh = 1e9
    assert model(frame) is None
