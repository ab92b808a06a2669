"""Bird / side mesh views (vis_human/main.py:23-113 items mesh_bird_view / mesh_side_view, vis_utils.py:26-51
rotate_view_weak_perspective) and the batched Sim3DR render (renderer.py:120-133 in a fixed number of launches).
Fixture: tests/golden/render_views.npz, written by the reference's own rendering_romp_bev_results driving its own
Sim3DR (scripts/make_golden_render_views.py).  CPU part: a numpy restatement of the view transform and the oracle
renderer against the fixture.  GPU part: the device transform, romp_sim3dr_render_batch and the API end to end.
Bar: BIT-EXACT vertices, centres, scales and uint8 images."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import sim3dr_oracle as SO

F = np.float32
ALL_ITEMS = ['mesh', 'mesh_bird_view', 'mesh_side_view']


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'render_views.npz'))


def _rotation(rx, ry):
    """vis_utils.py:10-24: float32 matrices of float64 cos / sin of np.radians(angle)."""
    ax, ay = np.radians(rx), np.radians(ry)
    mx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]]).astype(F)
    my = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]]).astype(F)
    return mx, my


def _rotate(v, m):
    return np.stack([(v[..., 0] * m[k, 0] + v[..., 1] * m[k, 1]) + v[..., 2] * m[k, 2] for k in range(3)], -1).astype(F)


def view_np(verts, rx, ry, img_shape, expand_ratio=1.2):
    """rotate_view_weak_perspective in float32: Rx then Ry as two rounded steps, centre 0.5*(min+max), scale
    1/(float32(expand_ratio) * max|xy / (w/2, h/2)|), then *= scale and xy += (w/2, h/2)."""
    h, w = img_shape
    mx, my = _rotation(rx, ry)
    r = _rotate(_rotate(np.asarray(verts, F), mx), my)
    flat = r.reshape(-1, 3)
    c = F(0.5) * (flat.min(0) + flat.max(0))
    a = r - c
    half = np.array([w / 2, h / 2], F)
    scale = F(1) / (F(expand_ratio) * np.abs(a[..., :2] / half).max())
    a = a * scale
    a[..., :2] += half
    return a, c, scale


def _camera_space(verts, cam_trans):
    """verts + cam_trans in depth order (far first), z negated: the input of both views (main.py:41-45)."""
    order = torch.sort(torch.from_numpy(np.asarray(cam_trans, F)[:, 2]), descending=True).indices.numpy()
    vt = (np.asarray(verts, F) + np.asarray(cam_trans, F)[:, None])[order]
    vt[:, :, 2] *= -1
    return vt, order


def _view_panels(verts, cam_trans, faces, h, w, items):
    """The bird / side panels the reference draws for `items`, from the restatement + the oracle renderer."""
    from romp_amd.vis import mesh_color_left2right
    vt, order = _camera_space(verts, cam_trans)
    colors = mesh_color_left2right(torch.from_numpy(np.asarray(cam_trans, F)))[order]
    canvas = np.full((h, h, 3), 255, np.uint8)
    panels = []
    for it, rx, ry, shape in (('mesh_bird_view', -90, 0, (h, h)), ('mesh_side_view', 0, -90, (h, w))):
        if it in items:
            panels.append(SO.render_meshes(view_np(vt, rx, ry, shape)[0], faces, canvas, colors, use_ref=SO.load_ref() is not None))
    return panels


def _cases(g):
    return [(name,) + g[name + '_frame'].shape[:2] for name in ('wide', 'tall')]


# ------------------------------------------------------------------------------------------------ CPU
def test_view_restatement_matches_reference_fixture(golden_dir):
    g = _golden(golden_dir)
    for name, h, w in _cases(g):
        for view, rx, ry, shape in (('bird', -90, 0, (h, h)), ('side', 0, -90, (h, w))):
            v, c, s = view_np(g[name + '_verts_tran'], rx, ry, shape)
            assert np.array_equal(v, g['%s_%s_verts' % (name, view)]), (name, view)
            assert np.array_equal(c, g['%s_%s_center' % (name, view)]) and s == g['%s_%s_scale' % (name, view)], (name, view)
        vt, _ = _camera_space(g[name + '_verts'], g[name + '_cam_trans'])
        assert np.array_equal(vt, g[name + '_verts_tran'])


def test_torch_scalar_rounding_of_the_scale():
    """The scale is `1 / (expand_ratio * t)` on a float32 0-dim tensor: torch rounds 1.2 to float32 before the product and
    computes 1 / t as a float32 reciprocal -- what view_np and the device kernel do."""
    rs = np.random.RandomState(0)
    m = rs.uniform(0.01, 100, 20000).astype(F)
    t = torch.from_numpy(m)
    got = (1 / (1.2 * t)).numpy()
    assert np.array_equal(got, F(1) / (F(1.2) * m))
    assert not np.array_equal(got, (1 / (1.2 * m.astype(np.float64))).astype(F))   # the float64 reading differs somewhere


def test_oracle_renders_fixture_view_panels(golden_dir):
    g = _golden(golden_dir)
    tri = g['triangles']
    for name, h, w in _cases(g):
        img = g[name + '_rendered_image']
        assert img.shape == (h, 2 * w + 2 * h, 3)
        bird, side = _view_panels(g[name + '_verts'], g[name + '_cam_trans'], tri, h, w, ALL_ITEMS)
        assert np.array_equal(bird, img[:, 2 * w:2 * w + h]) and np.array_equal(side, img[:, 2 * w + h:])
        assert (bird != 255).any() and (side != 255).any()


def test_new_symbols_exported():
    from romp_amd import lib
    names = ['romp_sim3dr_render_batch', 'romp_view_weak_perspective']
    assert names == lib.VIEW_EXPORTS and not set(names) & set(lib.EXPORTS)
    h = lib.load()
    assert all(hasattr(h, n) for n in names) and h.romp_abi_version() == 7
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'romp_hip_views.h')).read()
    assert 'romp_sim3dr_render_batch(' in header and 'romp_view_weak_perspective(' in header


@pytest.mark.parametrize('item', ['pj2d', 'j3d', 'center_conf', 'tracking'])
def test_cv2_items_still_raise(item):
    from romp_amd.vis import rendering_romp_bev_results
    outputs = {'smpl_face': torch.zeros(1, 3), 'cam_trans': torch.zeros(1, 3)}
    with pytest.raises(NotImplementedError, match='OpenCV'):
        rendering_romp_bev_results(None, outputs, np.zeros((4, 4, 3), np.uint8),
                                   {'mesh_color': 'identity', 'items': ['mesh', item], 'renderer': 'sim3dr'})


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def _smpl_sized(n, seed, spread=400):
    """n ellipsoids of SMPL size (6808 vertices, 13612 faces) in camera space."""
    rs = np.random.RandomState(seed)
    base, tri = SO.ellipsoid_mesh(84, 82, [0, 0, 0], [1, 1, 1])
    r = np.stack([rs.uniform(0.2, 0.35, n), rs.uniform(0.7, 0.9, n), rs.uniform(0.15, 0.3, n)], 1)
    verts = (base[None] * r[:, None]).astype(F)
    trans = np.stack([rs.uniform(-2, 2, n), rs.uniform(-0.5, 0.5, n), rs.uniform(3, 3 + n / spread * 10, n)], 1).astype(F)
    return verts, trans, tri


@pytest.mark.gpu
def test_device_view_transform_vs_fixture(dev, golden_dir):
    from romp_amd.renderer import view_weak_perspective
    g = _golden(golden_dir)
    for name, h, w in _cases(g):
        vt = torch.from_numpy(g[name + '_verts_tran']).to(dev)
        for view, rx, ry, shape in (('bird', -90, 0, (h, h)), ('side', 0, -90, (h, w))):
            v, c, s = view_weak_perspective(vt, rx, ry, shape)
            assert np.array_equal(v.cpu().numpy(), g['%s_%s_verts' % (name, view)]), (name, view)
            assert np.array_equal(c.cpu().numpy(), g['%s_%s_center' % (name, view)]), (name, view)
            assert s.item() == g['%s_%s_scale' % (name, view)], (name, view)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 64])
def test_device_view_transform_smpl_sized(dev, n):
    from romp_amd.renderer import view_weak_perspective
    verts, trans, _ = _smpl_sized(n, seed=n)
    vt, _ = _camera_space(verts, trans)
    for rx, ry, shape in ((-90, 0, (720, 720)), (0, -90, (720, 1280))):
        v, c, s = view_weak_perspective(torch.from_numpy(vt).to(dev), rx, ry, shape)
        rv, rc, rsc = view_np(vt, rx, ry, shape)
        assert np.array_equal(v.cpu().numpy(), rv) and np.array_equal(c.cpu().numpy(), rc) and s.item() == rsc


def _batch_scene(n, seed, h=128, w=160):
    """n overlapping small meshes on a shared topology with exact ties: two copies of one triangle inside every mesh
    (the lower index wins) and meshes repeated verbatim (the later mesh wins)."""
    rs = np.random.RandomState(seed)
    base, tri = SO.ellipsoid_mesh(12, 16, [0, 0, 0], [1, 1, 1])
    tri = np.concatenate([tri, tri[:20]]).astype(np.int32)
    verts = []
    for i in range(n):
        if i >= 2 and i % 5 == 0:
            verts.append(verts[i - 2].copy())
            continue
        c = [rs.uniform(0.2, 0.8) * w, rs.uniform(0.2, 0.8) * h, rs.uniform(-30, 30)]
        r = [rs.uniform(10, 40), rs.uniform(15, 50), rs.uniform(10, 30)]
        verts.append((base * np.array(r)[None] + np.array(c)[None]).astype(F))
    bg = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    colors = rs.uniform(0.2, 1.0, (7, 3))
    return np.stack(verts), tri, bg, colors


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 2, 17, 64, 300])
def test_render_batch_vs_per_person_composition(dev, n):
    from romp_amd.renderer import Sim3DR
    verts, tri, bg, colors = _batch_scene(n, seed=n)
    img = Sim3DR()(verts, tri, bg, mesh_colors=colors)
    ref = SO.render_meshes(verts, tri, bg, colors, use_ref=SO.load_ref() is not None)
    nd = int((img != ref).sum())
    print('%d meshes: differing bytes %d, painted px %d' % (n, nd, int((ref != bg).any(2).sum())))
    assert nd == 0
    per_mesh = Sim3DR()(verts, [tri] * n, bg, mesh_colors=colors)                 # per-mesh triangles: N = 1 batches
    assert np.array_equal(per_mesh, ref)


@pytest.mark.gpu
def test_render_batch_at_the_triangle_bit_limit(dev):
    """4097 meshes take 13 key bits, leaving 19 for the triangle: 2^19 triangles fit (the last one's low bits are 0), one
    more is rejected.  Four meshes (first two, last two) are on the canvas; the others lie far outside it."""
    from romp_amd import lib as L
    from romp_amd.renderer import Sim3DR
    n, ntri, h, w = 4097, 1 << 19, 64, 80
    rs = np.random.RandomState(7)
    nver = 64
    tri = np.tile(np.array([[60, 61, 62]], np.int32), (ntri, 1))               # degenerate, off-canvas filler
    real = rs.randint(0, 56, (64, 3)).astype(np.int32)
    real[-1] = real[-2]                                                        # a depth tie at the very last two triangles
    tri[-64:] = real
    verts = np.full((n, nver, 3), -1e4, F)
    visible = [0, 1, n - 2, n - 1]
    for m in visible:
        verts[m, :56] = np.stack([rs.uniform(-5, w + 5, 56), rs.uniform(-5, h + 5, 56), rs.uniform(-20, 20, 56)], 1)
    verts[visible[-1], :56] = verts[visible[-2], :56]                          # the last mesh repeats the one before: it wins
    verts[visible[-1], :56, :2] += 0.25
    bg = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    colors = rs.uniform(0.2, 1.0, (n, 3))
    img = Sim3DR()(torch.from_numpy(verts).to(dev), tri, bg, mesh_colors=colors)
    ref = SO.render_meshes(verts[visible], tri, bg, colors[visible], use_ref=SO.load_ref() is not None)
    nd = int((img != ref).sum())
    print('limit case: differing bytes %d, painted px %d' % (nd, int((ref != bg).any(2).sum())))
    assert nd == 0 and (ref != bg).any()
    # one triangle more does not fit: rejected before any launch
    buf = torch.zeros(16, dtype=torch.float32, device=dev)
    keys = torch.zeros(4, dtype=torch.int64, device=dev)
    img_d = torch.zeros((2, 2, 3), dtype=torch.uint8, device=dev)
    cfg = (ctypes.c_float * 14)()
    rc = L.load().romp_sim3dr_render_batch(L.ptr(img_d), 2, 2, L.ptr(buf), n, 1, L.ptr(buf), ntri + 1, L.ptr(buf), L.ptr(buf),
                                           L.ptr(buf), cfg, L.ptr(buf), L.ptr(buf), L.ptr(keys), L.stream_ptr(dev))
    assert rc != 0 and b'key bits' in L.load().romp_last_error()
    torch.cuda.synchronize()


def _fixture_outputs(g, name, dev):
    return {'smpl_face': torch.from_numpy(g['triangles'].astype(np.int64)).to(dev),
            'cam_trans': torch.from_numpy(g[name + '_cam_trans']).to(dev), 'verts': torch.from_numpy(g[name + '_verts']).to(dev),
            'verts_camed_org': torch.from_numpy(g[name + '_verts_camed_org']).to(dev)}


@pytest.mark.gpu
def test_rendering_results_vs_reference_fixture(dev, golden_dir):
    from romp_amd.renderer import Sim3DR
    from romp_amd.vis import rendering_romp_bev_results
    g = _golden(golden_dir)
    renderer = Sim3DR()
    for name, h, w in _cases(g):
        frame, want = g[name + '_frame'], g[name + '_rendered_image']
        for items in (ALL_ITEMS, ['mesh_side_view', 'mesh', 'mesh_bird_view'], ['mesh_bird_view', 'mesh_side_view', 'mesh']):
            cfgs = {'mesh_color': 'identity', 'items': items, 'renderer': 'sim3dr'}
            got = rendering_romp_bev_results(renderer, _fixture_outputs(g, name, dev), frame.copy(), cfgs)['rendered_image']
            assert got.shape == want.shape and np.array_equal(got, want), (name, items, int((got != want).sum()))
        cfgs = {'mesh_color': 'identity', 'items': ['mesh_bird_view'], 'renderer': 'sim3dr'}
        got = rendering_romp_bev_results(renderer, _fixture_outputs(g, name, dev), frame.copy(), cfgs)['rendered_image']
        assert np.array_equal(got, np.concatenate([frame, want[:, 2 * w:2 * w + h]], 1)), name


def _faces():
    _, base_tri = SO.ellipsoid_mesh(84, 82, [0, 0, 0], [1, 1, 1])
    faces = np.zeros((13776, 3), np.int64)                                   # a real closed surface over the first 6808 vertices
    faces[:len(base_tri)] = base_tri
    return faces


def _check_views(out, frame, faces, items, mesh_panels):
    h, w = frame.shape[:2]
    img = out['rendered_image']
    nviews = sum(it in items for it in ('mesh_bird_view', 'mesh_side_view'))
    assert img.shape == (h, w + mesh_panels * w + nviews * h, 3) and np.array_equal(img[:, :w], frame)
    panels = _view_panels(out['verts'], out['cam_trans'], faces.astype(np.int32), h, w, items)
    x0 = w + mesh_panels * w
    for i, ref in enumerate(panels):
        got = img[:, x0 + i * h:x0 + (i + 1) * h]
        nd = int((got != ref).sum())
        print('view panel %d: %d persons, differing bytes %d, painted px %d' % (i, len(out['cam_trans']), nd, int((ref != 255).any(2).sum())))
        assert nd == 0 and (ref != 255).any()


@pytest.mark.gpu
def test_romp_render_views_end_to_end(dev):
    import romp_amd
    from oracle import romp_oracle as O
    settings = romp_amd.romp_settings(['--render_mesh', '--show_items', ','.join(ALL_ITEMS)])
    settings.GPU, settings.center_thresh = 0, 1.25
    faces = _faces()
    smpl = dict(O.make_synthetic_smpl(0), f=torch.from_numpy(faces).float())
    model = romp_amd.ROMP(settings, state_dict=O.make_romp_state_dict(0, center_bias=2.0), smpl_model=smpl)
    frame = np.random.RandomState(3).randint(0, 256, (360, 640, 3)).astype(np.uint8)
    out = model(frame)
    assert out is not None
    _check_views(out, frame, faces, ALL_ITEMS, 1)


def _bev_model(args):
    from oracle import bev_oracle as BO
    from oracle import romp_oracle as O
    from romp_amd import bev
    s = bev.bev_settings(args)
    s.GPU, s.max_batch = 0, 4
    faces = _faces()
    smpla = dict(O.make_synthetic_smpl(0, 11), f=torch.from_numpy(faces).float())
    smil = dict(O.make_synthetic_smpl(5, 10), f=torch.from_numpy(faces).float())
    return bev.BEV(s, state_dict=BO.make_bev_state_dict(0), smpla_model=smpla, smil_model=smil), faces


def _first_detection(model, frame):
    for thresh in (0.9995, 0.999, 0.99, 0.9, 0.5, 0.2):
        model.model.centermap_parser.conf_thresh = thresh
        out = model(frame)
        if out is not None:
            return out
    return None


@pytest.mark.gpu
def test_bev_render_views_end_to_end(dev):
    model, faces = _bev_model(['--render_mesh', '--show_items', ','.join(ALL_ITEMS)])
    frame = np.random.RandomState(2).randint(0, 256, (360, 640, 3)).astype(np.uint8)
    out = _first_detection(model, frame)
    assert out is not None
    _check_views(out, frame, faces, ALL_ITEMS, 1)


@pytest.mark.gpu
def test_bev_crowd_render_views(dev):
    model, faces = _bev_model(['--crowd', '--render_mesh', '--show_items', 'mesh,mesh_bird_view'])
    frame = np.random.RandomState(1).randint(0, 256, (160, 480, 3)).astype(np.uint8)
    out = _first_detection(model, frame)
    assert out is not None and 'verts_camed_org' not in out
    _check_views(out, frame, faces, ['mesh', 'mesh_bird_view'], 1)
