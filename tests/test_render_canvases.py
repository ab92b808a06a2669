"""Many canvases in one pass (include/romp_hip_canvases.h): romp_sim3dr_render_canvases, the turntable transform
romp_view_turntable, and what vis.py builds on them (rendering_mesh_rotating_view, render_mesh_frames, the show item
'rotate_mesh').  Every canvas has an exact single-canvas equivalent (Sim3DR.__call__, romp_sim3dr_render_batch[_tex]), so
the bar is BIT-EXACT everywhere: images, keys, vertices, centres and scales.  CPU part: the exports, a numpy restatement of
the turntable transform and the angle schedule.  GPU part: the device code against the single-canvas calls, the oracle
renderer and the restatement."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import sim3dr_oracle as SO

F = np.float32
H, W = 128, 160


def _rotate(v, m):
    return np.stack([(v[..., 0] * m[k, 0] + v[..., 1] * m[k, 1]) + v[..., 2] * m[k, 2] for k in range(3)], -1).astype(F)


def _matrices(azimuth, tilt):
    """float32 matrices of float64 cos / sin of np.radians(angle): Ry(azimuth), Rx(tilt)."""
    ay, ax = np.radians(azimuth), np.radians(tilt)
    my = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]]).astype(F)
    mx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]]).astype(F)
    return my, mx


def turntable_np(verts, azimuths, tilts, img_shape, expand_ratio=1.2, order=None):
    """The turntable transform in float32, steps 1-6: c0 = 0.5*(min+max) of the unrotated points; a = v - c0;
    r_k = Rx(tilt_k) . (Ry(azimuth_k) . a) as two rounded steps; ONE scale 1/(float32(expand_ratio) * max over all views of
    |r_k.xy / (w/2, h/2)|); out[k, j] = r_k[order[k, j]] * scale, xy += (w/2, h/2).  -> (out (K,n,V,3), c0, scale)."""
    h, w = img_shape
    v = np.asarray(verts, F)
    tilts = np.broadcast_to(np.asarray(tilts, np.float64).reshape(-1), (len(azimuths),))
    flat = v.reshape(-1, 3)
    c0 = F(0.5) * (flat.min(0) + flat.max(0))
    a = v - c0
    r = []
    for az, ti in zip(azimuths, tilts):
        my, mx = _matrices(az, ti)
        r.append(_rotate(_rotate(a, my), mx))
    r = np.stack(r)
    half = np.array([w / 2, h / 2], F)
    scale = F(1) / (F(expand_ratio) * np.abs(r[..., :2] / half).max())
    if order is not None:
        r = np.stack([rk[np.asarray(o)] for rk, o in zip(r, order)])
    out = r * scale
    out[..., :2] += half
    return out, c0, scale


def _batch_scene(n, seed, h=H, w=W):
    """n overlapping small meshes on a shared topology with exact ties: two copies of one triangle inside every mesh
    (the lower index wins) and meshes repeated verbatim (the later mesh wins).  (As in tests/test_render_views.py.)"""
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


# ------------------------------------------------------------------------------------------------ CPU
def test_canvas_symbols_exported():
    from romp_amd import lib
    names = ['romp_sim3dr_render_canvases', 'romp_view_turntable']
    assert names == lib.CANVAS_EXPORTS
    others = lib.EXPORTS + lib.VIEW_EXPORTS + lib.MAP_EXPORTS + lib.TEXTURE_EXPORTS + lib.EVAL_EXPORTS + lib.RH_EXPORTS
    assert not set(names) & set(others)
    h = lib.load()
    assert h.romp_abi_version() == 7 == lib.ABI_VERSION
    for n in names:
        assert getattr(h, n).argtypes is not None and getattr(h, n).restype is ctypes.c_int, n
    assert len(h.romp_sim3dr_render_canvases.argtypes) == 21 and len(h.romp_view_turntable.argtypes) == 14
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'romp_hip_canvases.h')).read()
    assert all(n + '(' in header for n in names)


def test_turntable_restatement_is_a_rotation_about_the_centre():
    rs = np.random.RandomState(0)
    v = rs.uniform(-1, 1, (3, 50, 3)).astype(F) * np.array([2, 1, 0.5], F) + np.array([0.3, -0.2, 4], F)
    az = [0, 30, 90, 180, 275, 360]
    out, c0, scale = turntable_np(v, az, 0., (H, W))
    flat = v.reshape(-1, 3)
    assert np.array_equal(c0, F(0.5) * (flat.min(0) + flat.max(0)))
    half = np.array([W / 2, H / 2, 0], F)
    a = (v - c0).astype(np.float64)
    for k, deg in enumerate(az):
        back = (out[k].astype(np.float64) - half) / float(scale)            # the rotated, unscaled points
        t = np.radians(deg)
        ry = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
        assert np.allclose(back, a @ ry.T, atol=2e-5), deg                   # a pure rotation about c0 (float32 rounding)
        assert np.allclose(np.linalg.norm(back, axis=-1), np.linalg.norm(a, axis=-1), atol=2e-5)
        assert np.allclose(back[..., 1], a[..., 1], atol=1e-6), deg          # the vertical axis is the spin axis
    # azimuth 0 is the identity: the centred points, scaled and shifted, exactly
    want = (v - c0) * scale
    want[..., :2] += half[:2]
    assert np.array_equal(out[0], want)
    # ONE scale: the largest |xy| / half over ALL views is 1 / expand_ratio, and no single view exceeds it
    ext = np.abs((out[..., :2] - half[:2]) / half[:2]).reshape(len(az), -1).max(1)
    assert abs(ext.max() - 1 / 1.2) < 1e-5 and (ext[:-1] <= ext.max()).all() and ext.min() < ext.max() - 1e-3
    # the spin comes first, then the tilt: with a tilt the heights of a spun scene differ from the rotate-then-spin order
    tilted, _, s2 = turntable_np(v, [90], [-20], (H, W))
    my, mx = _matrices(90, -20)
    assert np.array_equal(tilted[0, ..., 2], _rotate(_rotate(v - c0, my), mx)[..., 2] * s2)
    assert not np.allclose(tilted[0, ..., 2], _rotate(_rotate(v - c0, mx), my)[..., 2] * s2, atol=1e-3)
    # an order only permutes the slots of each view
    order = [rs.permutation(3) for _ in az]
    perm = turntable_np(v, az, 0., (H, W), order=order)[0]
    assert all(np.array_equal(perm[k], out[k][order[k]]) for k in range(len(az)))


def test_turntable_angles_schedule():
    from romp_amd.vis import turntable_angles
    a = turntable_angles()
    want = [0.] * 24 + [5. * (i + 1) for i in range(72)]
    assert a.shape == (96,) and a.tolist() == want
    assert (a[:24] == 0).all() and a[24] == 5 and a[-1] == 360 and (np.diff(a[23:]) == 5).all()
    assert turntable_angles(pause=2, step=45).tolist() == [0, 0, 45, 90, 135, 180, 225, 270, 315, 360]


def test_rotate_mesh_is_a_device_item_and_a_setting():
    import romp_amd
    from romp_amd import bev
    from romp_amd.vis import DEVICE_ITEMS
    assert DEVICE_ITEMS == ('mesh', 'mesh_bird_view', 'mesh_side_view', 'rotate_mesh')
    assert romp_amd.romp_settings([]).rotate_size == 512 and bev.bev_settings([]).rotate_size == 512
    assert romp_amd.romp_settings(['--rotate_size', '96']).rotate_size == 96 and bev.bev_settings(['--rotate_size', '96']).rotate_size == 96


def test_result_saver_writes_the_turntable(tmp_path):
    from romp_amd.utils import ResultSaver, convert_tensor2numpy
    frames = np.arange(2 * 4 * 4 * 3, dtype=np.uint8).reshape(2, 4, 4, 3)
    out = convert_tensor2numpy({'rotate_mesh_frames': frames, 'cam_trans': torch.zeros(1, 3)})
    assert out['rotate_mesh_frames'] is frames
    ResultSaver(mode='image', save_path=str(tmp_path))(out, 'some/frame_07.jpg')
    assert 'rotate_mesh_frames' not in out
    assert np.array_equal(np.load(str(tmp_path / 'frame_07_rotate.npy')), frames)
    saved = np.load(str(tmp_path / 'frame_07.npz'), allow_pickle=True)['results'][()]
    assert 'rotate_mesh_frames' not in saved and 'cam_trans' in saved


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


COUNTS = [1, 0, 2, 17, 0]                                                 # mesh bits 0, -, 1, 5, -: empty in the middle and at the end


@pytest.fixture(scope='module')
def scene():
    """20 slots on 5 canvases with distinct random backgrounds; the verbatim repeats (slots 5, 10, 15) lie inside canvas 3."""
    n = sum(COUNTS)
    verts, tri, _, _ = _batch_scene(n, seed=20)
    rs = np.random.RandomState(5)
    bgs = rs.randint(0, 256, (len(COUNTS), H, W, 3)).astype(np.uint8)
    colors = rs.uniform(0.2, 1.0, (n, 3))
    vert_colors = rs.uniform(0, 1, verts.shape).astype(F)
    offsets = np.concatenate([[0], np.cumsum(COUNTS)])
    return verts, tri, bgs, colors, vert_colors, offsets


def _single(renderer, verts, tri, bg, colors, vert_colors, dev):
    """(image, keys) of the single-canvas call on one slice; no slot: the canvas itself and keys of 0."""
    keys = torch.zeros(H * W, dtype=torch.int64, device=dev)
    img = renderer(verts, tri, bg, mesh_colors=colors, vert_colors=vert_colors, keys=keys) if len(verts) else bg.copy()
    return img, keys.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['plain', 'vert_colors', 'specular2', 'rows'])
def test_canvases_vs_single_canvas_calls(dev, scene, mode):
    from romp_amd.renderer import Sim3DR
    verts, tri, bgs, colors, vert_colors, offsets = scene
    n, C = len(verts), len(COUNTS)
    renderer = Sim3DR(specular_exp=2) if mode == 'specular2' else Sim3DR()
    vc = vert_colors if mode in ('vert_colors', 'rows') else None
    rows = np.random.RandomState(9).permutation(n) if mode == 'rows' else None
    keys = torch.full((C, H, W), -1, dtype=torch.int64, device=dev)
    offs = torch.from_numpy(offsets.astype(np.int32)).to(dev) if mode == 'plain' else offsets      # device and host offsets
    bgs_before = bgs.copy()
    got = renderer.render_canvases(verts, tri, bgs, offs, mesh_colors=colors, vert_colors=vc, rows=rows, keys=keys)
    assert got.shape == (C, H, W, 3) and got.dtype == np.uint8 and np.array_equal(bgs, bgs_before)
    got_keys = keys.cpu().numpy().reshape(C, H * W)
    use_ref = SO.load_ref() is not None
    for c in range(C):
        sl = slice(offsets[c], offsets[c + 1])
        pick = rows[sl] if rows is not None else np.arange(n)[sl]            # the colour row of every slot of the slice
        img, k = _single(renderer, verts[sl], tri, bgs[c], colors[pick], None if vc is None else vc[pick], dev)
        nd = int((got[c] != img).sum())
        print('%s canvas %d: %d slots, differing bytes %d, differing keys %d, painted px %d'
              % (mode, c, COUNTS[c], nd, int((got_keys[c] != k).sum()), int((img != bgs[c]).any(2).sum())))
        assert nd == 0 and np.array_equal(got_keys[c], k)
        if COUNTS[c]:
            assert (got[c] != bgs[c]).any()                                  # a blank result cannot pass
        else:
            assert np.array_equal(got[c], bgs[c]) and not got_keys[c].any()
        if vc is None and mode != 'specular2':
            assert np.array_equal(got[c], SO.render_meshes(verts[sl], tri, bgs[c], colors[pick], use_ref=use_ref) if COUNTS[c] else bgs[c])
    # the keys of a canvas serve the dense maps of its slice
    sl = slice(offsets[3], offsets[4])
    a = renderer.maps(verts[sl], tri, (H, W), keys=keys[3].reshape(-1))
    b = renderer.maps(verts[sl], tri, (H, W))
    assert all(torch.equal(a[m], b[m]) for m in b) and int((b['person_map'] >= 0).sum()) > 0


@pytest.mark.gpu
def test_single_canvas_is_render_batch(dev):
    from romp_amd.renderer import Sim3DR
    verts, tri, bg, colors = _batch_scene(17, seed=17)
    k0 = torch.zeros(H * W, dtype=torch.int64, device=dev)
    k1 = torch.zeros(H * W, dtype=torch.int64, device=dev)
    ref = Sim3DR()(verts, tri, bg, mesh_colors=colors, keys=k0)               # romp_sim3dr_render_batch
    got = Sim3DR().render_canvases(verts, tri, bg[None], [0, 17], mesh_colors=colors, keys=k1)
    assert got.shape == (1, H, W, 3) and np.array_equal(got[0], ref) and torch.equal(k0, k1) and (ref != bg).any()
    # one (h,w,3) canvas is repeated; a device tensor comes back with return_tensor
    t = Sim3DR().render_canvases(torch.from_numpy(verts).to(dev), tri, torch.from_numpy(bg).to(dev), [0, 17, 17], mesh_colors=colors,
                                 return_tensor=True)
    assert torch.is_tensor(t) and t.is_cuda and tuple(t.shape) == (2, H, W, 3)
    assert np.array_equal(t[0].cpu().numpy(), ref) and np.array_equal(t[1].cpu().numpy(), bg)


@pytest.mark.gpu
@pytest.mark.parametrize('device_offsets', [False, True])
def test_chunked_canvases_equal_unchunked(dev, device_offsets):
    from romp_amd.renderer import Sim3DR
    verts, tri, _, colors = _batch_scene(7, seed=3)
    rs = np.random.RandomState(1)
    bgs = rs.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    vc = rs.uniform(0, 1, verts.shape).astype(F)
    offsets = np.array([0, 3, 4, 7], np.int32)
    offs = torch.from_numpy(offsets).to(dev) if device_offsets else offsets
    k_all = torch.zeros((3, H, W), dtype=torch.int64, device=dev)
    k_chunk = torch.full((3, H, W), -1, dtype=torch.int64, device=dev)
    whole = Sim3DR().render_canvases(verts, tri, bgs, offs, mesh_colors=colors, vert_colors=vc, keys=k_all)
    chunked = Sim3DR(max_canvases=2).render_canvases(verts, tri, bgs, offs, mesh_colors=colors, vert_colors=vc, keys=k_chunk)
    assert np.array_equal(whole, chunked) and torch.equal(k_all, k_chunk)
    assert np.array_equal(Sim3DR(max_canvases=1).render_canvases(verts, tri, bgs, offs, mesh_colors=colors, vert_colors=vc), whole)
    assert all((whole[c] != bgs[c]).any() for c in range(3))


def _abi_args(renderer, verts_d, tri, colors, dev):
    from romp_amd import renderer as R
    topo = R._topology(tri, verts_d.shape[1], dev)
    amb = torch.from_numpy(renderer._ambient(colors)).to(dev)
    return topo, amb, renderer._light_cfg(colors[:1])


@pytest.mark.gpu
def test_offsets_cannot_leave_the_buffers(dev):
    """Offsets below 0, above n and decreasing: each is clamped to [0, n], a decreasing pair is an empty canvas.  Guard bytes
    around `images` and guard words around `keys` stay intact and the empty canvases keep their bytes."""
    from romp_amd import lib as L
    from romp_amd.renderer import Sim3DR
    n, C, guard = 6, 4, 4096
    verts, tri, _, _ = _batch_scene(n, seed=6)
    rs = np.random.RandomState(2)
    colors = rs.uniform(0.2, 1.0, (n, 3))
    bgs = rs.randint(0, 256, (C, H, W, 3)).astype(np.uint8)
    renderer = Sim3DR()
    verts_d = torch.from_numpy(verts).to(dev)
    topo, amb, cfg = _abi_args(renderer, verts_d, tri, colors, dev)
    img_buf = torch.full((guard + bgs.size + guard,), 0xA5, dtype=torch.uint8, device=dev)
    img_buf[guard:guard + bgs.size] = torch.from_numpy(bgs).to(dev).reshape(-1)
    key_buf = torch.full((guard + C * H * W + guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    off = torch.tensor([-3, 2, 1, 9, 4], dtype=torch.int32, device=dev)      # canvases: [0,2), empty (2 > 1), [1,6) (9 -> 6), empty
    normals, light = torch.empty_like(verts_d), torch.empty_like(verts_d)
    images, keys = img_buf[guard:guard + bgs.size], key_buf[guard:guard + C * H * W]
    rc = L.load().romp_sim3dr_render_canvases(L.ptr(images), C, H, W, L.ptr(verts_d), n, topo.nver, L.ptr(off), L.ptr(topo.tri), topo.ntri,
                                              L.ptr(topo.adj_off), L.ptr(topo.adj_ent), L.ptr(amb), cfg, None, None, 1, L.ptr(normals),
                                              L.ptr(light), L.ptr(keys), L.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((img_buf[:guard] == 0xA5).all()) and bool((img_buf[-guard:] == 0xA5).all())
    assert bool((key_buf[:guard] == 0x5A5A5A5A5A5A5A5A).all()) and bool((key_buf[-guard:] == 0x5A5A5A5A5A5A5A5A).all())
    got = images.reshape(C, H, W, 3).cpu().numpy()
    got_keys = keys.reshape(C, H * W).cpu().numpy()
    for c, (lo, hi) in enumerate([(0, 2), (0, 0), (1, 6), (0, 0)]):
        img, k = _single(renderer, verts[lo:hi], tri, bgs[c], colors[lo:hi], None, dev)
        assert np.array_equal(got[c], img) and np.array_equal(got_keys[c], k), c
        assert (hi > lo) == bool((got[c] != bgs[c]).any())


@pytest.mark.gpu
def test_host_checks_before_any_launch(dev):
    from romp_amd import lib as L
    buf = torch.zeros(16, dtype=torch.float32, device=dev)
    keys = torch.zeros(4, dtype=torch.int64, device=dev)
    img = torch.full((2, 2, 3), 7, dtype=torch.uint8, device=dev)
    off = torch.zeros(2, dtype=torch.int32, device=dev)
    cfg = (ctypes.c_float * 14)()
    h = L.load()

    def call(n, ntri, spec, images=img):
        return h.romp_sim3dr_render_canvases(L.ptr(images), 1, 2, 2, L.ptr(buf), n, 1, L.ptr(off), L.ptr(buf), ntri, L.ptr(buf),
                                             L.ptr(buf), L.ptr(buf), cfg, None, None, spec, L.ptr(buf), L.ptr(buf), L.ptr(keys),
                                             L.stream_ptr(dev))
    assert call(4097, (1 << 19) + 1, 1) != 0 and b'key bits' in h.romp_last_error()     # 13 mesh bits leave 19 for the triangle
    assert call(1, 4, 0) != 0 and b'specular_exp' in h.romp_last_error()
    assert call(1, 4, 1, images=None) != 0 and b'bad arguments' in h.romp_last_error()
    assert call(0, 4, 1) != 0 and b'bad arguments' in h.romp_last_error()
    az = (ctypes.c_double * 1)(0.)
    assert h.romp_view_turntable(L.ptr(buf), 1, 1, 0, az, az, None, 2, 2, 1.2, L.ptr(buf), L.ptr(buf), L.ptr(buf), L.stream_ptr(dev)) != 0
    assert b'romp_view_turntable' in h.romp_last_error()
    torch.cuda.synchronize()
    assert bool((img == 7).all()) and not bool(keys.any())                   # nothing ran


def _small_scene_3d(n, seed):
    """n small ellipsoids in camera space (z negated: greater z is nearer)."""
    rs = np.random.RandomState(seed)
    base, tri = SO.ellipsoid_mesh(12, 16, [0, 0, 0], [1, 1, 1])
    r = np.stack([rs.uniform(0.2, 0.35, n), rs.uniform(0.6, 0.9, n), rs.uniform(0.15, 0.3, n)], 1)
    c = np.stack([rs.uniform(-1.5, 1.5, n), rs.uniform(-0.3, 0.3, n), rs.uniform(-6, -3, n)], 1)
    return (base[None] * r[:, None] + c[:, None]).astype(F), tri.astype(np.int32)


def _smpl_sized_3d(n, seed):
    rs = np.random.RandomState(seed)
    base, tri = SO.ellipsoid_mesh(84, 82, [0, 0, 0], [1, 1, 1])            # 6808 vertices
    r = np.stack([rs.uniform(0.2, 0.35, n), rs.uniform(0.7, 0.9, n), rs.uniform(0.15, 0.3, n)], 1)
    c = np.stack([rs.uniform(-2, 2, n), rs.uniform(-0.5, 0.5, n), rs.uniform(-8, -3, n)], 1)
    return (base[None] * r[:, None] + c[:, None]).astype(F), tri.astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['n1', 'n3', 'smpl2'])
def test_turntable_views_vs_restatement(dev, case):
    from romp_amd.renderer import turntable_views
    if case == 'smpl2':
        verts, _ = _smpl_sized_3d(2, seed=4)
        az, tilts, shape = [0, 77.5, 180, 300], [-20, -20, 10, 0], (512, 512)
    else:
        verts, _ = _small_scene_3d(1 if case == 'n1' else 3, seed=11)
        az, tilts, shape = [0, 90, 180, 360, 37.5, -120, 275], [0, -20, 0, 15, -20, 33, 0], (H, W)
    assert case != 'smpl2' or verts.shape[1] == 6808
    n, K = len(verts), len(az)
    vd = torch.from_numpy(verts).to(dev)
    rs = np.random.RandomState(8)
    order = np.stack([rs.permutation(n) for _ in range(K)])
    for o in (None, order):
        v, c, s = turntable_views(vd, az, tilts, shape, order=None if o is None else torch.from_numpy(o).to(dev))
        rv, rc, rsc = turntable_np(verts, az, tilts, shape, order=o)
        assert tuple(v.shape) == (K, n) + verts.shape[1:]
        assert np.array_equal(v.cpu().numpy(), rv) and np.array_equal(c.cpu().numpy(), rc) and s.item() == rsc
    # one tilt for all views
    v1 = turntable_views(vd, az, -20., shape)[0]
    assert np.array_equal(v1.cpu().numpy(), turntable_np(verts, az, -20., shape)[0])


def _turntable_scene():
    """Three people: an overlapping pair one behind the other (B nearer at azimuth 0, A nearer at 180) and one to the side."""
    base, tri = SO.ellipsoid_mesh(12, 16, [0, 0, 0], [1, 1, 1])
    centres = np.array([[0., 0., -0.5], [0.1, 0., 0.5], [1.3, 0.1, 0.15]])
    radii = np.array([[0.3, 0.45, 0.3], [0.3, 0.45, 0.3], [0.25, 0.5, 0.2]])
    verts = (base[None] * radii[:, None] + centres[:, None]).astype(F)
    colors = np.array([[1.0, 0.3, 0.2], [0.2, 0.4, 1.0], [0.3, 0.9, 0.3]])
    return verts, tri.astype(np.int32), colors


def _view_orders(verts, az, tilt):
    """Per view the persons far to near (ascending z of the rotated centroid), with the smallest depth gap over the extent."""
    cen = verts.astype(np.float64).mean(1)
    extent = float((verts.reshape(-1, 3).max(0) - verts.reshape(-1, 3).min(0)).max())
    orders, gap = [], np.inf
    for deg in az:
        a, t = np.radians(deg), np.radians(tilt)
        z = cen[:, 1] * np.sin(t) + (cen[:, 2] * np.cos(a) - cen[:, 0] * np.sin(a)) * np.cos(t)
        orders.append(np.argsort(z, kind='stable'))
        gap = min(gap, float(np.diff(np.sort(z)).min()) / extent)
    return np.stack(orders), gap


@pytest.mark.gpu
def test_turntable_frames(dev):
    from romp_amd.renderer import Sim3DR, turntable_views
    from romp_amd.vis import rendering_mesh_rotating_view
    verts, tri, colors = _turntable_scene()
    az, tilt = [0, 60, 135, 180, 270, 360], -20.
    orders, gap = _view_orders(verts, az, tilt)
    print('turntable: smallest centroid depth gap / extent %.4f' % gap)
    assert gap > 1e-3                                                      # no order here hangs on a rounding
    assert orders[0].tolist() == [0, 2, 1] and orders[3].tolist() == [1, 2, 0]
    vd = torch.from_numpy(verts).to(dev)
    renderer = Sim3DR()
    frames = rendering_mesh_rotating_view(renderer, vd, tri, (H, W), colors, azimuths=az, tilt=tilt)
    assert frames.shape == (len(az), H, W, 3) and frames.dtype == np.uint8
    white = np.full((H, W, 3), 255, np.uint8)
    views = turntable_views(vd, az, tilt, (H, W))[0]                         # mesh order; slots are taken below
    assert np.array_equal(views.cpu().numpy(), turntable_np(verts, az, tilt, (H, W))[0])
    for k in range(len(az)):
        o = orders[k]
        want = renderer(views[k][torch.from_numpy(o).to(dev)], tri, white, mesh_colors=colors[o])
        assert np.array_equal(frames[k], want), k
        assert (want != 255).any()
    assert np.array_equal(frames[0], frames[5])                              # azimuth 0 and 360
    # the overlapping pair at the pixel their midpoint projects to: B (1) covers A (0) in front, A covers B from behind
    mid = np.array([[[0.05, 0., 0.]]], F)
    scene = np.concatenate([verts.reshape(1, -1, 3), mid], 1)               # the midpoint rides along (inside the bbox: c0 unchanged)
    proj = turntable_np(scene, az, tilt, (H, W))[0][:, 0, -1]
    assert np.array_equal(turntable_np(scene, az, tilt, (H, W))[1], turntable_np(verts, az, tilt, (H, W))[1])
    for k, near, far in ((0, 1, 0), (3, 0, 1)):
        x, y = int(round(float(proj[k, 0]))), int(round(float(proj[k, 1])))
        alone = [renderer(views[k][m:m + 1], tri, white, mesh_colors=colors[m:m + 1])[y, x] for m in (near, far)]
        assert (alone[0] != 255).any() and (alone[1] != 255).any() and (alone[0] != alone[1]).any()   # both cover it, differently
        assert np.array_equal(frames[k][y, x], alone[0]), (k, x, y)
    # part colours follow the person; no person: white frames
    vc = np.random.RandomState(3).uniform(0, 1, verts.shape).astype(F)
    tex = rendering_mesh_rotating_view(renderer, vd, tri, (H, W), np.ones((3, 3)), vert_colors=vc, azimuths=az[:2], tilt=tilt)
    o = orders[1]
    want = renderer(views[1][torch.from_numpy(o).to(dev)], tri, white, mesh_colors=np.ones((3, 3)), vert_colors=vc[o])
    assert np.array_equal(tex[1], want)
    empty = rendering_mesh_rotating_view(renderer, vd[:0], tri, (8, 9), colors, azimuths=az)
    assert empty.shape == (6, 8, 9, 3) and (empty == 255).all()


def _faces():
    _, base_tri = SO.ellipsoid_mesh(84, 82, [0, 0, 0], [1, 1, 1])
    faces = np.zeros((13776, 3), np.int64)                                   # a real closed surface over the first 6808 vertices
    faces[:len(base_tri)] = base_tri
    return faces


def _check_rotate(out, plain, faces, dev):
    """`out`: a run with rotate_mesh; `plain`: the same frame without it."""
    from romp_amd.renderer import Sim3DR
    from romp_amd.vis import mesh_color_left2right, rendering_mesh_rotating_view
    frames = out['rotate_mesh_frames']
    assert isinstance(frames, np.ndarray) and frames.shape == (96, 96, 96, 3) and frames.dtype == np.uint8
    assert 'rotate_mesh_frames' not in plain and np.array_equal(out['rendered_image'], plain['rendered_image'])
    cam_trans = torch.from_numpy(np.asarray(out['cam_trans'], F))
    vt = (torch.from_numpy(np.asarray(out['verts'], F)) + cam_trans.unsqueeze(1)).to(dev)
    vt[:, :, 2] = vt[:, :, 2] * -1
    want = rendering_mesh_rotating_view(Sim3DR(), vt, faces.astype(np.int32), (96, 96), mesh_color_left2right(cam_trans))
    nd = int((frames != want).sum())
    print('rotate_mesh: %d persons, differing bytes %d, painted px %d' % (len(cam_trans), nd, int((want != 255).any(3).sum())))
    assert nd == 0 and (want != 255).any() and np.array_equal(frames[0], frames[95])


@pytest.mark.gpu
def test_romp_rotate_mesh_end_to_end(dev):
    import romp_amd
    from oracle import romp_oracle as O
    settings = romp_amd.romp_settings(['--render_mesh', '--show_items', 'mesh,rotate_mesh', '--rotate_size', '96'])
    settings.GPU, settings.center_thresh = 0, 1.25
    faces = _faces()
    smpl = dict(O.make_synthetic_smpl(0), f=torch.from_numpy(faces).float())
    model = romp_amd.ROMP(settings, state_dict=O.make_romp_state_dict(0, center_bias=2.0), smpl_model=smpl)
    frame = np.random.RandomState(3).randint(0, 256, (360, 640, 3)).astype(np.uint8)
    out = model(frame)
    assert out is not None
    model.visualize_items = ['mesh']
    plain = model(frame)
    _check_rotate(out, plain, faces, dev)


@pytest.mark.gpu
def test_bev_rotate_mesh_end_to_end(dev):
    from oracle import bev_oracle as BO
    from oracle import romp_oracle as O
    from romp_amd import bev
    s = bev.bev_settings(['--render_mesh', '--show_items', 'mesh,rotate_mesh', '--rotate_size', '96'])
    s.GPU, s.max_batch = 0, 4
    faces = _faces()
    smpla = dict(O.make_synthetic_smpl(0, 11), f=torch.from_numpy(faces).float())
    smil = dict(O.make_synthetic_smpl(5, 10), f=torch.from_numpy(faces).float())
    model = bev.BEV(s, state_dict=BO.make_bev_state_dict(0), smpla_model=smpla, smil_model=smil)
    frame = np.random.RandomState(2).randint(0, 256, (360, 640, 3)).astype(np.uint8)
    out = None
    for thresh in (0.9995, 0.999, 0.99, 0.9, 0.5, 0.2):
        model.model.centermap_parser.conf_thresh = thresh
        out = model(frame)
        if out is not None:
            break
    assert out is not None
    model.visualize_items = ['mesh']
    plain = model(frame)
    _check_rotate(out, plain, faces, dev)


@pytest.mark.gpu
def test_render_mesh_frames_vs_per_image_panels(dev):
    """B = 3 frames with 2, 0 and 1 persons in one call = the 'mesh' panel of three rendering_romp_bev_results calls."""
    from romp_amd.renderer import Sim3DR
    from romp_amd.vis import render_mesh_frames, rendering_romp_bev_results
    verts, tri, _, _ = _batch_scene(3, seed=12)
    rs = np.random.RandomState(4)
    frames = rs.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    cam_trans = torch.tensor([[0.4, 0., 3.0], [-0.6, 0.1, 5.0], [0.1, 0., 4.0]])   # frame 0: the left person is the farther one
    batch_ids = torch.tensor([0, 0, 2])
    vd, faces = torch.from_numpy(verts).to(dev), torch.from_numpy(tri.astype(np.int64)).to(dev)
    renderer = Sim3DR()
    for mode, extra in (('identity', {}), ('part', {'part_labels': np.arange(verts.shape[1]) % 24})):
        got = render_mesh_frames(renderer, vd, cam_trans.to(dev), batch_ids.to(dev), frames, tri, mesh_color=mode, **extra)
        assert got.shape == frames.shape and got.dtype == np.uint8
        for b in range(3):
            idx = torch.nonzero(batch_ids == b).reshape(-1)
            outputs = {'smpl_face': faces, 'cam_trans': cam_trans[idx].to(dev), 'verts_camed_org': vd[idx.to(dev)], 'verts': vd[idx.to(dev)]}
            cfgs = dict({'mesh_color': mode, 'items': ['mesh'], 'renderer': 'sim3dr'}, **extra)
            panel = rendering_romp_bev_results(renderer, outputs, frames[b].copy(), cfgs)['rendered_image'][:, W:]
            assert np.array_equal(got[b], panel), (mode, b)
            assert bool(len(idx)) == bool((got[b] != frames[b]).any())
