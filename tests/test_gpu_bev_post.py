"""bev_post_kernel and preprocess_kernel (csrc/post.hip) alone on the GPU (run with -m gpu), through the C entries
romp_bev_postprocess, romp_preprocess and romp_preprocess_batch.

Post-processing.  Scenes: the reference-made edge scenes of tests/golden/bev_post_edges.npz and the generated scenes of
tests/test_bev_post.py; tests/test_bev_post.py::test_bev_post_scene_conditions shows on the CPU that in every one of them no
compared value lies within 1e-3 of a threshold, so keep must equal the float64 restatement's set exactly (and the
reference's kept_final for the edge scenes).  Every float output is pre-filled with NaN and keep with -1, with 5 guard rows
past N: every row of a non-empty image must come back written, the guard rows untouched.

Tolerance for pj2d, pj2d_org and cam_trans: the rule of tests/test_gpu_fit.py.  error = max |delta| / max |float64
restatement| per tensor, and  err_HIP <= 8 * max(err_float32_restatement, 4 * 2^-24).  Every figure is printed before it is
asserted (pytest -s).

Pre-processing: bit-exact against oracle.cv_resize_oracle.img_preprocess at frame sizes where every cubic tap lands on the
replicated border, the centred pad is uneven or one pixel wide, or the frame is a strip, and at output sizes whose last
workgroup is partial."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import bev_post_oracle as PO
from test_bev_post import COUNTS, NMS, REL, chain_in_crowd, edge_scenes, find_scene
from test_cpu_host import PREPROCESS_FRAMES, PREPROCESS_SIZES

pytestmark = pytest.mark.gpu
FLOOR = 4 * 2.0 ** -24
GUARD = 5
FLOATS = ('pj2d', 'pj2d_org', 'cam_trans')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def run_post(dev, images, nms=NMS, rel=REL):
    """One romp_bev_postprocess call over `images`: a list of (joints, cam, pad) or None for an image with nobody (its pad
    row is NaN: nothing may depend on it).  Checks the sentinels, -> one dict(pj2d, pj2d_org, cam_trans, keep) of numpy
    arrays per image."""
    from romp_amd import lib as L
    lib = L.load()
    counts = [0 if im is None else len(im[1]) for im in images]
    N, B = sum(counts), len(images)
    assert N > 0
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    joints = torch.from_numpy(np.concatenate([im[0] for im in images if im is not None]).astype(np.float32)).to(dev)
    cam = torch.from_numpy(np.concatenate([im[1] for im in images if im is not None]).astype(np.float32)).to(dev)
    pads = torch.from_numpy(np.stack([np.full(6, np.nan, np.float32) if im is None else np.asarray(im[2], np.float32)
                                      for im in images])).to(dev)
    offsets = torch.from_numpy(offs).to(dev)
    nan = lambda *s: torch.full(s, float('nan'), device=dev, dtype=torch.float32)
    out = {'pj2d': nan(N + GUARD, 71, 2), 'pj2d_org': nan(N + GUARD, 71, 2), 'cam_trans': nan(N + GUARD, 3)}
    keep = torch.full((N + GUARD,), -1, dtype=torch.int32, device=dev)
    L.check(lib.romp_bev_postprocess(L.ptr(joints), L.ptr(cam), L.ptr(offsets), B, L.ptr(pads), nms, rel, L.ptr(out['pj2d']),
                                     L.ptr(out['pj2d_org']), L.ptr(out['cam_trans']), L.ptr(keep), L.stream_ptr(dev)))
    torch.cuda.current_stream(dev).synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got['keep'] = keep.cpu().numpy()
    for k in FLOATS:
        assert np.isfinite(got[k][:N]).all(), '%s: a row of a non-empty image was not written' % k
        assert np.isnan(got[k][N:]).all(), '%s: a guard row was written' % k
    assert np.isin(got['keep'][:N], (0, 1)).all() and (got['keep'][N:] == -1).all(), got['keep']
    return [{k: v[offs[b]:offs[b + 1]] for k, v in got.items()} for b in range(B)]


def accurate(tag, got, joints, cam, pad, rows=slice(None)):
    """The rule of the module docstring for the three float outputs of one image; prints the figures."""
    r64, r32 = PO.project(joints, cam, pad, np.float64), PO.project(joints, cam, pad)
    ok = True
    for name, a64, a32 in zip(FLOATS, r64, r32):
        ref = a64[rows]
        scale = np.abs(ref).max()
        e_hip, e_f32 = float(np.abs(got[name] - ref).max() / scale), float(np.abs(a32[rows] - ref).max() / scale)
        print(f'{tag} {name}: max|ref| {scale:.3g} err_hip {e_hip:.3e} err_cpu_f32 {e_f32:.3e} bound {8 * max(e_f32, FLOOR):.3e}')
        ok = ok and got[name].dtype == np.float32 and got[name].shape == ref.shape and e_hip <= 8 * max(e_f32, FLOOR)
    return ok


def check_scene(tag, got, joints, cam, pad, kept_final=None):
    r64 = PO.postprocess(joints, cam, pad, NMS, REL, dtype=np.float64)
    ok = accurate(tag, got, joints, cam, pad)
    kept = np.nonzero(got['keep'])[0].tolist()
    print(f'{tag} kept {kept if len(kept) <= 8 else len(kept)} stages {r64["stages"]} margin {r64["margin"]:.3g}')
    assert kept == np.nonzero(r64['keep'])[0].tolist()
    assert kept_final is None or kept == kept_final.tolist()
    assert ok


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in FLOATS + ('keep',))


@pytest.fixture(scope='module')
def scenes(golden_dir):
    return edge_scenes(golden_dir)


@pytest.fixture(scope='module')
def alone(dev, scenes):
    """Every edge scene as a B = 1 call."""
    return {name: run_post(dev, [(s['joints'], s['cam'], s['pad'])])[0] for name, s in scenes.items()}


# ------------------------------------------------------------------------------------------------ post-processing
def test_edge_scenes_alone(scenes, alone):
    assert len(scenes) == 13
    for name, s in scenes.items():
        check_scene(name, alone[name], s['joints'], s['cam'], s['pad'], s['kept_final'])


def test_edge_scenes_as_one_batch(dev, scenes, alone):
    """All scenes in one call, each with its own pad-info row; an image with nobody first, one between two scenes and one
    last.  Bit for bit what each scene gave alone: the pad-info row stride, nothing left in shared memory by the image
    before, the early return."""
    names = list(scenes)
    images = [None] + [(scenes[n]['joints'], scenes[n]['cam'], scenes[n]['pad']) for n in names] + [None]
    images.insert(6, None)
    order = [None] + names + [None]
    order.insert(6, None)
    got = run_post(dev, images)
    assert len(got) == len(names) + 3 and len({tuple(scenes[n]['pad']) for n in names}) >= 4
    for name, g in zip(order, got):
        if name is None:
            assert len(g['keep']) == 0
        else:
            assert same_bits(g, alone[name]), name


@pytest.mark.parametrize('n', COUNTS)
def test_person_counts(dev, n):
    found = find_scene(n)
    assert found is not None
    seed, (joints, cam, pad), r64 = found[:3]
    got = run_post(dev, [(joints, cam, pad)])[0]
    check_scene(f'n={n} seed {seed}', got, joints, cam, pad)
    if n == 64:
        assert r64['stages']['suppressed'] > 0 and r64['stages']['outliers'] > 0


def test_a_removed_row_still_removes_others(dev, golden_dir):
    """chain_in_crowd of tests/test_bev_post.py: B is marked in an earlier round of the wave that later looks at B-C."""
    seed, (joints, cam, pad) = chain_in_crowd(golden_dir)
    got = run_post(dev, [(joints, cam, pad)])[0]
    check_scene(f'chain in 64, seed {seed}', got, joints, cam, pad)
    assert got['keep'][[0, 4, 5]].tolist() == [1, 0, 0]


def test_more_than_64_persons(dev, scenes, alone):
    """An image of 65 rows, then one of 3.  The first 64 rows are processed as an image of those 64; row 64 is not kept, and
    its translation and projections, which are per-row quantities, are written all the same; the next image is untouched."""
    joints, cam, pad = find_scene(65)[1]
    s = scenes['outlier3']
    first64 = run_post(dev, [(joints[:64], cam[:64], pad)])[0]
    check_scene('first 64 of 65', first64, joints[:64], cam[:64], pad)
    got = run_post(dev, [(joints, cam, pad), (s['joints'], s['cam'], s['pad'])])
    assert same_bits({k: v[:64] for k, v in got[0].items()}, first64)
    assert got[0]['keep'][64] == 0
    assert accurate('row 64 of 65', {k: got[0][k][64:] for k in FLOATS}, joints, cam, pad, rows=slice(64, 65))
    assert same_bits(got[1], alone['outlier3'])


def test_two_calls_give_equal_bits(dev, scenes, alone):
    joints, cam, pad = find_scene(64)[1]
    images = [(joints, cam, pad), None, (scenes['chain']['joints'], scenes['chain']['cam'], scenes['chain']['pad'])]
    a, b = run_post(dev, images), run_post(dev, images)
    assert all(same_bits(x, y) for x, y in zip(a, b)) and same_bits(a[2], alone['chain'])


def test_a_side_stream_gives_the_default_streams_bits(dev, scenes):
    joints, cam, pad = find_scene(63)[1]
    images = [(joints, cam, pad), (scenes['survivors_only']['joints'], scenes['survivors_only']['cam'], scenes['survivors_only']['pad'])]
    want = run_post(dev, images)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        got = run_post(dev, images)
    s.synchronize()
    assert all(same_bits(x, y) for x, y in zip(want, got))


def test_bad_arguments(dev, scenes):
    """B = 0 and every null pointer: the error code, the entry's name in romp_last_error(), and nothing launched."""
    from romp_amd import lib as L
    lib = L.load()
    s = scenes['outlier3']
    joints, cam = torch.from_numpy(s['joints']).to(dev), torch.from_numpy(s['cam']).to(dev)
    offsets = torch.tensor([0, 3], dtype=torch.int32, device=dev)
    pads = torch.from_numpy(s['pad'][None]).to(dev)
    nan = lambda *sh: torch.full(sh, float('nan'), device=dev, dtype=torch.float32)
    pj, pjo, tr = nan(3, 71, 2), nan(3, 71, 2), nan(3, 3)
    keep = torch.full((3,), -1, dtype=torch.int32, device=dev)
    good = [joints, cam, offsets, pads, pj, pjo, tr, keep]

    def call(t, B):
        return lib.romp_bev_postprocess(L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), B, L.ptr(t[3]), NMS, REL, L.ptr(t[4]), L.ptr(t[5]),
                                        L.ptr(t[6]), L.ptr(t[7]), L.stream_ptr(dev))

    bad = [(good, 0), (good, -1)] + [(good[:i] + [None] + good[i + 1:], 1) for i in range(len(good))]
    for t, B in bad:
        assert call(t, B) == -1 and b'romp_bev_postprocess' in lib.romp_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(pj).all() and torch.isnan(pjo).all() and torch.isnan(tr).all() and (keep == -1).all())
    assert call(good, 1) == 0                                        # the same buffers are fine once everything is there
    torch.cuda.synchronize()
    assert keep.tolist() == [1, 1, 0]


# ------------------------------------------------------------------------------------------------ pre-processing
@pytest.mark.parametrize('out_size', PREPROCESS_SIZES)
@pytest.mark.parametrize('shape', PREPROCESS_FRAMES)
def test_preprocess_geometry(dev, shape, out_size):
    from oracle import cv_resize_oracle as CV
    from romp_amd import lib as L
    lib = L.load()
    H, W = shape
    S, guard = out_size, 64
    frames = np.random.RandomState(H * 1000 + W).randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    refs = [CV.img_preprocess(f, S) for f in frames]
    fd = torch.from_numpy(frames).to(dev)
    for B in (1, 3):
        out = torch.full((B * S * S * 3 + guard,), float('nan'), device=dev, dtype=torch.float32)
        pad = (C.c_float * 6)(*([-1.] * 6))
        if B == 1:
            L.check(lib.romp_preprocess(L.ptr(fd), H, W, L.ptr(out), S, pad, L.stream_ptr(dev)))
        else:
            L.check(lib.romp_preprocess_batch(L.ptr(fd), B, H, W, L.ptr(out), S, pad, L.stream_ptr(dev)))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isnan(got[B * S * S * 3:]).all(), 'an element past the output was written'
        got = got[:B * S * S * 3].reshape(B, S, S, 3)
        assert np.isfinite(got).all(), 'an output element was not written'
        for b in range(B):
            assert np.array_equal(got[b], refs[b][0][0]), (shape, out_size, B, b)
        assert list(pad) == refs[0][1].tolist()
