"""GPU tests of romp_parse ALONE (romp_amd/csrc/parse.hip: parse_nms_topk_kernel + parse_pack_kernel), the counterpart of the 3-D parse
block of tests/test_gpu_bev_kernels.py: called through ctypes directly, every one of the eight row outputs over-allocated and
pre-filled (integers -7, floats NaN), and after every call the rows beyond the returned count must still hold the fill.  Expected
values: O.parse_centermap / O.parsing_outputs, which tests/test_parse_nonfinite.py pins to the reference's own steps for the
non-finite maps used here.

Bit for bit: batch ids, flat indices, scores (a -0.0 is not a +0.0 here), centre predictions, betas and every column of params_pred
but the first.  Column 0 (1.1 ** x, also cam[:, 0]) keeps the project's rtol 2e-6 / atol 1e-6 for a powf.  The 22 rotations of a row
are judged as tests/test_gpu_body_kernels.py judges romp_rot6d_to_aa: the angle of R(aa_device)^T R_true in float64, R_true the
float64 Gram-Schmidt of the sampled 6-D code, under K.C_ORDER * d32 + K.FLOOR_ULPS * K.EPS32 with d32 the same angle for the float32
oracle -- for EVERY rotation: the parameter maps draw their codes from a table of pairs with Gram-Schmidt condition
kappa <= K.ROT6D_KAPPA_MAX (asserted, with K.rot6d_bound(kappa) < 1e-3 as tests/test_body_kernel_refs.py asserts it), so no share of
them is excused.  The two hand joints are exact zeros."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import body_kernels_ref as K
from oracle import romp_oracle as O
import test_parse_nonfinite as NF

pytestmark = pytest.mark.gpu

F = np.float32
MAP, NPIX, NCH = 64, 4096, 145
PAD = 3                                  # rows allocated beyond B * max_person
OUTPUTS = (('batch_ids', 1, torch.int32), ('flat_inds', 1, torch.int32), ('scores', 1, torch.float32), ('params_pred', NCH, torch.float32),
           ('cam', 3, torch.float32), ('thetas', 72, torch.float32), ('betas', 10, torch.float32), ('center_preds', 2, torch.int32))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def rot_table():
    """6-D codes of well-conditioned rotations: the seeded normal pairs of K.rot6d_inputs with kappa <= K.ROT6D_KAPPA_MAX."""
    x = K.rot6d_inputs(48)
    kappa = K.rot6d_to_rotmat64(x)[1]
    x = x[kappa <= K.ROT6D_KAPPA_MAX]
    assert len(x) >= 40 and K.rot6d_bound(K.rot6d_to_rotmat64(x)[1]).max() < 1e-3
    return x


def params_map(B):
    """(B,64,64,145) float32 NHWC from a cheap pattern: every row names its image and its pixel.  Channel 0 (the exponent of 1.1):
    multiples of 1/32 in [-1.5, 1.5]; 1, 2: the image and the pixel; 3..134: 22 table rows picked by (pixel, image, joint);
    135..144: (pixel + 4096 * image) / 1024 + k."""
    flat = np.arange(NPIX, dtype=np.int64)[None, :]
    b = np.arange(B, dtype=np.int64)[:, None]
    pm = np.empty((B, NPIX, NCH), F)
    pm[:, :, 0] = ((flat + 5 * b) % 97 - 48) / 32.0
    pm[:, :, 1] = b * 0.25 - 8.0 + 0 * flat
    pm[:, :, 2] = flat / 4096.0 - 0.5 + 0 * b
    table = rot_table()
    pick = (flat[:, :, None] * 7 + b[:, :, None] * 3 + np.arange(22)[None, None, :] * 5) % len(table)
    pm[:, :, 3:135] = table[pick].reshape(B, NPIX, 132)
    pm[:, :, 135:] = ((flat + NPIX * b) / 1024.0)[:, :, None] + np.arange(10)[None, None, :]
    return pm.reshape(B, MAP, MAP, NCH)


@functools.lru_cache(maxsize=2)
def params_on_device(B):
    pm = params_map(B)
    return pm, torch.from_numpy(pm).cuda()


def lattice(step=3):
    """Sites whose 5x5 windows do not hold each other (a window reaches 2, the sites are 3 apart): 22 x 22 = 484 of them."""
    return [(y, x) for y in range(0, MAP, step) for x in range(0, MAP, step)]


# ------------------------------------------------------------------------------------------------ harness
def run_parse(dev, cm, thresh, max_person):
    """romp_parse on centre maps cm (B,1,64,64) numpy and params_map(B) -> (rc, dict of the N returned rows as numpy, or None when
    the call was refused).  Asserts that nothing beyond row N was written in any of the eight outputs (nothing at all on refusal)."""
    from romp_amd import lib as L
    lib = L.load()
    cm = np.ascontiguousarray(cm, F)
    B = cm.shape[0]
    cmd = torch.from_numpy(cm.reshape(B, MAP, MAP)).to(dev)
    pmd = params_on_device(B)[1]
    k = min(max(max_person, 1), 1024)
    cap = B * k + PAD
    bufs = {name: torch.full((cap, w), -7 if dt == torch.int32 else float('nan'), dtype=dt, device=dev) for name, w, dt in OUTPUTS}
    ws = torch.zeros(B * (2 * k + 2) + 2, dtype=torch.int32, device=dev)
    n = C.c_int32(-1)
    rc = lib.romp_parse(L.ptr(cmd), L.ptr(pmd), B, float(thresh), int(max_person), C.byref(n), *[L.ptr(bufs[name]) for name, _, _ in OUTPUTS],
                        L.ptr(ws), L.stream_ptr(dev))
    torch.cuda.synchronize()
    N = n.value if rc == 0 else 0
    assert 0 <= N <= B * k
    out = {}
    for name, w, dt in OUTPUTS:
        host = bufs[name].cpu().numpy()
        tail = host[N:]
        assert (tail == -7).all() if dt == torch.int32 else np.isnan(tail).all(), 'rows beyond the count were written in ' + name
        out[name] = host[:N, 0] if w == 1 else host[:N]
    return rc, (out if rc == 0 else None)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check_rows(got, cm, thresh, max_person):
    """The returned rows against O.parse_centermap and O.parsing_outputs on the same maps.  -> the oracle's (bids, flat, scores)."""
    B = cm.shape[0]
    want = O.parse_centermap(cm, thresh, max_person)
    N = len(want[0])
    assert len(got['batch_ids']) == N, 'the device returned %d rows, the oracle %d' % (len(got['batch_ids']), N)
    assert np.array_equal(got['batch_ids'], want[0]), 'batch ids differ'
    assert np.array_equal(got['flat_inds'], want[1]), 'flat indices differ'
    assert np.array_equal(bits(got['scores']), bits(want[2])), 'scores differ'
    pm = params_on_device(B)[0]
    ref = O.parsing_outputs(cm, pm.transpose(0, 3, 1, 2), thresh, max_person)
    if N == 0:
        assert ref is None
        return want
    assert np.array_equal(ref['batch_ids'], want[0]) and np.array_equal(ref['flat_inds'], want[1])
    assert np.array_equal(got['center_preds'], ref['center_preds'])
    assert np.array_equal(bits(got['betas']), bits(ref['smpl_betas']))
    assert np.array_equal(bits(got['params_pred'][:, 1:]), bits(ref['params_pred'][:, 1:]))
    assert np.array_equal(bits(got['params_pred'][:, 1:]), bits(pm.reshape(B, NPIX, NCH)[want[0], want[1], 1:]))     # the pattern names the row
    assert np.array_equal(bits(got['cam']), bits(got['params_pred'][:, :3]))
    np.testing.assert_allclose(got['params_pred'][:, 0], ref['params_pred'][:, 0], rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(got['cam'], ref['cam'], rtol=2e-6, atol=1e-6)
    th = got['thetas']
    assert np.array_equal(bits(th[:, 66:]), np.zeros((N, 6), np.uint32)), 'the hand joints are not +0.0'
    assert np.isfinite(th).all()
    x6 = ref['params_pred'][:, 3:135].reshape(-1, 6)
    Rt, kappa = K.rot6d_to_rotmat64(x6)
    assert (kappa <= K.ROT6D_KAPPA_MAX).all()
    d32 = K.rotation_angle(K.rodrigues64(ref['smpl_thetas'][:, :66].reshape(-1, 3)), Rt)
    err = K.rotation_angle(K.rodrigues64(th[:, :66].reshape(-1, 3)), Rt)
    bound = K.C_ORDER * d32 + K.FLOOR_ULPS * K.EPS32
    print('BOUND romp_parse thetas, %d rotations: largest err/bound %.4f (largest angle err %.3e)' % (len(err), (err / bound).max(), err.max()))
    assert (err <= bound).all()
    return want


# ------------------------------------------------------------------------------------------------ cases
def test_parse_batch_of_70(dev):
    """B = 70: parse_pack_kernel's row offset is a prefix sum over the images before it in steps of 64 lanes.  A different count per
    image; images 0, 1, 35, 63, 64 and 69 empty; image 65 exactly full (64), image 2 beyond max_person (70).  Isolated peaks with
    distinct scores on the stride-3 lattice."""
    B = 70
    rs = np.random.RandomState(70)
    sites = lattice()
    assert len(sites) == 484
    counts = [(b * 7) % 23 + 1 for b in range(B)]
    for b in (0, 1, 35, 63, 64, 69):
        counts[b] = 0
    counts[65], counts[2] = 64, 70
    cm = np.zeros((B, 1, MAP, MAP), F)
    for b in range(B):
        for j, i in enumerate(rs.permutation(len(sites))[:counts[b]]):
            cm[(b, 0) + sites[i]] = 0.3 + 0.009 * j + 0.0001 * b
    rc, got = run_parse(dev, cm, 0.25, 64)
    assert rc == 0
    want = check_rows(got, cm, 0.25, 64)
    assert np.bincount(want[0], minlength=B).tolist() == [min(c, 64) for c in counts]
    assert np.bincount(got['batch_ids'], minlength=B).tolist() == [min(c, 64) for c in counts]


@pytest.mark.parametrize('max_person,n_peaks', [(1, 3), (64, 70)])
def test_parse_topk_cut_with_equal_scores(dev, max_person, n_peaks):
    """More isolated maxima than max_person in image 0, three EQUAL scores at ranks max_person - 2 .. max_person: lower flat index
    first.  torch.topk leaves the order of equal scores open, so this is judged against the oracle only.  Image 1 has one maximum."""
    rs = np.random.RandomState(max_person)
    sites = lattice()
    pick = [sites[i] for i in rs.permutation(len(sites))[:n_peaks]]
    scores = (0.9 - 0.0005 * np.arange(n_peaks)).astype(F)
    lo = max(max_person - 2, 0)
    scores[lo:lo + 3] = scores[lo]                                   # in random (not flat-index) order of sites
    assert len(set(scores.tolist())) == n_peaks - 2
    cm = torch.rand(2, 1, MAP, MAP, generator=torch.Generator().manual_seed(3)).numpy() * F(0.1) - F(0.05)
    for (y, x), s in zip(pick, scores):
        cm[0, 0, y, x] = s
    cm[1, 0, 7, 9] = 0.75
    rc, got = run_parse(dev, cm, 0.2, max_person)
    assert rc == 0
    want = check_rows(got, cm, 0.2, max_person)
    assert (want[0] == 0).sum() == max_person and (want[0] == 1).sum() == 1
    tied = np.nonzero(want[2] == scores[lo])[0]
    assert 1 <= len(tied) < 3, 'the cut must fall inside the tie'


def test_parse_topk_cut_1024_on_a_plateau(dev):
    """max_person = 1024: a 64x64 map holds 484 isolated maxima at most, so the map is a plateau of 0.5 (every pixel of it that no
    higher peak suppresses is a maximum) with five higher lattice peaks: more than 3000 candidates for the rank loop and the LDS
    counter, the cut deep inside the tie of the plateau, lower flat index first."""
    cm = np.full((1, 1, MAP, MAP), 0.5, F)
    for j, (y, x) in enumerate([(9, 9), (30, 33), (0, 63), (63, 0), (45, 12)]):
        cm[0, 0, y, x] = 0.9 - 0.05 * j
    assert len(O.parse_centermap(cm, 0.2, NPIX)[0]) > 3000
    rc, got = run_parse(dev, cm, 0.2, 1024)
    assert rc == 0
    want = check_rows(got, cm, 0.2, 1024)
    assert len(want[0]) == 1024 and (want[2][5:] == F(0.5)).all() and (want[2][:5] > 0.5).all() and (np.diff(want[1][5:]) > 0).all()


def test_parse_threshold_and_border(dev):
    """A peak equal to the threshold (excluded), one ulp above (kept), one ulp below (excluded); peaks on the 4 corners and on each of
    the 4 edges; the background is partly negative."""
    t = F(0.3)
    cm = torch.rand(2, 1, MAP, MAP, generator=torch.Generator().manual_seed(11)).numpy() * F(0.1) - F(0.05)
    assert (cm < 0).any()
    cm[0, 0, 20, 20], cm[0, 0, 20, 30], cm[0, 0, 20, 40] = t, np.nextafter(t, F(1)), np.nextafter(t, F(0))
    border = [(0, 0), (0, 63), (63, 0), (63, 63), (0, 31), (63, 17), (29, 0), (44, 63)]
    for j, (y, x) in enumerate(border):
        cm[1, 0, y, x] = 0.5 + 0.03 * j
    rc, got = run_parse(dev, cm, float(t), 64)
    assert rc == 0
    want = check_rows(got, cm, float(t), 64)
    assert want[0].tolist() == [0] + [1] * 8 and want[1][0] == 20 * MAP + 30 and want[2][0] == np.nextafter(t, F(1))
    assert sorted(want[1][1:].tolist()) == sorted(y * MAP + x for y, x in border)


def test_parse_negative_threshold_lets_suppressed_pixels_through(dev):
    """thresh < 0 on a small-valued map: a suppressed pixel scores v * 0, which is +0.0 or -0.0 by the sign of v, and passes `> thresh` in
    the reference too.  All 4096 pixels of an image are candidates; the zeros rank below the positive maxima, equal among themselves
    whatever their sign, by flat index; the scores come back with their signs."""
    cm = torch.rand(2, 1, MAP, MAP, generator=torch.Generator().manual_seed(12)).numpy() * F(0.004) - F(0.002)
    rc, got = run_parse(dev, cm, -0.5, 256)
    assert rc == 0
    want = check_rows(got, cm, -0.5, 256)
    zeros = want[2] == 0
    assert len(want[0]) == 512 and (want[2] > 0).sum() > 50 and (zeros & np.signbit(want[2])).sum() > 20 and (zeros & ~np.signbit(want[2])).sum() > 20


def test_parse_rejects_bad_arguments(dev):
    from romp_amd import lib as L
    lib = L.load()
    cm = np.zeros((1, 1, MAP, MAP), F)
    cm[0, 0, 5, 6] = 1.0
    for max_person in (0, 1025):
        rc, got = run_parse(dev, cm, 0.1, max_person)                # (asserts that no output was touched)
        msg = lib.romp_last_error().decode()
        assert rc != 0 and got is None and 'max_person' in msg, (max_person, rc, msg)
    rc, got = run_parse(dev, cm, 0.1, 64)                            # and the next valid call is served
    assert rc == 0
    check_rows(got, cm, 0.1, 64)
    assert got['flat_inds'].tolist() == [5 * MAP + 6] and got['scores'].tolist() == [1.0] and got['center_preds'].tolist() == [[48, 40]]


@pytest.mark.parametrize('name', NF.NAMES)
def test_parse_nonfinite_maps(dev, name):
    """NaN, +inf and -inf pixels (tests/test_parse_nonfinite.py): MaxPool2d hands a NaN on, so a peak within two pixels of one is NOT
    a detection (a maximum formed with fmaxf drops the NaN and keeps the peak); a peak three away is; an image that is NaN all over has
    no rows and the rows of the next image follow those of the one before; +inf peaks come first, by flat index among themselves; -inf
    changes nothing around it."""
    cm, kept = NF.case_2d(name)
    rc, got = run_parse(dev, cm, NF.THRESH, NF.MAX_PERSON)
    assert rc == 0
    print('%s: %d rows %s, expected %s' % (name, len(got['batch_ids']), sorted(zip(got['batch_ids'].tolist(), got['flat_inds'].tolist())), kept))
    want = check_rows(got, cm, NF.THRESH, NF.MAX_PERSON)
    assert sorted(zip(want[0].tolist(), want[1].tolist())) == kept
