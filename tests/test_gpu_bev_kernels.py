"""GPU tests of the BEV head's own kernels (romp_amd/csrc/bev.hip), each ALONE against a plain high-precision restatement of its
operation (oracle/bev_kernels_ref.py) and the reference-made edge fixture tests/golden/bev_edges.npz: the 3x3x3 conv (impulse
response bit-exact, random data inside a derived float32 bound, the refiner pair as the plan lowers it), the map builder and the
Conv1d packer (bit-exact, strided inputs with poisoned padding), the 3-D parse at the volume's borders / the top-K cut / B > 64 /
the candidate capacity / NaN and infinite voxels (the cases of tests/test_parse_nonfinite.py), and the per-person regression on crafted camera triples.  The tests drive the existing C ABI only: one-
or two-op programs through romp_net_create, and romp_bev_parse / romp_bev_regress directly.  They are written against the
operations, not against today's kernel boundaries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import bev_kernels_ref as K
from oracle import bev_oracle as BO
import test_parse_nonfinite as NF

pytestmark = pytest.mark.gpu

MAP, DEPTH, VOX = 128, 64, 64 * 128 * 128
BEV_CAP = 32768                      # candidate capacity per image of the 3-D parse (csrc/bev.hip)
ROMP_ECAPACITY = -4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def _host_floats(keep, values):
    arr = (C.c_float * len(values))(*[float(v) for v in values])
    keep.append(arr)
    return C.cast(arr, C.c_void_p).value


class _Net:
    """A tiny program on the network executor: the BEV ops are reachable through it only."""

    def __init__(self, dev, ops, sizes, B):
        from romp_amd import lib as L
        self.L, self.lib, self.dev, self.B, self.sizes = L, L.load(), dev, B, sizes
        self.h = C.c_void_p()
        arr = (L.RompOp * len(ops))(*ops)
        L.check(self.lib.romp_net_create(C.byref(self.h), arr, len(ops), (C.c_int64 * len(sizes))(*sizes), len(sizes), B))
        self.dummy = torch.zeros(64, device=dev)

    def write(self, buf, t):
        td = t.contiguous().to(self.dev)
        assert td.numel() == self.B * self.sizes[buf]
        self.L.check(self.lib.romp_net_write_buffer(self.h, buf, self.L.ptr(td), td.numel(), self.L.stream_ptr(self.dev)))
        torch.cuda.synchronize()

    def forward(self, center=None, params=None):
        L = self.L
        L.check(self.lib.romp_net_forward(self.h, L.ptr(self.dummy), self.B, L.ptr(center if center is not None else self.dummy),
                                          L.ptr(params if params is not None else self.dummy), L.stream_ptr(self.dev)))
        torch.cuda.synchronize()

    def read(self, buf):
        out = torch.empty(self.B * self.sizes[buf], device=self.dev)
        self.L.check(self.lib.romp_net_read_buffer(self.h, buf, self.B, self.L.ptr(out), out.numel(), self.L.stream_ptr(self.dev)))
        torch.cuda.synchronize()
        return out.cpu()

    def close(self):
        self.lib.romp_net_destroy(self.h)


def _conv3d_op(keep, C_, w, scale, shift, relu, in_buf, res_buf, out_buf):
    from romp_amd.lib import RompOp, OP_CONV3D
    o = RompOp()
    o.kind, o.in_buf, o.res_buf, o.out_buf = OP_CONV3D, in_buf, res_buf, out_buf
    o.Cin = o.Cout = C_
    o.relu = int(relu)
    o.weight = _host_floats(keep, np.asarray(w, np.float32).reshape(-1).tolist())
    o.scale, o.shift = _host_floats(keep, np.asarray(scale, np.float32).tolist()), _host_floats(keep, np.asarray(shift, np.float32).tolist())
    return o


def _run_conv3d(dev, x, w, scale, shift, relu, res, where):
    """One conv3d op.  x / res (B,C,64,128,128) float32 tensors; where: 'arena' | 'special' (BUF_CENTER for C = 1, BUF_PARAMS for C = 3).
    -> output (B,C,64,128,128) numpy; asserts that the input and residual buffers are unchanged afterwards."""
    from romp_amd.lib import BUF_NONE, BUF_CENTER, BUF_PARAMS
    B, C_ = x.shape[:2]
    keep = []
    out_buf = 2 if where == 'arena' else (BUF_CENTER if C_ == 1 else BUF_PARAMS)
    op = _conv3d_op(keep, C_, w, scale, shift, relu, 0, 1 if res is not None else BUF_NONE, out_buf)
    net = _Net(dev, [op], [C_ * VOX] * 3, B)
    try:
        net.write(0, x)
        net.write(2, torch.full((B * C_ * VOX,), float('nan')))
        if res is not None:
            net.write(1, res)
        special = torch.full((B, C_, DEPTH, MAP, MAP), float('nan'), device=dev)
        net.forward(center=special if C_ == 1 else None, params=special if C_ == 3 else None)
        out = (net.read(2) if where == 'arena' else special.cpu()).reshape(B, C_, DEPTH, MAP, MAP).numpy()
        assert np.array_equal(net.read(0).numpy(), x.reshape(-1).numpy()), 'conv3d changed its input'
        if res is not None:
            assert np.array_equal(net.read(1).numpy(), res.reshape(-1).numpy()), 'conv3d changed its residual'
        if where != 'arena':
            assert torch.isnan(net.read(2)).all(), 'conv3d wrote an arena buffer it was not given'
    finally:
        net.close()
    return out


# ------------------------------------------------------------------------------------------------ conv3d
@pytest.mark.parametrize('C_,B,relu,use_res,where', [
    (1, 1, 0, False, 'arena'), (1, 2, 1, True, 'special'), (1, 3, 0, True, 'arena'),
    (3, 1, 1, False, 'special'), (3, 2, 0, True, 'arena'), (3, 3, 1, True, 'special')])
def test_conv3d_impulse_exact(dev, C_, B, relu, use_res, where):
    """Single 1.0 voxels at the 8 corners, the 6 mid-faces and both sides of every brick seam (d 15|16 31|32 47|48, h 7|8 119|120,
    w 3|4 123|124), 27 C^2 distinct weights of both signs, scale 1, shift 0: every output voxel is one weight or zero, so the
    expected volume is a scatter of the flipped kernel cropped at the borders (plus the residual: one float32 addition; then the
    ReLU) -- compared bit for bit, one input channel at a time."""
    sets = K.impulse_sites(B, seed=10 * C_ + B)
    w = K.distinct_weights(C_, seed=C_ + B)
    rs = np.random.RandomState(B)
    res = torch.from_numpy(rs.randn(B, C_, DEPTH, MAP, MAP).astype(np.float32)) if use_res else None
    for ci in range(C_):
        x = K.impulse_volume(sets, C_, ci)
        exp = K.impulse_expected(sets, w, ci)
        if B >= 2:          # image 0's last plane and image 1's first are adjacent in memory: only the zero padding separates them
            assert x[0, ci, 63].any() and x[1, ci, 0].any()
        if res is not None:
            exp = exp + res.numpy()
        if relu:
            exp = np.maximum(exp, np.float32(0))
        assert exp.dtype == np.float32
        out = _run_conv3d(dev, torch.from_numpy(x), w, np.ones(C_), np.zeros(C_), relu, res, where)
        bad = np.argwhere(~((out == exp) | (np.isnan(out) & np.isnan(exp))))
        assert bad.size == 0, f'C={C_} ci={ci}: {len(bad)} voxels differ, first (b,co,d,h,w) {bad[:5].tolist()}'
        assert np.array_equal(out, exp)


def test_conv3d_batch_planes_do_not_leak(dev):
    """B = 2, C = 1: one impulse in image 0's d = 63 plane leaves image 1's d = 0 plane zero, and the reverse."""
    w = K.distinct_weights(1, seed=5, signed=False)
    for src, site, other, plane in ((0, (63, 40, 50), 1, 0), (1, (0, 90, 17), 0, 63)):
        sets = [[], []]
        sets[src] = [site]
        out = _run_conv3d(dev, torch.from_numpy(K.impulse_volume(sets, 1, 0)), w, np.ones(1), np.zeros(1), 0, None, 'arena')
        assert not out[other].any(), f'image {other} is not zero'
        assert not out[other, 0, plane].any()
        assert np.array_equal(out, K.impulse_expected(sets, w, 0))
        assert np.count_nonzero(out[src]) == 18


def _mixed(gen, shape):
    """Mixed sign, magnitudes from 1e-3 to 1e3 (an absolute gate would not do)."""
    return torch.randn(shape, generator=gen) * 10.0 ** (torch.rand(shape, generator=gen) * 6 - 3)


@pytest.mark.parametrize('C_,B,relu,use_res,where', [
    (1, 3, 0, False, 'special'), (1, 1, 1, False, 'arena'), (1, 2, 0, True, 'arena'), (1, 1, 1, True, 'special'),
    (3, 1, 0, False, 'arena'), (3, 2, 1, False, 'special'), (3, 1, 0, True, 'special'), (3, 3, 1, True, 'arena')])
def test_conv3d_random_within_float32_bound(dev, C_, B, relu, use_res, where):
    """Random data of mixed sign and magnitude against F.conv3d in float64 (then scale, shift, residual, ReLU in float64).  The
    tolerance is derived, not measured: per voxel (27 C + 3) 2^-24 (|scale| (|x| conv |w|) + |shift| + |res|)."""
    g = torch.Generator().manual_seed(100 * C_ + 10 * B + relu)
    x = _mixed(g, (B, C_, DEPTH, MAP, MAP))
    w = torch.randn(C_, C_, 3, 3, 3, generator=g)
    scale = (torch.rand(C_, generator=g) + 0.5) * torch.tensor([1.0, -1.0, 1.0])[:C_]
    shift = torch.randn(C_, generator=g) * 10
    res = _mixed(g, (B, C_, DEPTH, MAP, MAP)) if use_res else None
    ref, bound = K.conv3d_ref(x, w, scale, shift, res, bool(relu))
    out = _run_conv3d(dev, x, w.numpy(), scale.numpy(), shift.numpy(), relu, res, where)
    assert np.isfinite(out).all()
    err = (torch.from_numpy(out).double() - ref).abs()
    ratio = (err / bound).max().item()
    print(f'BOUND conv3d C={C_} B={B} relu={relu} res={use_res} {where}: largest err/bound {ratio:.4f} (max-abs err {err.max():.3e}, |ref| max {ref.abs().max():.3e})')
    assert ratio <= 1.0


@pytest.mark.parametrize('C_,B', [(1, 2), (3, 1)])
def test_refiner_as_lowered(dev, C_, B):
    """BasicBlock_3D as the plan lowers it: conv1 + BN + ReLU into an arena buffer, conv2 + BN + residual (the block's input) into
    BUF_CENTER (C = 1) / BUF_PARAMS (C = 3), against float64.  Tolerance: the stage-2 bound plus sum|w2| |scale2| times the largest
    stage-1 bound (oracle/bev_kernels_ref.refiner_ref)."""
    from romp_amd.lib import BUF_NONE, BUF_CENTER, BUF_PARAMS
    g = torch.Generator().manual_seed(40 + C_)
    x = torch.randn(B, C_, DEPTH, MAP, MAP, generator=g) * 2
    w1 = (torch.rand(C_, C_, 3, 3, 3, generator=g) * 2 - 1) / (27 * C_) ** 0.5
    w2 = (torch.rand(C_, C_, 3, 3, 3, generator=g) * 2 - 1) / (27 * C_) ** 0.5
    s1, b1 = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g) * 0.1
    s2, b2 = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g) * 0.1
    ref, bound = K.refiner_ref(x, w1, s1, b1, w2, s2, b2)
    keep = []
    ops = [_conv3d_op(keep, C_, w1.numpy(), s1.numpy(), b1.numpy(), 1, 0, BUF_NONE, 1),
           _conv3d_op(keep, C_, w2.numpy(), s2.numpy(), b2.numpy(), 0, 1, 0, BUF_CENTER if C_ == 1 else BUF_PARAMS)]
    net = _Net(dev, ops, [C_ * VOX] * 2, B)
    try:
        net.write(0, x)
        out = torch.full((B, C_, DEPTH, MAP, MAP), float('nan'), device=dev)
        net.forward(center=out if C_ == 1 else None, params=out if C_ == 3 else None)
        assert np.array_equal(net.read(0).numpy(), x.reshape(-1).numpy()), 'the refiner changed its input'
    finally:
        net.close()
    err = (out.cpu().double() - ref).abs()
    ratio = (err / bound).max().item()
    print(f'BOUND refiner C={C_} B={B}: largest err/bound {ratio:.4f} (max-abs err {err.max():.3e})')
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ maps / pack
@pytest.mark.parametrize('B', [1, 3])
def test_bev_maps_exact(dev, B):
    """center_map_3d and cam_maps_3d, bit for bit, against the float32 restatement in the reference's order of operations
    ((coord + off_fv) + off_bv on channel 2).  The inputs have channel strides wider than the lanes read (8 > 4, 160 > 128) with
    NaN in the rest: any NaN in an output is a read from a lane the kernel must not touch."""
    from romp_amd.lib import RompOp, OP_BEV_MAPS
    g = torch.Generator().manual_seed(20 + B)
    fv_cs, bv_cs = 8, 160
    fv = torch.full((B, MAP, MAP, fv_cs), float('nan'))
    fv[..., :4] = torch.randn(B, MAP, MAP, 4, generator=g) * torch.tensor([1.0, 0.3, 0.7, 1.9])
    bv = torch.full((B, MAP, bv_cs), float('nan'))                 # [w][0..63 centre | 64..127 offset]
    bv[..., :128] = torch.randn(B, MAP, 128, generator=g) * 10.0 ** (torch.rand(B, MAP, 128, generator=g) * 4 - 3)
    keep = []
    op = RompOp()
    op.kind, op.in_buf, op.res_buf, op.out_buf = OP_BEV_MAPS, 0, 1, 2
    op.in_cstride, op.res_cstride = fv_cs, bv_cs
    op.term_buf[0] = 3
    op.weight = _host_floats(keep, BO.cam3dmap_anchor(60, MAP).astype(np.float32).tolist())
    net = _Net(dev, [op], [MAP * MAP * fv_cs, MAP * bv_cs, VOX, 3 * VOX], B)
    try:
        net.write(0, fv)
        net.write(1, bv)
        net.write(2, torch.full((B * VOX,), float('nan')))
        net.write(3, torch.full((B * 3 * VOX,), float('nan')))
        net.forward()
        c3 = net.read(2).reshape(B, DEPTH, MAP, MAP).numpy()
        cam = net.read(3).reshape(B, 3, DEPTH, MAP, MAP).numpy()
        assert torch.equal(torch.isnan(net.read(0)), torch.isnan(fv.reshape(-1))) and torch.equal(torch.isnan(net.read(1)), torch.isnan(bv.reshape(-1)))
    finally:
        net.close()
    assert not np.isnan(c3).any() and not np.isnan(cam).any(), 'read from an unused lane'
    bvn = bv[..., :128].permute(0, 2, 1).numpy()                     # (B, 128 [centre d | offset d], w)
    c3r, camr = K.bev_maps_ref(fv[..., 0].numpy(), fv[..., 1:4].permute(0, 3, 1, 2).numpy(), bvn[:, :64], bvn[:, 64:])
    assert np.array_equal(c3, c3r)
    for c in range(3):
        assert np.array_equal(cam[:, c], camr[:, c]), f'cam_maps_3d channel {c}: {(cam[:, c] != camr[:, c]).sum()} voxels differ'


@pytest.mark.parametrize('B', [1, 2, 5])
def test_bev_pack_exact(dev, B):
    """summon_feats (model.py:190) is a permutation: exactly torch.cat([maps_fv, feats], 1).reshape(B, -1, 128) with the sequence
    axis first.  Channel strides wider than the channels read (8 > 4, 32 > 16), NaN in the padding.  B = 1 has fewer elements than
    the launch has threads; B >= 2 takes the grid-stride loop."""
    from romp_amd.lib import RompOp, OP_BEV_PACK
    g = torch.Generator().manual_seed(30 + B)
    fv_cs, f_cs = 8, 32
    fv = torch.full((B, MAP, MAP, fv_cs), float('nan'))
    fv[..., :4] = torch.randn(B, MAP, MAP, 4, generator=g)
    ft = torch.full((B, MAP, MAP, f_cs), float('nan'))
    ft[..., :16] = torch.randn(B, MAP, MAP, 16, generator=g)
    op = RompOp()
    op.kind, op.in_buf, op.res_buf, op.out_buf = OP_BEV_PACK, 0, 1, 2
    op.in_cstride, op.res_cstride = fv_cs, f_cs
    net = _Net(dev, [op], [MAP * MAP * fv_cs, MAP * MAP * f_cs, 20 * MAP * MAP], B)
    try:
        net.write(0, fv)
        net.write(1, ft)
        net.write(2, torch.full((B * 20 * MAP * MAP,), float('nan')))
        net.forward()
        out = net.read(2).reshape(B, MAP, 20 * MAP)
    finally:
        net.close()
    ref = K.bev_pack_ref(fv[..., :4].permute(0, 3, 1, 2), ft[..., :16].permute(0, 3, 1, 2))
    assert not torch.isnan(out).any(), 'read from the padding'
    assert np.array_equal(out.numpy(), ref.numpy())


# ------------------------------------------------------------------------------------------------ 3-D parse
def _parse(dev, cm, thresh, max_person):
    """romp_bev_parse directly -> (rc, bids, czyx, confs) as numpy (empty arrays when rc != 0)."""
    from romp_amd import lib as L
    lib = L.load()
    cmd = cm.contiguous().float().to(dev)
    B = cmd.shape[0]
    cap = B * max(max_person, 1)
    bids = torch.full((cap,), -7, device=dev, dtype=torch.int32)
    czyx = torch.full((cap, 3), -7, device=dev, dtype=torch.int32)
    conf = torch.full((cap,), float('nan'), device=dev)
    ws = torch.empty(B * (2 + 2 * BEV_CAP + 2 * min(max(max_person, 1), 1024)), device=dev, dtype=torch.int32)
    if 1 <= max_person <= 1024:
        assert ws.numel() == lib.romp_bev_workspace_ints(B, max_person)
    n = C.c_int32(-1)
    rc = lib.romp_bev_parse(L.ptr(cmd), B, float(thresh), max_person, C.byref(n), L.ptr(bids), L.ptr(czyx), L.ptr(conf), L.ptr(ws), L.stream_ptr(dev))
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None, None, None
    N = n.value
    assert (bids[N:] == -7).all() and torch.isnan(conf[N:]).all(), 'rows beyond the count were written'
    return rc, bids[:N].cpu().numpy().astype(np.int64), czyx[:N].cpu().numpy().astype(np.int64), conf[:N].cpu().numpy()


def _same(got, want):
    assert np.array_equal(got[1], want[0]), 'batch ids differ'
    assert np.array_equal(got[2], want[1]), 'centre coordinates differ'
    assert np.array_equal(got[3], want[2]), 'scores differ'


@pytest.mark.parametrize('name', ['border', 'threshold'])
def test_parse_edges_vs_reference(dev, golden_dir, name):
    """Planted peaks over a low (partly negative) background: all 8 corners, 12 edges and 6 faces of the volume; a peak exactly equal
    to the threshold (excluded), one ulp above (kept), one ulp below.  Against the reference's own parse (bev_edges.npz) and the oracle."""
    g = np.load(os.path.join(golden_dir, 'bev_edges.npz'))
    case = K.edge_parse_cases()[name]
    cm = K.planted_volume(case['B'], case['seed'], case['peaks'], case['background'])
    got = _parse(dev, cm, case['thresh'], case['max_person'])
    assert got[0] == 0
    _same(got, (g[f'parse_{name}_bids'], g[f'parse_{name}_czyx'], g[f'parse_{name}_confs']))
    _same(got, BO.parse_3dcentermap(cm, case['thresh'], case['max_person']))
    if name == 'border':
        assert {tuple(r) for r in got[2][got[1] == 0].tolist()} == set(K.volume_border_sites())
    else:
        assert (cm < 0).any() and np.float32(case['thresh']) in cm.numpy() and len(got[1]) == 3


def _lattice(step):
    return [(d, h, w) for d in range(0, DEPTH, step) for h in range(0, MAP, step) for w in range(0, MAP, step)]


@pytest.mark.parametrize('max_person,n_peaks', [(1, 3), (64, 70), (1024, 1100)])
def test_parse_topk_cut_with_equal_scores(dev, max_person, n_peaks):
    """More than max_person isolated maxima in one image, three EQUAL scores straddling the cut (ranks max_person - 2 .. max_person):
    this project's rule is lower flat index first.  The reference's torch.topk leaves the order of equal scores unspecified, so this
    one case is judged against BO.parse_3dcentermap only.  A second image has fewer maxima than max_person."""
    rs = np.random.RandomState(max_person)
    sites = _lattice(5)
    pick = [sites[i] for i in rs.permutation(len(sites))[:n_peaks]]
    scores = (0.9 - 0.0005 * np.arange(n_peaks)).astype(np.float32)
    lo = max(max_person - 2, 0)
    scores[lo:lo + 3] = scores[lo]                                   # three equal scores, in random (not flat-index) order of sites
    assert len(set(scores.tolist())) == n_peaks - 2
    cm = torch.rand(2, DEPTH, MAP, MAP, generator=torch.Generator().manual_seed(3)) * 0.1 - 0.05
    for (d, h, w), s in zip(pick, scores):
        cm[0, d, h, w] = float(s)
    cm[1, 7, 9, 11] = 0.75
    got = _parse(dev, cm, 0.2, max_person)
    assert got[0] == 0
    want = BO.parse_3dcentermap(cm, 0.2, max_person)
    assert (want[0] == 0).sum() == max_person and (want[0] == 1).sum() == 1
    tied = np.nonzero(want[2] == scores[lo])[0]
    assert 1 <= len(tied) < 3, 'the cut must fall inside the tie'
    _same(got, want)


def test_parse_rejects_bad_arguments(dev):
    from romp_amd import lib as L
    lib = L.load()
    cm = torch.zeros(1, DEPTH, MAP, MAP)
    cm[0, 5, 5, 5] = 1.0
    for max_person, thresh, word in ((0, 0.1, 'max_person'), (1025, 0.1, 'max_person'), (64, 0.0, 'conf_thresh'), (64, -0.5, 'conf_thresh')):
        rc = _parse(dev, cm, thresh, max_person)[0]
        msg = lib.romp_last_error().decode()
        assert rc != 0 and word in msg, (max_person, thresh, rc, msg)
    got = _parse(dev, cm, 0.1, 64)                                   # and the next valid call is served
    assert got[0] == 0 and got[2].tolist() == [[5, 5, 5]] and got[3].tolist() == [1.0]


def test_parse_batch_of_70(dev):
    """B = 70 (the row offsets are a prefix sum that walks the images in steps of 64 lanes), a different count per image, images
    with no detection at the front, in the middle and at the end."""
    B = 70
    rs = np.random.RandomState(70)
    sites = _lattice(5)
    cm = torch.zeros(B, DEPTH, MAP, MAP)
    counts = [(b * 7) % 23 + 1 for b in range(B)]
    for b in (0, 1, 35, 63, 64, 69):
        counts[b] = 0
    counts[65], counts[2] = 64, 70                                    # one image exactly full, one beyond max_person
    for b in range(B):
        for j, i in enumerate(rs.permutation(len(sites))[:counts[b]]):
            d, h, w = sites[i]
            cm[b, d, h, w] = 0.3 + 0.009 * j + 0.0001 * b
    got = _parse(dev, cm, 0.25, 64)
    assert got[0] == 0
    want = BO.parse_3dcentermap(cm, 0.25, 64)
    assert np.bincount(want[0], minlength=B).tolist() == [min(c, 64) for c in counts]
    _same(got, want)


@pytest.mark.parametrize('name', NF.NAMES)
def test_parse_nonfinite_volumes(dev, name):
    """NaN, +inf and -inf voxels (tests/test_parse_nonfinite.py, where the oracle is pinned to the reference's own steps for these very
    volumes): the pool hands a NaN on, so a peak within two voxels of one is NOT a detection -- a `neighbour > value` test alone would
    keep it; a peak three away is; +inf peaks come first, by flat index among themselves; -inf changes nothing around it."""
    cm, kept = NF.case_3d(name)
    got = _parse(dev, cm, NF.THRESH, NF.MAX_PERSON)
    assert got[0] == 0
    want = BO.parse_3dcentermap(cm, NF.THRESH, NF.MAX_PERSON)
    print('%s: %d rows, the oracle has %d' % (name, len(got[1]), len(want[0])))
    assert sorted((int(b),) + tuple(r) for b, r in zip(want[0], want[1].tolist())) == kept
    _same(got, want)


def _capacity_volume(n_lit, seed):
    """n_lit isolated maxima with distinct scores on the stride-3 lattice (a 5^3 window does not reach a neighbour 3 away)."""
    sites = np.array(_lattice(3))
    assert len(sites) == 22 * 43 * 43 > BEV_CAP
    rs = np.random.RandomState(seed)
    pick = sites[rs.permutation(len(sites))[:n_lit]]
    sc = (0.5 + rs.permutation(n_lit).astype(np.float64) * 2.0 ** -18).astype(np.float32)
    assert len(np.unique(sc)) == n_lit
    vol = torch.zeros(DEPTH, MAP, MAP)
    vol[pick[:, 0], pick[:, 1], pick[:, 2]] = torch.from_numpy(sc)
    return vol


def test_parse_capacity_boundary(dev):
    """Exactly BEV_CAP = 32768 maxima above the threshold: served, and the top 64 equal the oracle's.  One more (in image 1 of 2):
    ROMP_ECAPACITY, an error return that names the image -- and the next call on the same stream, a normal volume, is right."""
    from romp_amd import lib as L
    lib = L.load()
    full = _capacity_volume(BEV_CAP, 1)
    got = _parse(dev, full[None], 0.25, 64)
    assert got[0] == 0
    want = BO.parse_3dcentermap(full[None], 0.25, 64)
    assert len(want[0]) == 64
    _same(got, want)
    normal = torch.zeros(DEPTH, MAP, MAP)
    normal[3, 4, 5], normal[60, 100, 20] = 0.5, 0.8
    over = torch.stack([normal, _capacity_volume(BEV_CAP + 1, 2)])
    rc = _parse(dev, over, 0.25, 64)[0]
    msg = lib.romp_last_error().decode()
    print('capacity message:', msg)
    assert rc == ROMP_ECAPACITY
    assert 'image 1' in msg and str(BEV_CAP + 1) in msg
    got = _parse(dev, torch.stack([normal, normal]), 0.25, 64)
    assert got[0] == 0
    _same(got, BO.parse_3dcentermap(torch.stack([normal, normal]), 0.25, 64))
    assert got[1].tolist() == [0, 0, 1, 1] and got[2][0].tolist() == [60, 100, 20]


# ------------------------------------------------------------------------------------------------ regression
def _mlp_weights(seed=0):
    """MLP weights whose rot6D outputs stay near the identity's 6-D code plus a moderate perturbation: every rotation angle is below
    3.0 (asserted by the test), so the axis-angle conversion is well conditioned for every row."""
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(128, 128, generator=g) * 0.5
    W1, b1 = torch.randn(512, 128, generator=g) / 128 ** 0.5, torch.randn(512, generator=g) * 0.1
    W2, b2 = torch.randn(512, 512, generator=g) / 512 ** 0.5, torch.randn(512, generator=g) * 0.1
    W3, b3 = torch.randn(143, 512, generator=g) / 512 ** 0.5, torch.randn(143, generator=g) * 0.1
    W3[:132] *= 0.35
    b3[:132] = b3[:132] + torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 0.0]).repeat(22)     # (a1, a2 interleaved: the identity)
    return emb, [(W1, b1), (W2, b2), (W3, b3)]


def _regress_inputs():
    """257 rows over 3 images: the fixture's edge cams, the float32 anchor ties, random cams for the rest; each at its own voxel of a
    NaN-filled cam_maps_3d.  Features: channel stride 256, offset 128, NaN in the other 128 channels."""
    rs = np.random.RandomState(5)
    ties = K.anchor_tie_scales()
    cams = K.edge_cams()
    tie_cams = np.array([[s, rs.uniform(-0.9, 0.9), rs.uniform(-0.9, 0.9)] for s, _ in ties], np.float32)
    M = 257
    extra = np.stack([rs.uniform(0.02, 8.0, M), rs.uniform(-1.1, 1.1, M), rs.uniform(-1.1, 1.1, M)], 1).astype(np.float32)
    allc = np.concatenate([cams, tie_cams, extra])[:M]
    assert len(cams) + len(tie_cams) <= M
    flat = rs.permutation(3 * VOX)[:M]
    bids = (flat // VOX).astype(np.int32)
    assert set(bids.tolist()) == {0, 1, 2}
    r = flat % VOX
    czyx = np.stack([r // (MAP * MAP), (r // MAP) % MAP, r % MAP], 1).astype(np.int32)
    cam3d = np.full((3, 3, DEPTH, MAP, MAP), np.nan, np.float32)
    for i in range(M):
        cam3d[bids[i], :, czyx[i, 0], czyx[i, 1], czyx[i, 2]] = allc[i]
    feat = np.full((3, MAP, MAP, 256), np.nan, np.float32)
    feat[..., 128:] = rs.randn(3, MAP, MAP, 128).astype(np.float32)
    return allc, len(cams), len(tie_cams), bids, czyx, cam3d, feat


@pytest.fixture(scope='module')
def regress_setup(dev):
    allc, n_edge, n_tie, bids, czyx, cam3d, feat = _regress_inputs()
    emb, layers = _mlp_weights()
    d = dict(allc=allc, n_edge=n_edge, n_tie=n_tie, bids=bids, czyx=czyx, feat=feat, emb=emb, layers=layers)
    d['cam3d_d'], d['feat_d'] = torch.from_numpy(cam3d).to(dev), torch.from_numpy(feat).to(dev)
    d['w_d'] = [emb.contiguous().to(dev)] + [t.to(dev) for W, b in layers for t in (W.t().contiguous(), b.contiguous())]
    return d


def _regress(dev, s, rows, poison=float('nan')):
    from romp_amd import lib as L
    lib = L.load()
    N = len(rows)
    n_alloc = max(N, 4)
    f32 = dict(device=dev, dtype=torch.float32)
    out = {k: torch.full((n_alloc, c), poison, **f32) for k, c in (('params_pred', 146), ('cam', 3), ('thetas', 72), ('betas', 11), ('cam_trans', 3))}
    out['cam_czyx'] = torch.full((n_alloc, 3), -7, device=dev, dtype=torch.int32)
    b = torch.from_numpy(np.ascontiguousarray(s['bids'][rows])).to(dev) if N else torch.zeros(4, device=dev, dtype=torch.int32)
    z = torch.from_numpy(np.ascontiguousarray(s['czyx'][rows])).to(dev) if N else torch.zeros(4, 3, device=dev, dtype=torch.int32)
    anchors = (C.c_float * DEPTH)(*BO.cam3dmap_anchor(60, MAP).astype(np.float32).tolist())
    feat_ptr = C.c_void_p(s['feat_d'].data_ptr() + 4 * 128)
    w = s['w_d']
    rc = lib.romp_bev_regress(L.ptr(s['cam3d_d']), feat_ptr, 256, N, L.ptr(b), L.ptr(z), anchors, *[L.ptr(t) for t in w],
                              L.ptr(out['params_pred']), L.ptr(out['cam_czyx']), L.ptr(out['cam']), L.ptr(out['thetas']),
                              L.ptr(out['betas']), L.ptr(out['cam_trans']), L.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def test_regress_empty_is_a_no_op(dev, regress_setup):
    rc, out = _regress(dev, regress_setup, np.zeros(0, np.int64), poison=123.0)
    assert rc == 0
    assert all((out[k] == 123.0).all() for k in ('params_pred', 'cam', 'thetas', 'betas', 'cam_trans')) and (out['cam_czyx'] == -7).all()


@pytest.mark.parametrize('N', [1, 64, 257])
def test_regress_edges(dev, golden_dir, regress_setup, N):
    """romp_bev_regress on crafted cams: scale on every anchor, on both sides of every midpoint, at float32 anchor TIES (26 pairs exist;
    np.argmin and the kernel both keep the lower index -- the reference's torch.argmin leaves it open, so ties are judged against
    the oracle only), beyond both ends of the anchor range, negative, and near -1e-3 / tan_fov; y, x at and beyond the clamp and
    on exact-integer centre coordinates.

    cam_trans: 8 * 2^-24 relative against float64 for every row whose denominator scale * tan_fov + 1e-3 does not cancel (scale
    >= 0: six float32 operations, one rounding each, plus margin for the float32 tan_fov).  Where it cancels (the rows near -1e-3 /
    tan_fov, depth of order 1e5) no float32 evaluation can meet a flat 8 ulp -- the reference's own float32 result is ~100 ulp from
    float64 there -- so the same 8 * 2^-24 is scaled by the denominator's condition number (|scale| tan_fov + 1e-3) / |scale tan_fov
    + 1e-3|, which is 1 on every other row."""
    s = regress_setup
    M = len(s['allc'])
    rows = {1: np.array([7]), 64: np.arange(0, M, 4)[:64], 257: np.arange(M)}[N]
    assert len(rows) == N
    rc, out = _regress(dev, s, rows)
    assert rc == 0
    cams = s['allc'][rows]
    # exact parts
    assert np.array_equal(out['cam'][:N], cams) and np.array_equal(out['params_pred'][:N, :3], cams), 'sampled voxel'
    want_czyx = BO.cam_to_czyx(cams)
    assert np.array_equal(out['cam_czyx'][:N], want_czyx), f'rows {np.nonzero((out["cam_czyx"][:N] != want_czyx).any(1))[0][:8]} differ'
    assert np.array_equal(out['betas'][:N], out['params_pred'][:N, 135:])
    assert np.array_equal(out['thetas'][:N, 66:], np.zeros((N, 6), np.float32))
    if N == 257:
        g = np.load(os.path.join(golden_dir, 'bev_edges.npz'))
        ne = s['n_edge']
        assert np.array_equal(cams[:ne], g['cams'])
        assert np.array_equal(out['cam_czyx'][:ne], g['cam_czyx']), "differs from the reference's cam -> centre coordinates"
        assert s['n_tie'] > 0
        ties = K.anchor_tie_scales()
        assert out['cam_czyx'][ne:ne + s['n_tie'], 0].tolist() == [max(k, 1) for _, k in ties], 'anchor tie: lower index first'
    # MLP: float64 on the same float32 inputs, running forward bound
    x = s['feat'][s['bids'][rows], want_czyx[:, 1], want_czyx[:, 2], 128:] + s['emb'].numpy()[want_czyx[:, 0]]
    assert x.dtype == np.float32 and np.isfinite(x).all()
    y, e = K.mlp_ref(x, [(W.numpy(), b.numpy()) for W, b in s['layers']])
    err = np.abs(out['params_pred'][:N, 3:].astype(np.float64) - y)
    r_mlp = (err / e).max()
    print(f'BOUND regress N={N} MLP: largest err/bound {r_mlp:.5f} (max-abs err {err.max():.3e}, bound max {e.max():.3e})')
    assert r_mlp <= 1.0
    # translation
    ref = K.cam_trans_ref(cams)
    sc = cams[:, 0].astype(np.float64)
    kappa = (np.abs(sc) * BO.TAN_FOV + 1e-3) / np.abs(sc * BO.TAN_FOV + 1e-3)
    assert (kappa[sc >= 0] == 1.0).all()
    terr = np.abs(out['cam_trans'][:N].astype(np.float64) - ref)
    r_tr = (terr / (8 * K.U * kappa[:, None] * np.abs(ref) + 1e-300)).max()
    print(f'BOUND regress N={N} cam_trans: largest err/bound {r_tr:.4f} (largest |depth| {np.abs(ref[:, 2]).max():.3e}, largest condition number {kappa.max():.1f})')
    assert r_tr <= 1.0
    if N == 257:
        assert np.abs(ref[:, 2]).max() > 5e4 and kappa.max() > 100
        tol = 16 * K.U * kappa[:ne, None] * np.abs(ref[:ne])                     # both sides carry their own 8 ulp
        assert (np.abs(out['cam_trans'][:ne].astype(np.float64) - g['cam_trans'].astype(np.float64)) <= tol).all()
    # rot6D -> axis-angle on the device's own params_pred, at test_rot6d_golden's tolerance, no row left out
    pk = BO.pack_params(out['params_pred'][:N])
    ang = np.linalg.norm(pk['smpl_thetas'][:, :66].reshape(N, 22, 3), axis=2)
    assert ang.max() < 3.0, 'the MLP weights must keep every rotation well conditioned'
    e_th = np.abs(out['thetas'][:N, :66] - pk['smpl_thetas'][:, :66]).max()
    print(f'BOUND regress N={N} thetas: max-abs err {e_th:.3e} / 2e-5 = {e_th / 2e-5:.4f} (largest angle {ang.max():.3f})')
    assert e_th <= 2e-5


# ------------------------------------------------------------------------------------------------ the head's 2-D convs
def _conv_runs(lib, op, B, f32):
    buf = C.create_string_buffer(128)
    runs = ([(1, -1)] if f32 else []) + [(0, -1)] + [(0, v) for v in range(lib.romp_conv_num_variants())
                                                      if lib.romp_conv_describe(C.byref(op), B, v, buf, 128) == 0]
    assert len(runs) >= 2
    return runs, buf


@pytest.mark.parametrize('fmt', ['f32', 'h2'])
@pytest.mark.parametrize('B', [1, 3])
def test_head_conv2_two_groups_residual(dev, B, fmt):
    """bev.heads.conv2: the groups = 2 (det_head | param_head) 128 -> 128 3x3 + BN + residual + ReLU, whose output is the persistent
    256-wide front-view feature buffer, by test_conv_layer's procedure (naive kernel, heuristic, every variant on offer; 3e-5
    against F.conv2d)."""
    import torch.nn.functional as F
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math, encode_h2, decode_h2, ACT_SHIFT
    lib = L.load()
    H = 64
    g = torch.Generator().manual_seed(77 + B)
    x = torch.randn(B, H, H, 256, generator=g)
    ws = [torch.randn(128, 128, 3, 3, generator=g) / (128 * 9) ** 0.5 for _ in range(2)]
    scs = [torch.rand(128, generator=g) + 0.5 for _ in range(2)]
    shs = [torch.randn(128, generator=g) * 0.1 for _ in range(2)]
    res = torch.randn(B, H, H, 256, generator=g)
    ref = F.conv2d(x.permute(0, 3, 1, 2), torch.cat(ws, 0), None, padding=1, groups=2)
    ref = torch.relu(ref * torch.cat(scs).view(1, -1, 1, 1) + torch.cat(shs).view(1, -1, 1, 1) + res.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    P = Program(dev)
    set_conv_math(P, 'all')
    P.buf_floats += [256 * H * H] * 2
    y = Act(P.alloc(256 * H * H, persistent=True), 256, H, H, 256)
    P.conv('bev.heads.conv2', Act(0, 256, H, H, 256), ws, scs, shs, 3, 1, True, res=Act(1, 256, H, H, 256), out=y, groups=2)
    op = P.ops[0]
    assert op.groups == 2 and op.in_gstride == 128 and op.out_gstride == 128 and op.res_gstride == 128 and op.out_cstride == 256
    x_in, res_in, out_h2 = x, res, False
    if fmt == 'h2':
        assert op.weight_h2
        out_h2 = True
        op.act_shift, op.in_fmt, op.out_fmt, op.res_fmt = ACT_SHIFT, L.FMT_H2, L.FMT_H2, L.FMT_H2
        x_in, res_in = encode_h2(x), encode_h2(res)
    xd, rd = x_in.to(dev), res_in.to(dev)
    runs, buf = _conv_runs(lib, op, B, fmt == 'f32')
    for mode, variant in runs:
        out = torch.full((B, H, H, 256), float('nan'), device=dev)
        L.check(lib.romp_conv_forward(C.byref(op), L.ptr(xd), L.ptr(rd), L.ptr(out), B, mode, variant, L.stream_ptr(dev)))
        torch.cuda.synchronize()
        o = decode_h2(out.cpu()) if out_h2 else out.cpu()
        err = (o - ref).abs().max().item()
        name = 'naive'
        if mode == 0:
            L.check(lib.romp_conv_describe(C.byref(op), B, variant, buf, 128))
            name = buf.value.decode()
        print(f'{name} (variant {variant}, {fmt}): max-abs err {err:.3e}')
        assert err < 3e-5, f'{name} err {err}'


@pytest.mark.parametrize('fmt', ['f32', 'h2'])
@pytest.mark.parametrize('B', [1, 3])
def test_head_det_out_reads_channel_slice(dev, B, fmt):
    """bev.det_out: the 128 -> 4 1x1 (bias, no BN, no ReLU) whose input is channels [0, 128) of the 256-stride feature buffer; the
    other 128 channels (param_head's features) are NaN here, so any read of them poisons the output.  Same procedure, 3e-5."""
    import torch.nn.functional as F
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math, encode_h2, ACT_SHIFT
    lib = L.load()
    H = 128
    g = torch.Generator().manual_seed(78 + B)
    x = torch.full((B, H, H, 256), float('nan'))
    x[..., :128] = torch.randn(B, H, H, 128, generator=g)
    w = torch.randn(4, 128, 1, 1, generator=g) / 128 ** 0.5
    bias = torch.randn(4, generator=g)
    ref = (F.conv2d(x[..., :128].permute(0, 3, 1, 2), w, bias)).permute(0, 2, 3, 1)
    P = Program(dev)
    set_conv_math(P, 'all')
    P.buf_floats.append(256 * H * H)
    P.conv('bev.det_out', Act(0, 128, H, H, 256, 0), [w], [torch.ones(4)], [bias], 1, 1, False)
    op = P.ops[0]
    assert op.in_cstride == 256 and op.in_coff == 0 and op.Cin == 128 and op.out_cstride == 4
    x_in = x
    if fmt == 'h2':
        assert op.weight_h2
        op.act_shift, op.in_fmt = ACT_SHIFT, L.FMT_H2
        x_in = encode_h2(x)
        assert torch.isnan(x_in[..., 128:].contiguous().view(torch.float16).float()).all()
    xd = x_in.to(dev)
    runs, buf = _conv_runs(lib, op, B, fmt == 'f32')
    for mode, variant in runs:
        out = torch.full((B, H, H, 4), float('nan'), device=dev)
        L.check(lib.romp_conv_forward(C.byref(op), L.ptr(xd), None, L.ptr(out), B, mode, variant, L.stream_ptr(dev)))
        torch.cuda.synchronize()
        o = out.cpu()
        name = 'naive'
        if mode == 0:
            L.check(lib.romp_conv_describe(C.byref(op), B, variant, buf, 128))
            name = buf.value.decode()
        assert not torch.isnan(o).any(), f'{name}: read outside the channel slice'
        err = (o - ref).abs().max().item()
        print(f'{name} (variant {variant}, {fmt}): max-abs err {err:.3e}')
        assert err < 3e-5, f'{name} err {err}'

