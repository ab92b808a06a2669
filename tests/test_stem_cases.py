"""tests/stem_cases.py without a device: the tables lower to the op kinds tests/test_gpu_stem_edges.py expects, the BatchNorm shifts
leave about half of every layer's pre-activations positive, the partial-round cases are partial on 256 CUs, the max-pool reference is
what a hand-written loop gives, and the launchers' refusals carry their names before any device is touched."""
import ctypes as C

import pytest
import torch

import stem_cases as SC


def _kinds(P):
    return [o.kind for o in P.ops]


@pytest.mark.parametrize('H,W', SC.STEM3_SIZES)
def test_stem3_tables_lower_to_the_stem(H, W):
    from romp_amd import lib as L
    c = SC.stem3_case(H, W)
    assert H % 32 == 0 and W % 32 == 0
    for kernel, fmt in SC.STEM3_FORMS:
        P, op = SC.lower_stem3('cpu', c, H, W, kernel, fmt)
        assert _kinds(P) == [L.OP_STEM] and op.in_buf == L.BUF_IMAGE
        assert bool(op.flags & L.OPF_STEM_VALU) == (kernel == 'valu') and op.out_fmt == (L.FMT_H2 if fmt == 'h2' else L.FMT_F32)
    assert float(c['w'].abs().max()) * 256.0 < 65504.0, 'the MFMA form must be eligible'
    assert sorted(set(c['img'].flatten().tolist()) - set(range(256))) == [], 'integer-valued pixels in 0..255'
    assert {(k, f) for (_, _, _, k, f) in SC.STEM3} == set(SC.STEM3_FORMS) and {B for (_, _, B, _, _) in SC.STEM3} == {1, 3}
    Hw, Ww, Bw, cs, co = SC.STEM3_WIDE
    assert (Hw, Ww) in SC.STEM3_SIZES and cs - 64 == 32 and co == 16 and co % 4 == 0


@pytest.mark.parametrize('H,W', SC.STEM3_SIZES)
def test_stem3_relu_share(H, W):
    """Random frames by construction; the constant frames (all 0, all 255) with the same layer constants: every tap is -1 / +1, a
    channel's sign is the sign of its weight sum, and still about half of the values pass the ReLU."""
    for frame in (None,) + SC.CONST_FRAMES:
        s = SC.stem3_case(H, W, frame)['share']
        print('stem3 %dx%d frame %s: %.3f of the pre-ReLU values positive' % (H, W, frame, s))
        assert SC.SHARE[0] <= s <= SC.SHARE[1], (H, W, frame, s)


def test_constant_frames_show_padding_before_normalisation():
    """x / 255 * 2 - 1 of 0 and 255 is exactly -1 and +1; were the padding applied BEFORE the normalisation, the border taps would
    read -1: on the all-0 frame every border pixel would equal its interior neighbour, here it differs by a weight sum."""
    for frame in SC.CONST_FRAMES:
        assert float(SC.normalise_hrnet(torch.tensor([frame]))) == (-1.0 if frame == 0.0 else 1.0)
    c = SC.stem3_case(32, 32, 0.0)
    import torch.nn.functional as F
    x = torch.full((3, 3, 34, 34), -1.0, dtype=torch.float64)                   # the wrong order: pad (with pixel value 0), then normalise
    wrong = torch.relu(F.conv2d(x, c['w'].double(), None, stride=2, padding=0) * c['scale'].double().view(1, -1, 1, 1) + c['shift'].double().view(1, -1, 1, 1))
    d = (wrong.permute(0, 2, 3, 1).float() - c['ref']).abs()
    assert float(d[:, 1:, 1:].max()) < 1e-6 and float(d[:, 0].max()) > 0.1 and float(d[:, :, 0].max()) > 0.1


@pytest.mark.parametrize('H,W', SC.STEM3_SIZES + [(32, 64), (320, 384)])
def test_stem7_relu_share_and_lowering(H, W, monkeypatch):
    from romp_amd import lib as L
    c = SC.stem7_case(H, W)
    print('stem7 %dx%d: %.3f of the pre-ReLU values positive, float32 CPU error %.2e' % (H, W, c['share'], c['err_cpu']))
    assert SC.SHARE[0] <= c['share'] <= SC.SHARE[1]
    assert torch.equal(c['pooled'], SC.pool_reference(c['m'])), 'the pool of the rounded map is the rounded pool: max commutes with rounding'
    P, op = SC.stem7_alone('cpu', c, H, W)
    assert _kinds(P) == [L.OP_STEM7] and (op.in_buf, op.out_buf) == (L.BUF_IMAGE, L.BUF_CENTER)
    monkeypatch.delenv('ROMP_STEM', raising=False)
    for fmt in ('h2', 'f32'):
        P, ops, y = SC.lower_stem7('cpu', c, H, W, fmt)
        assert P.fused_stem7p == 1 and _kinds(P) == [L.OP_NOP, L.OP_STEM7P]
        assert P.ops[1].out_fmt == (L.FMT_H2 if fmt == 'h2' else L.FMT_F32) and P.buf_floats[y.buf] == (H // 4) * (W // 4) * 64
    monkeypatch.setenv('ROMP_STEM', 'valu')
    P, ops, y = SC.lower_stem7('cpu', c, H, W, 'f32')
    assert P.fused_stem7p == 0 and _kinds(P) == [L.OP_STEM7, L.OP_MAXPOOL] and P.ops[1].out_fmt == L.FMT_F32


@pytest.mark.parametrize('H,W', sorted({c[1:] for c in SC.STEM2}) + [(320, 384)])
def test_stem2_relu_share_and_lowering(H, W, monkeypatch):
    from romp_amd import lib as L
    c = SC.stem2_case(H, W)
    print('stem2 %dx%d: %.3f / %.3f of the two layers\' pre-ReLU values positive' % ((H, W) + c['share']))
    assert all(SC.SHARE[0] <= s <= SC.SHARE[1] for s in c['share'])
    monkeypatch.setenv('ROMP_FUSE_STEM2', '1')
    P, ops, b = SC.lower_stem2('cpu', c, H, W)
    assert P.fused_stem2 == 1 and _kinds(P)[:2] == [L.OP_NOP, L.OP_STEM2] and P.buf_floats[b.buf] == (H // 4) * (W // 4) * 64
    monkeypatch.setenv('ROMP_FUSE_STEM2', '0')
    P, ops, b = SC.lower_stem2('cpu', c, H, W)
    assert P.fused_stem2 == 0 and _kinds(P)[:2] == [L.OP_STEM, L.OP_CONV]


def test_partial_rounds_on_256_cus():
    """stem2: B = 3 at 320 x 384 is 3 * 20 * 6 = 360 tiles of 16 x 64 image pixels on a grid of 256: one full round and 104 tiles in the
    second.  stem7p: 3 * 20 * 12 = 720 tiles of 16 x 32 on a grid of 2 * 256 = 512: one full round and 208.  Every other case is under
    one round (and a device with another CU count still finds a candidate)."""
    case, tiles, grid = SC.partial_round('stem2', 256)
    assert (case, tiles, grid) == ((3, 320, 384), 360, 256) and tiles - grid == 104 and tiles > grid and tiles % grid != 0
    case, tiles, grid = SC.partial_round('stem7p', 256)
    assert (case, tiles, grid) == ((3, 320, 384), 720, 512) and tiles - grid == 208 and tiles > grid and tiles % grid != 0
    assert all(SC.stem2_tiles(*c) <= 256 for c in SC.STEM2) and all(SC.stem7p_tiles(*c) <= 512 for c in SC.STEM7P)
    for cus in (64, 80, 104, 120, 228, 256, 304):
        for kind in ('stem2', 'stem7p'):
            _, tiles, grid = SC.partial_round(kind, cus)
            assert tiles > grid and tiles % grid != 0


def test_maxpool_reference_is_the_hand_written_loop():
    for kind in SC.POOL_INPUTS:
        x = SC.pool_input(3, 2, 6, 4, kind)
        ref = SC.pool_reference(x)
        assert ref.shape == (3, 1, 3, 4) and torch.equal(ref, SC.pool_by_hand(x)), kind
        if kind == 'negative':
            assert float(x.max()) < 0 and float(ref.max()) < 0, 'a pool padded with 0 would answer 0 everywhere'
        if kind == 'inf':
            assert bool(torch.isinf(x).any()) and bool((x == float('inf')).any()) and bool((x == -float('inf')).any())
        if kind == 'normal':
            assert float(ref.min()) < 0, 'a window whose maximum is negative: a pool padded with 0 would answer 0 there'
    for (H, W, Cc, ics, ocs) in SC.POOL:
        assert H % 2 == 0 and W % 2 == 0 and Cc % 4 == 0 and ics >= Cc and ocs >= Cc and ics % 4 == 0 and ocs % 4 == 0
    assert sum(1 for p in SC.POOL if p[3] > p[2] and p[4] > p[2]) == 1
    B, H, W, Cc = SC.pool_big_shape()
    items = B * (H // 2) * (W // 2) * (Cc // 4)
    assert items > SC.POOL_GRID_CAP * SC.POOL_THREADS and B * H * W * Cc * 4 < 400e6
    assert items - (W // 2) * (Cc // 4) * 2 <= SC.POOL_GRID_CAP * SC.POOL_THREADS, 'the smallest such map of its width'


def test_ksum_tables():
    assert [s[3] % 8 for s in SC.KSUM_SHAPES] == [1, 0, 1, 1, 7] and [s[3] for s in SC.KSUM_SHAPES] == [1, 8, 9, 17, 7]
    for shape in SC.KSUM_SHAPES:
        H, W, Cc, G = shape
        cfgs = SC.ksum_configs(shape)
        assert {(r, f) for r, f, _, _ in cfgs} == {(0, 0), (1, 0), (1, 8), (1, Cc - 8)}
        assert {x for _, _, x, _ in cfgs} == {'none', 'f32', 'h2'} and {x for _, _, _, x in cfgs} == {'f32', 'h2'}
        c = SC.ksum_case(SC.KSUM_B, H, W, Cc, G)
        mag = c['mag'].tolist()
        assert len(set(mag)) == G and mag[-1] == max(mag)
        # a dropped or a doubled last slice moves the reference far beyond any bound in use
        ref, err_cpu = SC.ksum_reference(c, 0, 0, 'none')
        if G > 1:
            dropped = dict(c, part=c['part'][..., :G - 1, :])
            d = (SC.ksum_reference(dropped, 0, 0, 'none')[0] - ref).abs().max().item() / ref.abs().max().item()
            assert d > 1e-2 > 100 * SC.f32_bound(err_cpu, ref.abs().max().item(), 4)
        # relu_from: the channels below it keep their negative values, the ones from it on have none
        for relu, rf, _, _ in cfgs:
            r, _ = SC.ksum_reference(c, relu, rf, 'f32')
            if relu:
                assert float(r[..., rf:].min()) >= 0 if rf < Cc else True
                assert rf == 0 or float(r[..., :rf].min()) < 0
                assert rf >= Cc or float((r[..., rf:rf + 8] == 0).float().mean()) > 0.2, 'c > relu_from instead of >= would leave this octet unclamped'
    shape, rf, res, rco, rcs, oco, ocs = SC.KSUM_WIDE
    assert shape in SC.KSUM_SHAPES and rco == 8 and oco == 8 and rcs > shape[2] + rco - 1 and ocs > shape[2] + oco - 1 and res == 'h2'
    B, H, W, Cc, G = SC.ksum_big_shape()
    assert B * H * W * Cc // 8 > SC.KSUM_GRID_CAP * SC.KSUM_THREADS and B * H * W * Cc * G * 4 < 400e6
    x = torch.randn(4, 16) * 3.0
    from romp_amd.plan import encode_h2, decode_h2
    assert torch.equal(SC.h2_value(x).float(), decode_h2(encode_h2(x))) and float((SC.h2_value(x) - x.double()).abs().max()) <= SC.h2_quantum(float(x.abs().max()))


def test_launchers_refuse_by_name_without_a_device(monkeypatch):
    """A 48 x 64 image for the stems, an odd map for the pool, a ksum whose in_cstride is not groups * Cout: romp_net_create (and
    romp_conv_forward for a stand-alone stem) run the launchers' checks on the ops before they touch the device, so the named error
    comes back on a host without one, and no net is made."""
    from romp_amd import lib as L
    lib = L.load()
    monkeypatch.delenv('ROMP_STEM', raising=False)
    monkeypatch.delenv('ROMP_FUSE_STEM2', raising=False)
    c3 = dict(w=torch.randn(64, 3, 3, 3) * 0.1, scale=torch.ones(64), shift=torch.zeros(64))
    c7 = dict(w=torch.randn(64, 3, 7, 7) * 0.1, scale=torch.ones(64), shift=torch.zeros(64))
    _, stem = SC.lower_stem3('cpu', c3, 48, 64, 'valu', 'f32')
    _, stem7 = SC.stem7_alone('cpu', c7, 48, 64)
    P7, _, _ = SC.lower_stem7('cpu', c7, 48, 64, 'h2')                      # (the plan does not fuse a 48-row image: [STEM7, MAXPOOL])
    assert _kinds(P7) == [L.OP_STEM7, L.OP_MAXPOOL]
    stem7p = L.RompOp.from_buffer_copy(stem7)
    stem7p.kind = L.OP_STEM7P
    consts = torch.zeros(16)
    bad_ksum = SC.ksum_op(4, 8, 16, 3, 0, 0, 'none', 'f32', consts.data_ptr(), consts.data_ptr())
    bad_ksum.in_cstride = 3 * 16 + 8
    refusals = [([stem], 'stem: input 48x64 must be a multiple of 32'), ([stem7], 'stem7: input 48x64 must be a multiple of 32'),
                ([stem7p], 'stem7p: input 48x64 must be a multiple of 32'), ([SC.pool_op(6, 5, 4, 4, 4)], 'maxpool: bad shape'),
                ([SC.pool_op(5, 6, 4, 4, 4)], 'maxpool: bad shape'), ([bad_ksum], 'ksum: partials must be 3 x 16 channels')]
    for ops, msg in refusals:
        h = C.c_void_p()
        rc = lib.romp_net_create(C.byref(h), (L.RompOp * len(ops))(*ops), len(ops), (C.c_int64 * 1)(64), 1, 1)
        got = lib.romp_last_error().decode()
        assert rc == -1 and msg in got and not h.value, (msg, rc, got)                 # ROMP_EINVAL
    x, o = torch.zeros(1, 48, 64, 3), torch.zeros(1, 24, 32, 64)
    rc = lib.romp_conv_forward(C.byref(stem), L.ptr(x), None, L.ptr(o), 1, 0, -1, None)
    assert rc == -1 and 'stem: input 48x64 must be a multiple of 32' in lib.romp_last_error().decode()
    assert not bool(o.any())
    # the fused stem2 refuses a 48-row image at the plan already (no STEM2 op), and its launcher's own check by name
    c2 = SC.stem2_case(64, 64)
    monkeypatch.setenv('ROMP_FUSE_STEM2', '1')
    P, ops, _ = SC.lower_stem2('cpu', c2, 64, 64)
    assert _kinds(P)[:2] == [L.OP_NOP, L.OP_STEM2]
    ops[0].H = ops[0].W = 96
    ops[1].H = ops[1].W = 48
    h = C.c_void_p()
    rc = lib.romp_net_create(C.byref(h), ops, len(P.ops), (C.c_int64 * len(P.buf_floats))(*P.buf_floats), len(P.buf_floats), 1)
    assert rc == -1 and 'stem2: 96x96 image: a multiple of 64 expected' in lib.romp_last_error().decode() and not h.value
