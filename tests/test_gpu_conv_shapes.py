"""The convolution-family kernels on NON-SQUARE feature maps and partial row tiles (run with -m gpu on the MI355X box).

Every other test of these kernels uses a square map whose side is a power of two (or 48): an H / W transposition in a tile decode, a
row stride taken from the wrong dimension, a store that ignores the row mask of a partial tile or a loader that ignores iy < H all
give the right answer there.  Here H != W throughout, the row counts are 13, 3, 20 and 24 (partial tiles behind full ones, a map
smaller than every tile, an odd input height under stride 2), and the single-layer sweep runs inside guarded buffers: bands of a
sentinel around the output (a stray store shows as a changed word), bands of NaN around the input and the residual (a stray load
shows as a wrong value).  The bands are ordinary memory of the same allocation: nothing here can fault.

Case tables and their no-device checks: tests/test_conv_shapes.py."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from test_conv_shapes import (BBLOCK_R, BBLOCK_STRIP, BBLOCK_V1, FUSEUP, SEAM, SHAPE_PARAMS, conv_weights, same_variants_as_square,
                              shape_id)
from test_gpu_parity import _fused_basic_block, _fuseup, _lower_conv_layer, _seam1x1, _seam1x1_downsample
from test_gpu_resnet import _parity_convs, _parity_convs_h2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from romp_amd import lib
    lib.load()                       # fail loudly if the HIP extension is missing
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------ single conv layers
SENTINEL = 0x5A5A5A5A                # the output bands (a finite float32: 1.5e16)
NAN_F32 = 0x7FC00000                 # input / residual bands read as float32 ...
NAN_H2 = 0x7E007E00                  # ... and as fp16 pairs (both units of an H2 octet are such words)


@functools.lru_cache(maxsize=2)
def _reference(case, H, W):
    """Inputs for B = 3 and the float64 reference, rounded to float32 (B = 1 takes the first image).  Treat as read-only."""
    cin, cout, k, s = case[:4]
    relu, use_res = case[5:7]
    relu_from = case[7] if len(case) > 7 else 0
    w, scale, shift = conv_weights(case)
    g = torch.Generator().manual_seed(7 * H + W + cin)
    x = torch.randn(3, H, W, cin, generator=g)
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    res = torch.randn(3, Ho, Wo, cout, generator=g) if use_res else None
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), None, stride=s, padding=k // 2)
    ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if res is not None:
        ref = ref + res.permute(0, 3, 1, 2).double()
    if relu:
        ref = torch.cat([ref[:, :relu_from], torch.relu(ref[:, relu_from:])], 1)
    return x, res, ref.permute(0, 2, 3, 1).float().contiguous(), (w, scale, shift)


class Guarded:
    """A tensor inside a larger allocation: `band` words of `fill` before and after it (a multiple of 64 words: the interior keeps
    the allocation's 256-byte alignment)."""

    def __init__(self, dev, shape, band, fill):
        self.band = (band + 63) // 64 * 64
        self.fill = fill
        n = 1
        for d in shape:
            n *= d
        self.raw = torch.empty(2 * self.band + n, dtype=torch.int32, device=dev)
        self.inner = self.raw[self.band:self.band + n].view(torch.float32).view(*shape)
        self.reset()

    def reset(self, value=None):
        self.raw.fill_(self.fill if self.fill < 2 ** 31 else self.fill - 2 ** 32)
        if value is None:
            self.inner.fill_(float('nan'))
        else:
            self.inner.copy_(value)

    def bands_intact(self):
        want = self.fill if self.fill < 2 ** 31 else self.fill - 2 ** 32
        lo, hi = self.raw[:self.band], self.raw[self.raw.numel() - self.band:]
        return bool((lo == want).all()) and bool((hi == want).all())


@pytest.mark.parametrize('case,H,W,fmt,B', SHAPE_PARAMS, ids=[shape_id(v) for v in SHAPE_PARAMS])
def test_conv_layer_nonsquare(dev, case, H, W, fmt, B):
    """test_conv_layer's sweep -- the naive kernel, the heuristic choice, every variant romp_conv_describe accepts -- on an H x W map
    with H != W, in guarded buffers, against conv2d in float64.  Bound: the family's 3e-5 max-abs on unit-scale inputs."""
    from romp_amd import lib as L
    from romp_amd.plan import encode_h2, decode_h2
    cin, cout, k, s = case[:4]
    assert H != W
    x, res, ref, wsb = _reference(case, H, W)
    x, ref = x[:B], ref[:B]
    res = res[:B] if res is not None else None
    Ho, Wo = ref.shape[1:3]
    P, op, out_h2 = _lower_conv_layer(dev, case, H, W, *wsb, fmt)
    lib = L.load()
    variants = same_variants_as_square(lib, dev, case, H, W, fmt, B, wsb, op)
    res_h2 = res is not None and op.res_fmt == L.FMT_H2
    x_in = encode_h2(x) if fmt == 'h2' else x
    res_in = encode_h2(res) if res_h2 else res
    # bands of at least 32 rows of the widest map: further than any tile reaches past the first / last image
    xg = Guarded(dev, x_in.shape, 32 * W * cin, NAN_H2 if fmt == 'h2' else NAN_F32)
    xg.reset(x_in.to(dev))
    rg = None
    if res is not None:
        rg = Guarded(dev, res_in.shape, 32 * W * cout, NAN_H2 if res_h2 else NAN_F32)
        rg.reset(res_in.to(dev))
    og = Guarded(dev, (B, Ho, Wo, cout), 32 * W * cout, SENTINEL)
    buf = C.create_string_buffer(128)
    runs = ([(1, -1)] if fmt == 'f32' else []) + [(0, -1)] + [(0, v) for v in variants]
    assert len(runs) >= 2
    for mode, variant in runs:
        og.reset()
        L.check(lib.romp_conv_forward(C.byref(op), L.ptr(xg.inner), L.ptr(rg.inner if rg else None), L.ptr(og.inner), B, mode, variant, L.stream_ptr(dev)))
        torch.cuda.synchronize()
        name = 'naive'
        if mode == 0:
            L.check(lib.romp_conv_describe(C.byref(op), B, variant, buf, 128))
            name = buf.value.decode()
        o = og.inner.cpu()
        if out_h2:
            o = decode_h2(o)
        assert og.bands_intact(), '%s (variant %d) wrote outside its %d images of %dx%d' % (name, variant, B, Ho, Wo)
        assert not bool(torch.isnan(o).any()), '%s (variant %d) left NaN: rows %s' % (name, variant, sorted(set(torch.isnan(o).nonzero()[:, 1].tolist())))
        err = (o - ref).abs().max().item()
        print(f'{name} (variant {variant}, {fmt}) B={B} {H}x{W} -> {Ho}x{Wo}: max-abs err {err:.3e} (ref absmax {ref.abs().max():.2f})')
        assert err < 3e-5, f'{name} err {err}'
    assert xg.bands_intact() and (rg is None or rg.bands_intact())


# ------------------------------------------------------------------------------ fused chains
@pytest.mark.parametrize('B,H,W,Cc,impl', [c + ('r',) for c in BBLOCK_R] + [c + ('v1',) for c in BBLOCK_V1])
def test_fused_basic_block_nonsquare(dev, B, H, W, Cc, impl, monkeypatch):
    """conv_h2c.h ('r') / conv_h2b.hip ('v1') with more tile columns than tile rows and the other way round, against float64."""
    monkeypatch.setenv('ROMP_BBLOCK_RUN', '0')
    _fused_basic_block(dev, B, H, Cc, impl, monkeypatch, W=W, ref_dtype=torch.float64)


@pytest.mark.parametrize('B,H,W,Cc,run', BBLOCK_STRIP)
def test_fused_basic_block_strip_nonsquare(dev, B, H, W, Cc, run, monkeypatch):
    """The halo-carrying form: runs of vertically consecutive tiles on maps whose tile rows and tile columns differ."""
    if run is None:
        monkeypatch.delenv('ROMP_BBLOCK_RUN', raising=False)
    else:
        assert (H // 8) % run == 0
        monkeypatch.setenv('ROMP_BBLOCK_RUN', str(run))
    _fused_basic_block(dev, B, H, Cc, 'r', monkeypatch, W=W, ref_dtype=torch.float64)


@pytest.mark.parametrize('CO,NUP,ND,H,W,B', FUSEUP)
def test_fuseup_nonsquare(dev, CO, NUP, ND, H, W, B):
    """conv_fup.hip's three tile shapes (8x64, 8x32, 4x32) on maps with H != W, against float64."""
    _fuseup(dev, CO, NUP, ND, H, B, W=W, ref_dtype=torch.float64)


@pytest.mark.parametrize('B,H,W', SEAM)
def test_seam1x1_nonsquare(dev, B, H, W, monkeypatch):
    _seam1x1(dev, B, H, monkeypatch, W=W)


@pytest.mark.parametrize('B,H,W', SEAM)
def test_seam1x1_downsample_nonsquare(dev, B, H, W, monkeypatch):
    _seam1x1_downsample(dev, B, H, monkeypatch, W=W)


# ------------------------------------------------------------------------------ the general fuse sum
FUSESUM_CONFIGS = (((0, 0, 0), 0, 0), ((1, 1, 1), 1, 0), ((1, 0, 1), 0, 0), ((0, 1, 0), 1, 0), ((1, 1, 1), 1, 32), ((0, 0, 1), 0, 64))


def _fusesum_op(H, W, Cc, fmts, ofmt, coff1, wide):
    from romp_amd.lib import RompOp, OP_FUSESUM, BUF_NONE
    op = RompOp()
    op.kind, op.in_buf, op.res_buf, op.out_buf = OP_FUSESUM, BUF_NONE, BUF_NONE, 3
    op.H, op.W, op.Cin, op.Cout, op.relu, op.n_terms = H, W, Cc, Cc, 1, 3
    op.out_cstride, op.out_fmt, op.act_shift = Cc, ofmt, 4
    for k in range(3):
        op.term_buf[k], op.term_shift[k], op.term_cstride[k], op.term_fmt[k] = k, k, Cc, fmts[k]
    op.term_cstride[1], op.term_coff[1] = wide, coff1
    return op


# (8, 24, 64): W no power of two; (8, 32, 96): C / 8 = 12; (12, 20, 96): both; (24, 12, 64): H > W.  Rows of 192 / 384 / 240 / 96
# (pixel, octet) units: workgroups of 128, 256, 128 and 64 threads
@pytest.mark.parametrize('H,W,Cc', [(8, 24, 64), (8, 32, 96), (12, 20, 96), (24, 12, 64)])
def test_fusesum_general_form(dev, H, W, Cc):
    """fusesum_kernel<0> (csrc/stem_fuse.hip: the form with divisions, taken when W or C / 8 is no power of two) with terms at shifts
    0, 1 and 2 in test_fusesum_formats' six format / channel-slice configurations.  The reference is exact: relu(t0 + up(t1, 2) +
    up(t2, 4)) in float64; bound 2e-6 as there."""
    from romp_amd import lib as L
    from romp_amd.lib import RompOp
    from romp_amd.plan import encode_h2, decode_h2
    assert (W & (W - 1)) or ((Cc // 8) & (Cc // 8 - 1)), 'the power-of-two form would run'
    lib = L.load()
    B = 2
    g = torch.Generator().manual_seed(H * 100 + W + Cc)
    ts = [torch.randn(B, H >> k, W >> k, Cc, generator=g) for k in range(3)]
    up = lambda t, f: t.repeat_interleave(f, 1).repeat_interleave(f, 2)
    ref = torch.relu(ts[0].double() + up(ts[1].double(), 2) + up(ts[2].double(), 4)).float()
    for fmts, ofmt, coff1 in FUSESUM_CONFIGS:
        wide = Cc + 96 if coff1 else Cc                      # channel stride of term 1's buffer
        op = _fusesum_op(H, W, Cc, fmts, ofmt, coff1, wide)
        sizes = [H * W * Cc, H * W * wide // 4, H * W * Cc // 16, H * W * Cc]
        h = C.c_void_p()
        L.check(lib.romp_net_create(C.byref(h), (RompOp * 1)(op), 1, (C.c_int64 * 4)(*sizes), 4, B))
        try:
            for k, t in enumerate(ts):
                if k == 1 and coff1:                         # embed the term in a wider tensor of other data
                    w_ = torch.randn(B, H // 2, W // 2, wide, generator=g) * 7.0
                    w_[..., coff1:coff1 + Cc] = t
                    t = w_
                td = (encode_h2(t) if fmts[k] else t).to(dev).contiguous()
                L.check(lib.romp_net_write_buffer(h, k, L.ptr(td), td.numel(), L.stream_ptr(dev)))
            dummy = torch.zeros(B * 16, device=dev)
            L.check(lib.romp_net_forward(h, L.ptr(dummy), B, L.ptr(dummy), L.ptr(dummy), L.stream_ptr(dev)))
            out = torch.empty(B * sizes[3], device=dev)
            L.check(lib.romp_net_read_buffer(h, 3, B, L.ptr(out), out.numel(), L.stream_ptr(dev)))
            torch.cuda.synchronize()
            o = out.cpu().reshape(B, H, W, Cc)
            if ofmt:
                o = decode_h2(o)
            err = (o - ref).abs().max().item()
            print(f'fusesum {H}x{W}x{Cc} term fmts', fmts, 'out fmt', ofmt, 'max-abs err %.3e' % err)
            assert err < 2e-6
        finally:
            lib.romp_net_destroy(h)


@pytest.mark.parametrize('H,W,bad', [(8, 6, 'W'), (6, 8, 'H')])
def test_fusesum_refuses_a_shift_that_does_not_divide_the_map(dev, H, W, bad):
    """A term at 1 / 4 resolution of a map whose width (height) is no multiple of 4: launch_fusesum returns an error that names the
    dimension and launches nothing (the output buffer keeps its contents)."""
    from romp_amd import lib as L
    from romp_amd.lib import RompOp
    lib = L.load()
    B, Cc = 1, 64
    op = _fusesum_op(H, W, Cc, (0, 0, 0), 0, 0, Cc)
    sizes = [H * W * Cc, (H // 2) * (W // 2) * Cc, ((H + 3) // 4) * ((W + 3) // 4) * Cc, H * W * Cc]
    h = C.c_void_p()
    L.check(lib.romp_net_create(C.byref(h), (RompOp * 1)(op), 1, (C.c_int64 * 4)(*sizes), 4, B))
    try:
        for k in range(3):
            L.check(lib.romp_net_write_buffer(h, k, L.ptr(torch.ones(sizes[k], device=dev)), sizes[k], L.stream_ptr(dev)))
        mark = torch.full((sizes[3],), -7.0, device=dev)
        L.check(lib.romp_net_write_buffer(h, 3, L.ptr(mark), sizes[3], L.stream_ptr(dev)))
        dummy = torch.zeros(16, device=dev)
        rc = lib.romp_net_forward(h, L.ptr(dummy), B, L.ptr(dummy), L.ptr(dummy), L.stream_ptr(dev))
        msg = lib.romp_last_error().decode()
        assert rc != 0 and ('term 2 shift 2 does not divide %s' % bad) in msg, (rc, msg)
        out = torch.empty(sizes[3], device=dev)
        L.check(lib.romp_net_read_buffer(h, 3, B, L.ptr(out), sizes[3], L.stream_ptr(dev)))
        torch.cuda.synchronize()
        assert torch.equal(out, mark), 'a kernel ran'
    finally:
        lib.romp_net_destroy(h)


# ------------------------------------------------------------------------------ transposed-conv parity layers
# input maps 6 x 16 -> 12 x 32 and 32 x 16 -> 64 x 32.  (A 16 x 8 input cannot run: its parity convs have 8 output columns, no kernel
# variant has tiles narrower than 16; 32 x 16 is the smallest map with H > W that can.)
@pytest.mark.parametrize('cin,cout,H,W', [(256, 128, 6, 16), (256, 128, 32, 16)])
def test_transposed_conv_as_parity_convs_nonsquare(dev, cin, cout, H, W):
    _parity_convs(dev, cin, cout, H, W)


@pytest.mark.parametrize('cin,cout,H,W', [(256, 128, 6, 16), (256, 128, 32, 16)])
def test_transposed_conv_as_parity_convs_h2_nonsquare(dev, cin, cout, H, W):
    _parity_convs_h2(dev, cin, cout, H, W)
