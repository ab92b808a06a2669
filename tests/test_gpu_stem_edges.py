"""The kernels that read the image first, the max-pool and the split-K tail, each ALONE against float64 (run with -m gpu on the MI355X
box): csrc/stem_fuse.hip (stem_conv_kernel, stem_mfma_kernel, stem7_conv_kernel, maxpool3s2_kernel, ksum_kernel), csrc/stem2.hip,
csrc/stem7p.hip.  Case tables, references and their no-device checks: tests/stem_cases.py, tests/test_stem_cases.py.

Every launch runs inside guards (test_gpu_conv_shapes.py's): a band of NaN around what the kernel reads (a stray load shows as a
wrong value; for the max-pool the band is +inf, because fmaxf drops a NaN), a band of a sentinel around what it writes (a stray
store shows as a changed word).  The bands are ordinary memory of the same allocation: nothing here can fault.  Which guard an op gets:

  ROMP_OP_STEM (3x3)     romp_conv_forward takes caller pointers: image and output both in bands
  ROMP_OP_STEM7, MAXPOOL one-op nets from ROMP_BUF_IMAGE to ROMP_BUF_CENTER: caller pointers, both in bands
  ROMP_OP_KSUM           partials through ROMP_BUF_IMAGE and the result through ROMP_BUF_CENTER in bands; the residual can only be an
                         arena buffer: a spare batch image of NaN behind it
  ROMP_OP_STEM2, STEM7P  the image in bands; the output is an arena buffer: the net is made for B + 1 images, the buffer pre-filled
                         with the sentinel, B images run, image B + 1 must keep it

Bounds: exact operations (max-pool, sentinels) bit for bit; float32 kernels 8 x the error of float32 torch on the CPU, both against
float64 over max |ref| (stem_cases.f32_bound; ksum, where that error can be 0, not below 4 ulp); H2 / f16x2 kernels the bounds the
project holds them to (3e-5 max-abs on the unit-scale 3x3 stem, 3e-5 / 2e-5 of max |ref| for stem2 / stem7p, 2e-5 max(1, max |ref|)
between a fused kernel and its unfused lowering); ksum's H2 output: its float32 bound plus the format's own step (stem_cases.h2_quantum)."""
import ctypes as C

import pytest
import torch

import stem_cases as SC
from test_gpu_conv_shapes import Guarded, SENTINEL, NAN_F32, NAN_H2  # noqa: F401  (NAN_H2: H2 inputs have no case here, kept with its siblings)

pytestmark = pytest.mark.gpu

POS_INF = 0x7F800000


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from romp_amd import lib
    lib.load()                       # fail loudly if the HIP extension is missing
    return torch.device('cuda:0')


def _guard_in(dev, t, band, fill=NAN_F32):
    g = Guarded(dev, t.shape, band, fill)
    g.reset(t.to(dev))
    return g


def _guard_out(dev, shape, band, sentinel_inside=False):
    """Output guard; interior NaN (an unwritten element shows), or the sentinel where only a slice of the channels is written."""
    g = Guarded(dev, shape, band, SENTINEL)
    if sentinel_inside:
        g.raw.fill_(SENTINEL)
    return g


def _is_sentinel(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


def _check_guards(what, og, *inputs):
    assert og.bands_intact(), '%s wrote outside its output' % what
    for xg, want in inputs:
        assert xg.bands_intact() and torch.equal(xg.inner.view(torch.int32), want.to(xg.inner.device).view(torch.int32)), '%s changed its input' % what


class OneOpNet:
    """A net of the given ops (romp_net_create) for `max_batch` images."""

    def __init__(self, dev, ops, buf_floats, max_batch):
        from romp_amd import lib as L
        self.L, self.lib, self.dev = L, L.load(), dev
        self.h = C.c_void_p()
        arr = ops if isinstance(ops, C.Array) else (L.RompOp * len(ops))(*ops)
        sizes = (C.c_int64 * max(1, len(buf_floats)))(*buf_floats)
        L.check(self.lib.romp_net_create(C.byref(self.h), arr, len(arr), sizes, len(buf_floats), max_batch))
        self.dummy = torch.zeros(64, device=dev)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.romp_net_destroy(self.h)

    def forward(self, image, B, center=None):
        L = self.L
        L.check(self.lib.romp_net_forward(self.h, L.ptr(image), B, L.ptr(self.dummy if center is None else center), L.ptr(self.dummy), L.stream_ptr(self.dev)))
        torch.cuda.synchronize()

    def write(self, buf, t):
        t = t.to(self.dev).contiguous()
        self.L.check(self.lib.romp_net_write_buffer(self.h, buf, self.L.ptr(t), t.numel(), self.L.stream_ptr(self.dev)))
        torch.cuda.synchronize()

    def read(self, buf, B, n):
        out = torch.empty(n, device=self.dev)
        self.L.check(self.lib.romp_net_read_buffer(self.h, buf, B, self.L.ptr(out), n, self.L.stream_ptr(self.dev)))
        torch.cuda.synchronize()
        return out.cpu()


# ------------------------------------------------------------------------------ the 3x3 stem
def _run_stem3(dev, c, H, W, B, kernel, fmt, cs=64, co=0):
    """-> the kernel's output (B, H/2, W/2, 64) as float32, guards checked."""
    from romp_amd import lib as L
    from romp_amd.plan import decode_h2
    P, op = SC.lower_stem3(dev, c, H, W, kernel, fmt, cs, co)
    img = c['img'][:B].contiguous()
    xg = _guard_in(dev, img, 32 * W * 3)
    og = _guard_out(dev, (B, H // 2, W // 2, cs), 32 * (W // 2) * cs, sentinel_inside=cs != 64)
    L.check(L.load().romp_conv_forward(C.byref(op), L.ptr(xg.inner), None, L.ptr(og.inner), B, 0, -1, L.stream_ptr(dev)))
    torch.cuda.synchronize()
    what = 'stem %s %s B=%d %dx%d' % (kernel, fmt, B, H, W)
    _check_guards(what, og, (xg, img))
    o = og.inner.cpu()
    if cs != 64:
        assert _is_sentinel(o[..., :co]) and _is_sentinel(o[..., co + 64:]), '%s wrote channels outside its slice' % what
        o = o[..., co:co + 64].contiguous()
    if fmt == 'h2':
        o = decode_h2(o)
    assert not bool(torch.isnan(o).any()), '%s left NaN' % what
    return o


def _judge_stem3(what, o, c, B, fmt):
    ref = c['ref'][:B]
    err = (o - ref).abs().max().item()
    mx = ref.abs().max().item()
    if fmt == 'h2':
        print('%s: max-abs err %.3e (bound 3e-5; ref absmax %.2f)' % (what, err, mx))
        assert err < 3e-5, (what, err)
    else:
        bound = SC.f32_bound(c['err_cpu'], mx)
        print('%s: err %.3e of max |ref| (float32 CPU %.3e, bound %.3e; ref absmax %.2f)' % (what, err / mx, c['err_cpu'], bound, mx))
        assert err / mx <= bound, (what, err / mx, bound)


@pytest.mark.parametrize('H,W,B,kernel,fmt', SC.STEM3, ids=lambda v: str(v))
def test_stem3(dev, H, W, B, kernel, fmt):
    """stem_mfma_kernel and stem_conv_kernel (ROMP_OPF_STEM_VALU; H2 and float32 output) on one tile with all four borders, one tile
    row and one tile column, against conv2d in float64."""
    c = SC.stem3_case(H, W)
    _judge_stem3('stem %s %s B=%d %dx%d' % (kernel, fmt, B, H, W), _run_stem3(dev, c, H, W, B, kernel, fmt), c, B, fmt)


def test_stem3_into_a_wider_tensor(dev):
    """The float32 form at out_cstride = 96, out_coff = 16: the other 32 channels of every pixel keep the sentinel."""
    H, W, B, cs, co = SC.STEM3_WIDE
    c = SC.stem3_case(H, W)
    _judge_stem3('stem valu f32 B=%d %dx%d cstride %d coff %d' % (B, H, W, cs, co), _run_stem3(dev, c, H, W, B, 'valu', 'f32', cs, co), c, B, 'f32')


@pytest.mark.parametrize('H,W', SC.STEM3_SIZES)
@pytest.mark.parametrize('frame', SC.CONST_FRAMES)
def test_stem3_constant_frames(dev, frame, H, W):
    """All-0 and all-255 frames: every tap is exactly -1 / +1 in the fp16 pieces, and a kernel that pads before it normalises reads
    -1 where the padding's 0 belongs, at every border pixel."""
    c = SC.stem3_case(H, W, frame)
    for kernel, fmt in SC.STEM3_FORMS:
        _judge_stem3('stem %s %s %dx%d frame %g' % (kernel, fmt, H, W, frame), _run_stem3(dev, c, H, W, 1, kernel, fmt), c, 1, fmt)


# ------------------------------------------------------------------------------ the 7x7 stem alone
@pytest.mark.parametrize('H,W,B', SC.STEM7)
def test_stem7_alone(dev, H, W, B):
    """stem7_conv_kernel (ROMP_OP_STEM7, float32) as a one-op net between caller pointers: every pixel of m, not only the maxima
    that survive the pool."""
    c = SC.stem7_case(H, W)
    P, op = SC.stem7_alone(dev, c, H, W)
    img = c['img'][:B].contiguous()
    xg = _guard_in(dev, img, 32 * W * 3)
    og = _guard_out(dev, (B, H // 2, W // 2, 64), 32 * (W // 2) * 64)
    with OneOpNet(dev, [op], [], B) as net:
        net.forward(xg.inner, B, og.inner)
    what = 'stem7 B=%d %dx%d' % (B, H, W)
    _check_guards(what, og, (xg, img))
    o = og.inner.cpu()
    assert not bool(torch.isnan(o).any()), '%s left NaN' % what
    ref = c['m'][:B]
    mx = ref.abs().max().item()
    err, bound = (o - ref).abs().max().item() / mx, SC.f32_bound(c['err_cpu'], mx)
    print('%s: err %.3e of max |ref| (float32 CPU %.3e, bound %.3e; ref absmax %.2f)' % (what, err, c['err_cpu'], bound, mx))
    assert err <= bound, (what, err, bound)


# ------------------------------------------------------------------------------ the max-pool alone
def _run_pool(dev, x, Cc, out_cs):
    """x: (B, H, W, in_cstride) with the map in channels 0 .. C - 1 -> (B, H/2, W/2, out_cstride) as the kernel left it."""
    B, H, W, in_cs = x.shape
    op = SC.pool_op(H, W, Cc, in_cs, out_cs)
    xg = _guard_in(dev, x, 32 * W * in_cs, POS_INF)
    og = _guard_out(dev, (B, H // 2, W // 2, out_cs), 32 * (W // 2) * out_cs, sentinel_inside=out_cs != Cc)
    with OneOpNet(dev, [op], [], B) as net:
        net.forward(xg.inner, B, og.inner)
    _check_guards('maxpool %dx%dx%d' % (H, W, Cc), og, (xg, x))
    return og.inner.cpu()


@pytest.mark.parametrize('H,W,Cc,in_cs,out_cs', SC.POOL)
def test_maxpool_alone(dev, H, W, Cc, in_cs, out_cs):
    """maxpool3s2_kernel (ROMP_OP_MAXPOOL as a one-op net) on maps down to 2 x 2, with negative values, an all-negative map (the
    answer is the negative maximum: padding is -inf, not 0) and infinities: bit for bit.  NaN inputs are out of scope -- fmaxf drops
    them, torch hands them on, and nothing upstream can produce one behind the kernel's own ReLU: neither behaviour is pinned."""
    B = 3
    for kind in SC.POOL_INPUTS:
        x = SC.pool_input(B, H, W, Cc, kind)
        ref = SC.pool_reference(x)
        xin = x
        if in_cs != Cc:                                   # the map as a channel slice of a wider tensor of +inf decoys
            xin = torch.full((B, H, W, in_cs), float('inf'))
            xin[..., :Cc] = x
        o = _run_pool(dev, xin, Cc, out_cs)
        if out_cs != Cc:
            assert _is_sentinel(o[..., Cc:]), 'the pool wrote channels outside its slice'
            o = o[..., :Cc].contiguous()
        assert not bool(torch.isnan(o).any())
        same = torch.equal(o.view(torch.int32), ref.view(torch.int32))
        print('maxpool %dx%dx%d (cstride %d -> %d) %s: %s' % (H, W, Cc, in_cs, out_cs, kind, 'bit-equal' if same else 'DIFFERS at %d elements' % int((o.view(torch.int32) != ref.view(torch.int32)).sum())))
        assert same, (H, W, Cc, kind)


def test_maxpool_grid_stride_loop(dev):
    """A map whose output has more float4 items than 16384 workgroups x 256 threads: the second pass of the kernel's grid-stride
    loop writes the last rows.  Bit for bit."""
    B, H, W, Cc = SC.pool_big_shape()
    assert B * (H // 2) * (W // 2) * (Cc // 4) > SC.POOL_GRID_CAP * SC.POOL_THREADS
    x = SC.pool_input(B, H, W, Cc, 'normal')
    ref = SC.pool_reference(x)
    o = _run_pool(dev, x, Cc, Cc)
    same = torch.equal(o.view(torch.int32), ref.view(torch.int32))
    print('maxpool %dx%dx%d, %d float4 items on a grid of %d x %d: %s' % (H, W, Cc, ref.numel() // 4, SC.POOL_GRID_CAP, SC.POOL_THREADS, 'bit-equal' if same else 'DIFFERS'))
    assert same


# ------------------------------------------------------------------------------ the split-K tail alone
def _run_ksum(dev, c, B, H, W, Cc, G, relu, rf, res, fmt, consts, res_cs=None, res_coff=0, out_cs=None, out_coff=0):
    """-> (output (B, H, W, C) float32, reference, err_cpu), guards checked."""
    from romp_amd.plan import encode_h2, decode_h2
    res_cs, out_cs = res_cs or Cc, out_cs or Cc
    op = SC.ksum_op(H, W, Cc, G, relu, rf, res, fmt, consts[0].data_ptr(), consts[1].data_ptr(), res_cs, res_coff, out_cs, out_coff)
    part = c['part'].reshape(B, H, W, G * Cc)
    pg = _guard_in(dev, part, 32 * W * G * Cc)
    og = _guard_out(dev, (B, H, W, out_cs), 32 * W * out_cs, sentinel_inside=out_cs != Cc)
    what = 'ksum %dx%dx%d G=%d relu %d from %d res %s out %s' % (H, W, Cc, G, relu, rf, res, fmt)
    with OneOpNet(dev, [op], [H * W * res_cs] if res != 'none' else [], B + 1) as net:
        if res != 'none':
            r = torch.full((B + 1, H, W, res_cs), float('nan'))             # decoy channels and the spare image: NaN (as fp16 pieces too)
            r[:B, ..., res_coff:res_coff + Cc] = c['res']
            net.write(0, encode_h2(r) if res == 'h2' else r)
        net.forward(pg.inner, B, og.inner)
    _check_guards(what, og, (pg, part))
    o = og.inner.cpu()
    if out_cs != Cc:
        assert _is_sentinel(o[..., :out_coff]) and _is_sentinel(o[..., out_coff + Cc:]), '%s wrote channels outside its slice' % what
        o = o[..., out_coff:out_coff + Cc].contiguous()
    if fmt == 'h2':
        o = decode_h2(o)
    assert not bool(torch.isnan(o).any()), '%s left NaN' % what
    ref, err_cpu = SC.ksum_reference(c, relu, rf, res)
    mx = ref.abs().max().item()
    err = (o - ref).abs().max().item() / mx
    bound = SC.f32_bound(err_cpu, mx, 4) + (SC.h2_quantum(mx) / mx if fmt == 'h2' else 0.0)
    print('%s: err %.3e of max |ref| (float32 CPU %.3e, bound %.3e)' % (what, err, err_cpu, bound))
    assert err <= bound, (what, err, bound)
    return err


def _ksum_consts(dev, c):
    return [c['scale'].to(dev).contiguous(), c['shift'].to(dev).contiguous()]


@pytest.mark.parametrize('H,W,Cc,G', SC.KSUM_SHAPES)
def test_ksum_alone(dev, H, W, Cc, G):
    """ksum_kernel (ROMP_OP_KSUM as a one-op net): G = 1, exactly one eight-slice round, one slice past one and past two rounds, a
    short round; without ReLU and with ReLU from channel 0, 8 and C - 8 on; no residual, a float32 one, an H2 one; both output formats.
    Reference: the float32 slices summed in order in float64."""
    B = SC.KSUM_B
    c = SC.ksum_case(B, H, W, Cc, G)
    consts = _ksum_consts(dev, c)
    worst = 0.0
    for relu, rf, res, fmt in SC.ksum_configs((H, W, Cc, G)):
        worst = max(worst, _run_ksum(dev, c, B, H, W, Cc, G, relu, rf, res, fmt, consts))
    print('ksum %dx%dx%d G=%d: worst err %.3e of max |ref|' % (H, W, Cc, G, worst))


@pytest.mark.parametrize('fmt', SC.KSUM_FMTS)
def test_ksum_channel_slices(dev, fmt):
    """The residual read at res_coff = 8 of a wider H2 tensor, the result written at out_coff = 8 of a wider tensor: the other channels
    of every pixel keep the sentinel, the residual's decoy channels (NaN) are not read."""
    (H, W, Cc, G), rf, res, rco, rcs, oco, ocs = SC.KSUM_WIDE
    B = SC.KSUM_B
    c = SC.ksum_case(B, H, W, Cc, G)
    _run_ksum(dev, c, B, H, W, Cc, G, 1, rf, res, fmt, _ksum_consts(dev, c), rcs, rco, ocs, oco)


def test_ksum_grid_stride_loop(dev):
    """More octet items than 4096 workgroups x 256 threads: the second pass of the kernel's grid-stride loop writes the last rows."""
    B, H, W, Cc, G = SC.ksum_big_shape()
    assert B * H * W * Cc // 8 > SC.KSUM_GRID_CAP * SC.KSUM_THREADS
    c = SC.ksum_case(B, H, W, Cc, G)
    _run_ksum(dev, c, B, H, W, Cc, G, 1, 0, 'f32', 'f32', _ksum_consts(dev, c))


# ------------------------------------------------------------------------------ the fused stems
def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _run_stem_net(dev, P, ops, act, img, B, fmt, what):
    """A lowered stem program on B images of a guarded image inside a net made for B + 1: -> the tensor `act` (B, h, w, 64) float32.
    The output buffer is pre-filled with the sentinel; image B + 1 must keep it."""
    from romp_amd.plan import decode_h2
    n1 = P.buf_floats[act.buf]
    assert n1 == act.H * act.W * 64
    xg = _guard_in(dev, img, 32 * img.shape[2] * 3)
    with OneOpNet(dev, ops, P.buf_floats, B + 1) as net:
        net.write(act.buf, torch.full(((B + 1) * n1,), SENTINEL, dtype=torch.int32).view(torch.float32))
        net.forward(xg.inner, B)
        out = net.read(act.buf, B + 1, (B + 1) * n1)
    assert _is_sentinel(out[B * n1:]), '%s wrote beyond its %d images' % (what, B)
    assert xg.bands_intact() and torch.equal(xg.inner.cpu(), img), '%s changed its input' % what
    o = out[:B * n1].reshape(B, act.H, act.W, 64)
    assert not _is_sentinel(o[..., :8]) and not bool((o.view(torch.int32) == SENTINEL).all(-1).any()), '%s left pixels unwritten' % what
    if fmt == 'h2':
        o = decode_h2(o)
    assert not bool(torch.isnan(o).any()), '%s left NaN' % what
    return o


def _stem2(dev, B, H, W, monkeypatch):
    from romp_amd import lib as L
    c = SC.stem2_case(H, W)
    img, ref = c['img'][:B].contiguous(), c['ref'][:B]
    mx = ref.abs().max().item()
    outs = {}
    for fuse in ('1', '0'):
        monkeypatch.setenv('ROMP_FUSE_STEM2', fuse)
        P, ops, b = SC.lower_stem2(dev, c, H, W)
        assert P.fused_stem2 == int(fuse) and [o.kind for o in P.ops[:2]] == ([L.OP_NOP, L.OP_STEM2] if fuse == '1' else [L.OP_STEM, L.OP_CONV])
        assert P.ops[1].out_fmt == L.FMT_H2
        what = 'stem2 fuse=%s B=%d %dx%d' % (fuse, B, H, W)
        outs[fuse] = _run_stem_net(dev, P, ops, b, img, B, 'h2', what)
        err = (outs[fuse] - ref).abs().max().item() / mx
        print('%s: err %.3e of max |ref| (bound 3e-5; ref absmax %.2f)' % (what, err, mx))
        assert err < 3e-5, (what, err)
    d = (outs['1'] - outs['0']).abs().max().item()
    print('stem2 B=%d %dx%d: fused against the two launches %.3e (bound %.3e)' % (B, H, W, d, 2e-5 * max(1.0, mx)))
    assert d < 2e-5 * max(1.0, mx), d


@pytest.mark.parametrize('B,H,W', SC.STEM2)
def test_stem2(dev, B, H, W, monkeypatch):
    """stem2_kernel on one tile column, three tile columns and one tile column of twelve rows, against float64, and against the
    ROMP_FUSE_STEM2=0 lowering of the same program."""
    _stem2(dev, B, H, W, monkeypatch)


def test_stem2_partial_last_round(dev, monkeypatch):
    """More tiles than the persistent grid and no multiple of it: in the last round only some workgroups still have a tile, and the
    next-tile halo prefetch of the others has to stop (on 256 CUs: B = 3 at 320 x 384, 360 tiles = 256 + 104)."""
    (B, H, W), tiles, grid = SC.partial_round('stem2', _cus(dev))
    print('stem2 partial round: %d CUs, B=%d %dx%d: %d tiles on a grid of %d' % (_cus(dev), B, H, W, tiles, grid))
    assert tiles == B * (H // 16) * (W // 64) and grid == min(tiles, _cus(dev))
    assert tiles > grid and tiles % grid != 0
    _stem2(dev, B, H, W, monkeypatch)


def _stem7p(dev, B, H, W, monkeypatch):
    from romp_amd import lib as L
    c = SC.stem7_case(H, W)
    img, ref = c['img'][:B].contiguous(), c['pooled'][:B]
    mx = ref.abs().max().item()
    outs = {}
    for fmt in ('h2', 'f32'):
        monkeypatch.delenv('ROMP_STEM', raising=False)
        P, ops, y = SC.lower_stem7(dev, c, H, W, fmt)
        assert P.fused_stem7p == 1 and [o.kind for o in P.ops] == [L.OP_NOP, L.OP_STEM7P]
        assert P.ops[1].out_fmt == (L.FMT_H2 if fmt == 'h2' else L.FMT_F32)
        what = 'stem7p %s B=%d %dx%d' % (fmt, B, H, W)
        outs[fmt] = _run_stem_net(dev, P, ops, y, img, B, fmt, what)
        err = (outs[fmt] - ref).abs().max().item() / mx
        print('%s: err %.3e of max |ref| (bound 2e-5; ref absmax %.2f)' % (what, err, mx))
        assert err < 2e-5, (what, err)
    # the float32 pair on the same images: its m is compared at every pixel by test_stem7_alone, its pool bit for bit by
    # test_maxpool_alone; the fused kernel's pooled output must agree with the pooled pair
    monkeypatch.setenv('ROMP_STEM', 'valu')
    P, ops, y = SC.lower_stem7(dev, c, H, W, 'f32')
    assert P.fused_stem7p == 0 and [o.kind for o in P.ops] == [L.OP_STEM7, L.OP_MAXPOOL] and P.ops[1].out_fmt == L.FMT_F32
    what = 'stem7 + maxpool B=%d %dx%d' % (B, H, W)
    pair = _run_stem_net(dev, P, ops, y, img, B, 'f32', what)
    err = (pair - ref).abs().max().item() / mx
    bound = SC.f32_bound(c['err_cpu'], mx)
    print('%s: err %.3e of max |ref| (float32 CPU, of m: %.3e, bound %.3e)' % (what, err, c['err_cpu'], bound))
    assert err <= bound, (what, err, bound)
    for fmt in ('h2', 'f32'):
        d = (outs[fmt] - pair).abs().max().item()
        print('stem7p %s B=%d %dx%d: fused against the pair %.3e (bound %.3e)' % (fmt, B, H, W, d, 2e-5 * max(1.0, mx)))
        assert d < 2e-5 * max(1.0, mx), (fmt, d)


@pytest.mark.parametrize('B,H,W', SC.STEM7P)
def test_stem7p(dev, B, H, W, monkeypatch):
    """stem7p_kernel in both output formats on two tile rows of one tile, of two tiles, and six tile rows, against float64, and
    against the [STEM7, MAXPOOL] pair (ROMP_STEM=valu) on the same images."""
    _stem7p(dev, B, H, W, monkeypatch)


def test_stem7p_partial_last_round(dev, monkeypatch):
    """More tiles than the persistent grid of two workgroups per CU and no multiple of it (on 256 CUs: B = 3 at 320 x 384, 720 tiles =
    512 + 208): the last round's idle workgroups fetch no further halo."""
    (B, H, W), tiles, grid = SC.partial_round('stem7p', _cus(dev))
    print('stem7p partial round: %d CUs, B=%d %dx%d: %d tiles on a grid of %d' % (_cus(dev), B, H, W, tiles, grid))
    assert tiles == B * (H // 16) * (W // 32) and grid == min(tiles, 2 * _cus(dev))
    assert tiles > grid and tiles % grid != 0
    _stem7p(dev, B, H, W, monkeypatch)
