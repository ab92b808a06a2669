"""Case tables and float64 references for the kernels that read the image first, and for the two small kernels that only ever ran
inside whole networks (a helper, not a conftest): csrc/stem_fuse.hip (stem_conv_kernel, stem_mfma_kernel, stem7_conv_kernel,
maxpool3s2_kernel, ksum_kernel), csrc/stem2.hip, csrc/stem7p.hip.  tests/test_stem_cases.py shows without a device that the tables are
not vacuous, tests/test_gpu_stem_edges.py runs them on the kernels.

Every reference is F.conv2d / F.max_pool2d / a plain sum in float64 on the CPU, rounded to float32 once; inputs are seeded.  The
normalisation is written as the models write it -- x / 255 * 2 - 1 (HRNet), (x / 255 - mean) / std (ResNet-50) -- and conv2d's zero
padding comes after it.  Images are integer-valued floats in 0..255.  The BatchNorm shift of every stem layer is chosen from the
layer's own pre-activations (their per-channel median, plus a little noise) so that about half of the pre-ReLU values are positive:
the ReLU neither hides the conv nor goes untested (`share`, asserted to lie in 0.3 .. 0.7 by test_stem_cases.py for every case).

Next to each float64 reference stands the SAME layer in float32 torch on the CPU: `err_cpu`, its max-abs error against float64 over
max |ref|, is the yardstick of the float32 kernels (test_gpu_smpl_grad.py's: a kernel may be 8 x as far from float64 as float32 torch
is -- three bits for another summation order, nothing else).  The references are shared between tests: treat them as read-only."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

ACT_SHIFT = 4
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BATCHES = (1, 3)                      # every reference is built for 3 images; B = 1 takes the first
SHARE = (0.3, 0.7)

# ------------------------------------------------------------------------------------------------------------------ tables
# 3x3 stem (16 x 16 output tiles): one tile with all four borders in it, one tile row, one tile column
STEM3_SIZES = [(32, 32), (32, 96), (96, 32)]
STEM3_FORMS = [('mfma', 'h2'), ('valu', 'h2'), ('valu', 'f32')]                # (kernel, output format); the MFMA kernel writes H2 only
STEM3 = [(H, W, B, k, f) for (H, W) in STEM3_SIZES for B in BATCHES for (k, f) in STEM3_FORMS]
STEM3_WIDE = (32, 96, 3, 96, 16)      # H, W, B, out_cstride, out_coff: the float32 form into a wider tensor
CONST_FRAMES = (0.0, 255.0)           # x / 255 * 2 - 1 = -1 / +1: exact in the fp16 pieces
STEM7 = [(H, W, B) for (H, W) in STEM3_SIZES for B in BATCHES]

# max-pool: (H, W, C, in_cstride, out_cstride); the last one reads and writes slices of wider tensors
POOL_MAPS = [(2, 2), (2, 6), (6, 2), (16, 48), (48, 16)]
POOL = [(H, W, Cc, Cc, Cc) for (H, W) in POOL_MAPS for Cc in (4, 64)] + [(16, 48, 4, 12, 8)]
POOL_INPUTS = ('normal', 'negative', 'inf')
POOL_GRID_CAP, POOL_THREADS = 16384, 256                                       # launch_maxpool: float4 items beyond cap x threads take the grid-stride loop


def pool_big_shape():
    """-> (B, H, W, C) of the smallest map of 2048 output columns x 4 channels whose output has more float4 items than one pass of the
    capped grid (computed from the launcher's cap).  Input: 269 MB."""
    Wo, Cc = 2048, 4
    Ho = POOL_GRID_CAP * POOL_THREADS // (Wo * Cc // 4) + 2
    return 1, 2 * Ho, 2 * Wo, Cc


# fused stems: (B, H, W).  stem2: 4 x 16 output tiles of y = image / 4, i.e. 16 x 64 image pixels; stem7p: 4 x 8 pooled pixels, i.e.
# 16 x 32 image pixels.  The last entry of each is the partial-round case on 256 CUs (partial_round()).
STEM2 = [(B, H, W) for (H, W) in [(64, 64), (64, 192), (192, 64)] for B in BATCHES]
STEM7P = [(1, 32, 32), (3, 32, 32), (3, 32, 64), (3, 96, 32)]
PARTIAL_CANDIDATES = [(3, 320, 384), (3, 192, 256), (3, 512, 512), (2, 320, 384)]


def stem2_tiles(B, H, W):
    return B * (H // 16) * (W // 64)


def stem7p_tiles(B, H, W):
    return B * (H // 16) * (W // 32)


def partial_round(kind, cus):
    """-> ((B, H, W), tiles, grid): the first candidate whose tiles need more than one round of the persistent grid and leave a last
    round in which only some workgroups still have a tile (the next-tile prefetch has to stop there)."""
    for c in PARTIAL_CANDIDATES:
        tiles = stem2_tiles(*c) if kind == 'stem2' else stem7p_tiles(*c)
        grid = min(tiles, cus if kind == 'stem2' else 2 * cus)
        if tiles > grid and tiles % grid:
            return c, tiles, grid
    raise AssertionError('no candidate has a partial last round on %d CUs' % cus)


# split-K tail: partials of (H, W, C, G).  G = 1: the `g0 + g == 0` path alone; 8: exactly one round of the eight-slice loop; 9 and
# 17: one slice past one and past two rounds; 7: a short round
KSUM_SHAPES = [(3, 5, 8, 1), (4, 24, 64, 8), (5, 8, 32, 9), (2, 6, 16, 17), (4, 8, 64, 7)]
KSUM_RES = ('none', 'f32', 'h2')
KSUM_FMTS = ('f32', 'h2')
KSUM_WIDE = ((5, 8, 32, 9), 8, 'h2', 8, 48, 8, 48)      # shape, relu_from, residual, res_coff, res_cstride, out_coff, out_cstride
KSUM_GRID_CAP, KSUM_THREADS = 4096, 256                  # launch_ksum: octet items beyond cap x threads take the grid-stride loop
KSUM_B = 3


def ksum_relus(Cc):
    """(relu, relu_from) settings of a shape: no ReLU, then ReLU from channel 0, 8 and C - 8 on (without duplicates)."""
    return [(0, 0)] + [(1, f) for f in sorted({0, 8, Cc - 8}) if f <= Cc]


def ksum_configs(shape):
    return [(relu, rf, res, fmt) for (relu, rf) in ksum_relus(shape[2]) for res in KSUM_RES for fmt in KSUM_FMTS]


def ksum_big_shape():
    """-> (B, H, W, C, G): more octet items than one pass of the capped grid (from the launcher's cap); partials: 67 MB."""
    Wd, Cc = 1024, 8
    Hh = KSUM_GRID_CAP * KSUM_THREADS // (Wd * Cc // 8) + 2
    return 1, Hh, Wd, Cc, 2


# ------------------------------------------------------------------------------------------------------------------ references
def normalise_hrnet(img):
    return img.double() / 255.0 * 2.0 - 1.0


def normalise_resnet(img):
    return (img.double() / 255.0 - torch.tensor(MEAN, dtype=torch.float64)) / torch.tensor(STD, dtype=torch.float64)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _bn(y, scale, shift):
    return y * scale.to(y.dtype).view(1, -1, 1, 1) + shift.to(y.dtype).view(1, -1, 1, 1)


def _balanced_shift(y, scale, g):
    """y: (B, C, H, W) float64 conv outputs -> the float32 shift that puts each channel's median pre-activation near 0."""
    Cc = y.shape[1]
    med = (y * scale.double().view(1, -1, 1, 1)).permute(1, 0, 2, 3).reshape(Cc, -1).median(1).values
    return (-med + 0.05 * torch.randn(Cc, generator=g).double()).float()


def _share(pre):
    return float((pre > 0).double().mean())


def _rel(a, ref64):
    return float((a.double() - ref64).abs().max() / ref64.abs().max())


def _images(g, H, W):
    return torch.randint(0, 256, (3, H, W, 3), generator=g).float()


@functools.lru_cache(maxsize=None)
def stem3_case(H, W, frame=None):
    """The 3x3 stride-2 3 -> 64 stem + BN + ReLU on 3 images of H x W.  frame: None (random pixels) or a constant pixel value (same
    layer constants as the random frame of the size).  -> dict(img, w, scale, shift, ref (3, H/2, W/2, 64), err_cpu, share)."""
    g = torch.Generator().manual_seed(1000 * H + W)
    img = _images(g, H, W)
    w = torch.randn(64, 3, 3, 3, generator=g) * 0.3
    scale = torch.rand(64, generator=g) + 0.5
    shift = _balanced_shift(F.conv2d(_nchw(normalise_hrnet(img)), w.double(), None, stride=2, padding=1), scale, g)
    if frame is not None:
        img = torch.full((3, H, W, 3), float(frame))
    pre = _bn(F.conv2d(_nchw(normalise_hrnet(img)), w.double(), None, stride=2, padding=1), scale, shift)
    ref64 = torch.relu(pre).permute(0, 2, 3, 1)
    cpu = torch.relu(_bn(F.conv2d(_nchw(img / 255.0 * 2.0 - 1.0), w, None, stride=2, padding=1), scale, shift)).permute(0, 2, 3, 1)
    return dict(img=img, w=w, scale=scale, shift=shift, ref=ref64.float().contiguous(), err_cpu=_rel(cpu, ref64), share=_share(pre))


@functools.lru_cache(maxsize=None)
def stem7_case(H, W):
    """ResNet-50's stem: ImageNet normalisation, conv 7x7 s2 p3 3 -> 64, BN, ReLU (`m`, every pixel), then MaxPool2d(3, 2, 1)
    (`pooled`).  -> dict(img, w, scale, shift, m (3, H/2, W/2, 64), pooled (3, H/4, W/4, 64), err_cpu (of m), share)."""
    g = torch.Generator().manual_seed(7000 * H + W)
    img = _images(g, H, W)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.08
    scale = torch.rand(64, generator=g) + 0.5
    y = F.conv2d(_nchw(normalise_resnet(img)), w.double(), None, stride=2, padding=3)
    shift = _balanced_shift(y, scale, g)
    pre = _bn(y, scale, shift)
    m64 = torch.relu(pre)
    x32 = (img / 255.0 - torch.tensor(MEAN)) / torch.tensor(STD)
    cpu = torch.relu(_bn(F.conv2d(_nchw(x32), w, None, stride=2, padding=3), scale, shift))
    return dict(img=img, w=w, scale=scale, shift=shift, m=m64.permute(0, 2, 3, 1).float().contiguous(),
                pooled=F.max_pool2d(m64, 3, 2, 1).permute(0, 2, 3, 1).float().contiguous(), err_cpu=_rel(cpu, m64), share=_share(pre))


@functools.lru_cache(maxsize=None)
def stem2_case(H, W):
    """HRNet's stem and conv2: x / 255 * 2 - 1, conv 3x3 s2 3 -> 64 + BN + ReLU, conv 3x3 s2 64 -> 64 + BN + ReLU (zero padding of both
    convs at the borders).  w[2] / scale[2] / shift[2]: the 1x1 reader that keeps conv2's output an H2 tensor with a consumer.
    -> dict(img, w [3], scale [3], shift [3], ref (3, H/4, W/4, 64), share (of both layers))."""
    g = torch.Generator().manual_seed(2000 * H + W)
    img = _images(g, H, W)
    w = [torch.randn(64, 3, 3, 3, generator=g) * 0.3, torch.randn(64, 64, 3, 3, generator=g) / (64 * 9) ** 0.5,
         torch.randn(64, 64, 1, 1, generator=g) / 8.0]
    scale = [torch.rand(64, generator=g) + 0.5 for _ in range(3)]
    y1 = F.conv2d(_nchw(normalise_hrnet(img)), w[0].double(), None, stride=2, padding=1)
    sh0 = _balanced_shift(y1, scale[0], g)
    pre1 = _bn(y1, scale[0], sh0)
    y2 = F.conv2d(torch.relu(pre1), w[1].double(), None, stride=2, padding=1)
    sh1 = _balanced_shift(y2, scale[1], g)
    pre2 = _bn(y2, scale[1], sh1)
    shift = [sh0, sh1, torch.randn(64, generator=g) * 0.2]
    return dict(img=img, w=w, scale=scale, shift=shift, ref=torch.relu(pre2).permute(0, 2, 3, 1).float().contiguous(),
                share=(_share(pre1), _share(pre2)))


def pool_input(B, H, W, Cc, kind, seed=0):
    """NHWC float32 map: standard normal; all negative (the answer is the negative maximum, never 0); or normal with a tenth of the
    entries -inf and a tenth +inf.  (NaN inputs are out of scope: fmaxf drops them, torch hands them on, nothing upstream makes one.)"""
    g = torch.Generator().manual_seed(97 * H + 13 * W + Cc + seed)
    x = torch.randn(B, H, W, Cc, generator=g)
    if kind == 'negative':
        x = -x.abs() - 0.5
    elif kind == 'inf':
        u = torch.rand(B, H, W, Cc, generator=g)
        x = torch.where(u < 0.1, torch.full_like(x, -float('inf')), torch.where(u > 0.9, torch.full_like(x, float('inf')), x))
    else:
        assert kind == 'normal', kind
    return x


def pool_reference(x):
    """MaxPool2d(3, 2, 1) of an NHWC float32 map in float64 (padding -inf, as torch); exact, so the kernel must match it bit for bit."""
    return F.max_pool2d(_nchw(x.double()), 3, 2, 1).permute(0, 2, 3, 1).float().contiguous()


def pool_by_hand(x):
    """The same as a hand-written loop (small maps only)."""
    B, H, W, Cc = x.shape
    out = torch.full((B, H // 2, W // 2, Cc), -float('inf'))
    for b in range(B):
        for oy in range(H // 2):
            for ox in range(W // 2):
                for c in range(Cc):
                    m = -float('inf')
                    for iy in range(2 * oy - 1, 2 * oy + 2):
                        for ix in range(2 * ox - 1, 2 * ox + 2):
                            if 0 <= iy < H and 0 <= ix < W:
                                m = max(m, float(x[b, iy, ix, c]))
                    out[b, oy, ox, c] = m
    return out


def h2_value(x):
    """The value an H2 tensor holds for x (plan.encode_h2: fp16 pieces h1 + h2 of x * 2^ACT_SHIFT), in float64."""
    xs = x.float() * 2.0 ** ACT_SHIFT
    h1 = xs.half()
    h2 = (xs - h1.float()).half()
    return (h1.double() + h2.double()) * 2.0 ** -ACT_SHIFT


def h2_quantum(maxabs):
    """Largest error of storing |v| <= maxabs as H2: the low piece keeps 11 bits below the high piece's 11 (2^-22 relative), down to
    the fp16 subnormal step of the scaled value (half of 2^-24, over 2^ACT_SHIFT)."""
    return 2.0 ** -22 * maxabs + 2.0 ** (-25 - ACT_SHIFT)


@functools.lru_cache(maxsize=8)
def ksum_case(B, H, W, Cc, G):
    """Partial sums (B, H, W, G, C) whose slices all have different magnitudes (0.5 + 0.37 g: the last is the largest, a dropped or a
    doubled slice shows), the layer's scale and shift, and a residual (B, H, W, C)."""
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + Cc + G)
    mag = 0.5 + 0.37 * torch.arange(G, dtype=torch.float32)
    assert len(set(mag.tolist())) == G and float(mag[-1]) >= float(mag.max())
    part = torch.randn(B, H, W, G, Cc, generator=g) * mag.view(1, 1, 1, G, 1)
    return dict(part=part, scale=torch.rand(Cc, generator=g) + 0.5, shift=torch.randn(Cc, generator=g) * 0.3,
                res=torch.randn(B, H, W, Cc, generator=g), mag=mag)


def ksum_reference(c, relu, relu_from, res):
    """The float32 slices summed in order in float64, then scale, shift, residual ('none' / 'f32' / 'h2': the values the H2 tensor
    holds), ReLU on channels >= relu_from.  -> (ref float32, err_cpu: the same in float32 against it, over max |ref|)."""
    part = c['part']
    G = part.shape[3]
    acc64, acc32 = part[..., 0, :].double(), part[..., 0, :].clone()
    for k in range(1, G):
        acc64 = acc64 + part[..., k, :].double()
        acc32 = acc32 + part[..., k, :]
    v64 = acc64 * c['scale'].double() + c['shift'].double()
    v32 = acc32 * c['scale'] + c['shift']
    if res != 'none':
        r64 = c['res'].double() if res == 'f32' else h2_value(c['res'])
        v64, v32 = v64 + r64, v32 + r64.float()
    if relu:
        v64 = torch.cat([v64[..., :relu_from], torch.relu(v64[..., relu_from:])], -1)
        v32 = torch.cat([v32[..., :relu_from], torch.relu(v32[..., relu_from:])], -1)
    return v64.float().contiguous(), _rel(v32, v64)


def f32_bound(err_cpu, maxabs, floor_ulps=0):
    """Relative bound of a float32 kernel: 8 x the float32 CPU error, not below `floor_ulps` float32 ulps of max |ref| (over max |ref|)."""
    return max(8.0 * err_cpu, floor_ulps * float(np.spacing(np.float32(maxabs))) / maxabs)


# ------------------------------------------------------------------------------------------------------------------ lowering
def lower_stem3(dev, c, H, W, kernel, fmt, out_cstride=64, out_coff=0):
    """-> (program, its one ROMP_OP_STEM op) for romp_conv_forward: the MFMA kernel (H2 only) or the float32 VALU kernel."""
    from romp_amd import lib as L
    from romp_amd.plan import Program, set_conv_math
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    P.stem('stem', c['w'], c['scale'], c['shift'], H, W)
    op = P.ops[0]
    assert not (op.flags & L.OPF_STEM_VALU), 'ordinary weights take the MFMA stem'
    op.out_fmt, op.act_shift = (L.FMT_H2 if fmt == 'h2' else L.FMT_F32), ACT_SHIFT
    op.out_cstride, op.out_coff = out_cstride, out_coff
    if kernel == 'valu':
        op.flags |= L.OPF_STEM_VALU
    assert kernel == 'valu' or fmt == 'h2'
    return P, op


def lower_stem2(dev, c, H, W):
    """HRNet's stem + conv2 + a 1x1 reader, lowered (env ROMP_FUSE_STEM2 decides: [NOP, STEM2, CONV] or [STEM, CONV, CONV]).
    -> (program, op array, conv2's output activation)."""
    from romp_amd.plan import Program, set_conv_math
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    a = P.stem('stem.conv1', c['w'][0], c['scale'][0], c['shift'][0], H, W)
    b = P.conv('stem.conv2', a, [c['w'][1]], [c['scale'][1]], [c['shift'][1]], 3, 2, True)
    P.conv('reader', b, [c['w'][2]], [c['scale'][2]], [c['shift'][2]], 1, 1, True)
    return P, P.op_array(), b


def lower_stem7(dev, c, H, W, fmt):
    """ResNet-50's stem conv + max-pool, lowered (env ROMP_STEM=valu keeps the float32 pair [STEM7, MAXPOOL]; else [NOP, STEM7P]).
    fmt 'f32': the pooled tensor is one the host reads.  -> (program, op array, the pooled activation)."""
    from romp_amd.plan import Program, set_conv_math
    from romp_amd.resnet_plan import _stem7, _maxpool
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    y = _maxpool(P, 'pool', _stem7(P, 'stem', c['w'], c['scale'], c['shift'], H, W))
    if fmt == 'f32':
        P.exported_bufs.add(y.buf)
    return P, P.op_array(), y


def stem7_alone(dev, c, H, W):
    """-> (program, ROMP_OP_STEM7 from the caller's image pointer to the caller's output pointer): a one-op net."""
    from romp_amd import lib as L
    from romp_amd.plan import Program, set_conv_math
    from romp_amd.resnet_plan import _stem7
    P = Program(dev)
    set_conv_math(P, 'f32')
    _stem7(P, 'stem', c['w'], c['scale'], c['shift'], H, W)
    op = P.ops[0]
    assert op.kind == L.OP_STEM7 and op.in_buf == L.BUF_IMAGE
    op.out_buf = L.BUF_CENTER
    return P, op


def pool_op(H, W, Cc, in_cs, out_cs):
    """ROMP_OP_MAXPOOL from the caller's image pointer to the caller's output pointer."""
    from romp_amd import lib as L
    op = L.RompOp()
    op.kind, op.in_buf, op.res_buf, op.out_buf = L.OP_MAXPOOL, L.BUF_IMAGE, L.BUF_NONE, L.BUF_CENTER
    op.H, op.W, op.Cin, op.Cout, op.ksize, op.stride = H, W, Cc, Cc, 3, 2
    op.in_cstride, op.out_cstride = in_cs, out_cs
    return op


def ksum_op(H, W, Cc, G, relu, relu_from, res, fmt, scale_ptr, shift_ptr, res_cs=None, res_coff=0, out_cs=None, out_coff=0):
    """ROMP_OP_KSUM: partials from the caller's image pointer, the result to the caller's output pointer, the residual in arena
    buffer 0 (an op input other than `in` can only be an arena buffer)."""
    from romp_amd import lib as L
    op = L.RompOp()
    op.kind, op.in_buf, op.out_buf = L.OP_KSUM, L.BUF_IMAGE, L.BUF_CENTER
    op.res_buf = L.BUF_NONE if res == 'none' else 0
    op.H, op.W, op.Cin, op.Cout, op.groups, op.relu, op.relu_from = H, W, G * Cc, Cc, G, relu, relu_from
    op.in_cstride, op.out_cstride, op.out_coff = G * Cc, out_cs or Cc, out_coff
    op.res_cstride, op.res_coff = res_cs or Cc, res_coff
    op.out_fmt, op.res_fmt, op.act_shift = (L.FMT_H2 if fmt == 'h2' else L.FMT_F32), (L.FMT_H2 if res == 'h2' else L.FMT_F32), ACT_SHIFT
    op.scale, op.shift = scale_ptr, shift_ptr
    return op
