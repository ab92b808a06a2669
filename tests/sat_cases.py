"""Case tables for the clamp-site tests (a helper, not a conftest): tests/test_sat_cases.py proves them sound without a device,
tests/test_gpu_sat_sites.py runs them on the kernels.

The f16x2 kernels clamp a value beyond 65504 / 2^ACT_SHIFT when they split it into fp16 pieces, and every site that clamps must
report into the net's counter (csrc/conv_common.h: sat_track / sat_report, sat_track_pk / sat_report_pk).
A case drives ONE op so that ONE of its sites sees a planted value T (given here in the site's scaled domain, x * 2^ACT_SHIFT;
T / 2^ACT_SHIFT is exact) and everything else is far inside the range:

  output-side sites   all-zero input (every accumulator is exactly 0), T / s in the BatchNorm shift of one channel;
  residual sites      an in-range r at single elements of the residual and T / s - r in the shift (both exact in float32; the sum is
                      T / s again, exactly); values no H2 residual could help to form (1e30, inf, NaN) stay in the shift alone;
  input-side sites    T / s at single elements of an otherwise zero float32 input; the conv copies a channel (weights 0.5 on one input
                      channel, scale 1, shift 0: one non-zero product per output, exact);
  fused blocks        one site at a time, conv1 all-zero weights, conv2 a centre-tap 0.25 copy with scale 1.

`restate_*` are the float64 "clamped arithmetic" of each op: the layer in float64 with clip(v * s, lo, 65504) / s at each site it
has (lo = 0 behind a ReLU, else -65504; a NaN goes the way fminf / fmaxf send it: to lo) and the 22-bit h1 + h2 rounding of
plan.encode_h2 where a tensor is stored as H2.  They return the site values BEFORE the clamp (scaled) too."""
import numpy as np
import torch
import torch.nn.functional as F

ACT_SHIFT = 4
S = 2.0 ** ACT_SHIFT
L = 65504.0
F32 = np.float32
INF, NAN = float('inf'), float('nan')


def pred(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


def succ(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


# the planted values (scaled domain) and their negatives
T_POS = [('pred_L', pred(L)), ('L', L), ('succ_L', succ(L)), ('65520', 65520.0), ('1e30', float(F32(1e30))), ('inf', INF),
         ('65488', 65488.0), ('succ_65488', succ(65488.0))]
PLANTED = [(n, t) for n, t in T_POS] + [('-' + n, -t) for n, t in T_POS] + [('nan', NAN)]
RES_R = 2560.0          # the in-range residual element of a residual-site case (unscaled; 40960 scaled: one fp16 piece)


def unscaled(T):
    """T / s as a float32 (exact: s is a power of two, no planted value is subnormal)."""
    v = F32(T) / F32(S)
    assert np.isnan(T) or float(v) * S == float(F32(T)), T
    return float(v)


def expect(T, form, relu, site='out'):
    """-> (report, clamps): what the counter must do when the site sees T, per form.
    report: 'zero' (counter 0 and scan column 0), 'some' (>= 1), 'any' (not asserted).  clamps: the value is beyond the limit."""
    if np.isnan(T):
        # Where no ReLU stands in front of the split -- an input-side site, a float-form output site without ReLU -- h2_sat turns the
        # NaN into the finite -65504 / s while the float32 kernels propagate it: reported.  In front of a ReLU the float32 kernels
        # give 0 (fmaxf) and so do these: the two programs agree, nothing is asserted.  That covers EVERY packed-form site: each
        # forms its pieces from relu(...) -- fmaxf / v_med3 -- so a NaN planted in front of one is 0 when it gets there (no input of
        # these ops reaches sat_report_pk's NaN arm, and no test here does).
        return ('some' if (site == 'in' or not relu) else 'any'), False
    if relu and T < 0:
        return 'zero', False                      # ReLU, not a clamp
    a = abs(T)
    if a > L:
        return 'some', True
    if form == 'packed':
        return ('any' if a > 65488.0 else 'zero'), False      # the one-ulp band (65488, 65504]: the high piece rounds to 0x7BFF
    return ('any' if a == L else 'zero'), False               # "or hit the limit exactly"


def h2_round(v):
    """The value an H2 tensor holds for the in-range float v: (h1 + h2) / s with the two fp16 roundings of plan.encode_h2."""
    xs = np.asarray(v, dtype=np.float64).astype(F32) * F32(S)
    h1 = xs.astype(np.float16)
    h2 = (xs - h1.astype(F32)).astype(np.float16)
    return ((h1.astype(F32) + h2.astype(F32)) / F32(S)).astype(np.float64)


def clamp_site(v, relu_mask):
    """float64 v (unscaled) at a site; relu_mask (broadcastable bool): the site sits behind a ReLU there.
    -> (scaled values before the clamp -- after the ReLU where there is one --, the unscaled values after it, H2-rounded)."""
    v = np.asarray(v, dtype=np.float64)
    lo = np.where(relu_mask, 0.0, -L)
    with np.errstate(invalid='ignore', over='ignore'):
        pre = np.where(relu_mask, np.fmax(v, 0.0), v) * S
        post = np.fmin(np.fmax(v * S, lo), L) / S
    return pre, h2_round(post)


def _conv64(x, w, stride):
    k = w.shape[-1]
    if not np.any(x):                                # (an all-zero input convolves to zero: most cases here)
        Ho, Wo = (x.shape[1] + 2 * (k // 2) - k) // stride + 1, (x.shape[2] + 2 * (k // 2) - k) // stride + 1
        return np.zeros((x.shape[0], Ho, Wo, w.shape[0]))
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2).double(), w.double(), None, stride=stride, padding=k // 2)
    return y.permute(0, 2, 3, 1).numpy()


def relu_mask(cout, relu, relu_from=0):
    return (np.arange(cout) >= relu_from) & bool(relu)


def restate_conv(x, w, scale, shift, res, relu, relu_from, stride, in_site, out_site):
    """One conv + BN (+ residual) (+ ReLU on channels >= relu_from) layer, NHWC.  in_site: the float32 input is split (clamped) while
    staged; out_site: the output is stored as H2.  -> (sites {'in' / 'out': scaled values before the clamp}, output float64)."""
    sites = {}
    x = np.asarray(x, dtype=np.float64)
    if in_site:
        sites['in'], x = clamp_site(x, False)
    y = _conv64(x, w, stride) * scale.double().numpy() + shift.double().numpy()
    if res is not None:
        y = y + np.asarray(res, dtype=np.float64)
    m = relu_mask(w.shape[0], relu, relu_from)
    if out_site:
        sites['out'], y = clamp_site(y, m)
    else:
        y = np.where(m, np.fmax(y, 0.0), y)
    return sites, y


def restate_bblock(x, w1, s1, b1, w2, s2, b2):
    """A BasicBlock as the fused kernels run it: t = relu(bn1(conv1 x)) split into pieces (site 'mid'), y = relu(bn2(conv2 t) + x)
    split into pieces (site 'out').  x is an H2 tensor (already rounded)."""
    sites = {}
    x = np.asarray(x, dtype=np.float64)
    t = _conv64(x, w1, 1) * s1.double().numpy() + b1.double().numpy()
    sites['mid'], t = clamp_site(t, True)
    y = _conv64(t, w2, 1) * s2.double().numpy() + b2.double().numpy() + x
    sites['out'], y = clamp_site(y, True)
    return sites, y


def restate_fusesum(terms, shifts, relu):
    """y = (relu)(sum_k up_{2^shift_k}(t_k)), stored as H2 (site 'out')."""
    y = 0.0
    for t, s in zip(terms, shifts):
        y = y + np.asarray(t, dtype=np.float64).repeat(1 << s, 1).repeat(1 << s, 2)
    sites = {}
    sites['out'], y = clamp_site(y, bool(relu))
    return sites, y


def restate_ksum(part, G, scale, shift, res, relu):
    """The split-K tail: the G float32 partial tensors (channel slices of `part`) added in order, BN, (+ residual), (ReLU), H2."""
    Cc = part.shape[-1] // G
    y = np.asarray(part, dtype=np.float64).reshape(*part.shape[:-1], G, Cc).sum(-2) * scale.double().numpy() + shift.double().numpy()
    if res is not None:
        y = y + np.asarray(res, dtype=np.float64)
    sites = {}
    sites['out'], y = clamp_site(y, bool(relu))
    return sites, y


def restate_stem(img, w, scale, shift):
    """x / 255 * 2 - 1, conv 3x3 s2 3 -> 64, BN, ReLU, H2 (site 'out')."""
    x = np.asarray(img, dtype=np.float64) / 255.0 * 2.0 - 1.0
    y = _conv64(x, w, 2) * scale.double().numpy() + shift.double().numpy()
    sites = {}
    sites['out'], y = clamp_site(y, True)
    return sites, y


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def base_shift(c):
    """An unplanted BatchNorm shift: small values of both signs, exact in fp16."""
    return ((torch.arange(c) % 5).float() - 2.0) * 0.25


def positions(B, H, W, Cc):
    """(name, (b, y, x, c)): the first element of image 0, the last element of the last image (B = 3: a persistent workgroup's last
    work item), an element of the last row (a partial row tile of the 13-row maps) in a middle channel chunk."""
    return [('first', (0, 0, 0, 0)), ('last', (B - 1, H - 1, W - 1, Cc - 1)), ('lastrow', (B // 2, H - 1, W // 2, Cc // 2 + 1))]


# (Cin, Cout, k, stride, H, W): float32 input, float32 output -- the input-side split (write_pieces) is the layer's only site
CONV_IN = [(32, 32, 3, 1, 13, 32), (64, 64, 1, 1, 13, 32), (64, 128, 3, 2, 26, 64)]
# (Cin, Cout, k, stride, H, W, relu, residual, relu_from): H2 in / out (/ residual).  Between them every kernel family's epilogue
# (tests/test_sat_cases.py checks that): generic, direct (conv_h2r / conv_h2s), conv_h2k (B = 1), conv_h2g
CONV_OUT = [
    (32, 32, 3, 1, 13, 32, True, True, 0), (64, 64, 3, 1, 13, 32, True, False, 0), (64, 128, 3, 2, 26, 64, False, False, 0),
    (32, 96, 3, 2, 26, 64, True, False, 64), (128, 96, 1, 1, 13, 32, False, False, 0), (128, 512, 1, 1, 13, 32, True, True, 0),
    (256, 64, 1, 1, 13, 32, True, True, 0), (256, 128, 1, 1, 13, 32, False, False, 0), (64, 64, 1, 2, 26, 64, True, False, 0),
]
# (H, W, C, relu): W and C / 8 powers of two (fusesum_kernel<1>) or not (fusesum_kernel<0>)
FUSESUM = [(8, 32, 64, 1), (8, 32, 64, 0), (8, 24, 64, 1), (12, 20, 96, 0)]
# (H, W, C, G, relu, residual)
KSUM = [(4, 24, 64, 4, 1, False), (4, 24, 64, 4, 0, False), (5, 8, 32, 9, 1, True)]
# (C, H, W, impl, run): conv_h2c.h 'r' (run 0: plain tiles; run > 1: the strip form) and conv_h2b.hip 'v1'
BBLOCK = [(32, 16, 48, 'r', 0), (32, 16, 48, 'v1', 0), (32, 32, 48, 'r', 2), (64, 8, 48, 'r', 0), (64, 24, 16, 'r', 3)]
# (H, W, kernel)
STEM = [(32, 64, 'mfma'), (32, 64, 'valu'), (96, 64, 'mfma')]


def conv_in_case(cfg, B, T, pos):
    """-> dict(x, w, scale, shift, planted index)."""
    cin, cout, k, s, H, W = cfg
    x = torch.zeros(B, H, W, cin)
    x[pos] = unscaled(T)
    w = torch.zeros(cout, cin, k, k)
    w[torch.arange(cout), torch.arange(cout) % cin] = 0.5
    return dict(x=x, w=w, scale=torch.ones(cout), shift=torch.zeros(cout), res=None, relu=False, relu_from=0, stride=s, planted=('in', pos))


def conv_weights(cfg):
    cin, cout, k = cfg[:3]
    g = torch.Generator().manual_seed(cin * 1000 + cout + 10 * k + cfg[3])
    return torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, torch.rand(cout, generator=g) + 0.5


def conv_out_case(cfg, B, T, ch, pos=None):
    """Zero input; shift[ch] = T / s, or (residual layers, T a value a residual can help to form) shift[ch] = T / s - r and r in the
    residual at `pos` (b, y, x) of channel ch.  T None: the baseline."""
    cin, cout, k, s, H, W, relu, use_res, relu_from = cfg
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    w, scale = conv_weights(cfg)
    shift = base_shift(cout)
    res = torch.zeros(B, Ho, Wo, cout) if use_res else None
    planted = ('out', (slice(None), slice(None), slice(None), ch))
    if T is not None:
        if use_res and np.isfinite(T) and abs(T) < 1e6:
            planted = ('out', (pos[0], pos[1], pos[2], ch))
            r = float(np.sign(T)) * RES_R
            shift[ch] = float(F32(unscaled(T)) - F32(r))
            assert float(F32(shift[ch].item()) + F32(r)) == unscaled(T)          # the kernel's float32 sum is T / s again
            res[pos[0], pos[1], pos[2], ch] = r
        else:
            shift[ch] = unscaled(T)
    return dict(x=torch.zeros(B, H, W, cin), w=w, scale=scale, shift=shift, res=res, relu=relu, relu_from=relu_from, stride=s, planted=planted)


def fusesum_case(cfg, B, T, pos):
    H, W, Cc, relu = cfg
    ts = [torch.zeros(B, H >> k, W >> k, Cc) for k in range(3)]
    ts[1][..., :] = base_shift(Cc)                   # an unplanted background of both signs
    ts[2][..., :] = 0.5
    if T is not None:
        b, y, x, c = pos
        ts[0][pos] = float(F32(unscaled(T)) - F32(ts[1][b, y // 2, x // 2, c].item()) - F32(0.5)) if np.isfinite(T) and abs(T) < 1e6 else unscaled(T)
    return dict(terms=ts, shifts=[0, 1, 2], relu=relu, planted=('out', pos))


def ksum_case(cfg, B, T, pos):
    H, W, Cc, G, relu, use_res = cfg
    part = torch.zeros(B, H, W, G * Cc)
    shift = base_shift(Cc)
    res = torch.zeros(B, H, W, Cc) if use_res else None
    if T is not None:
        b, y, x, c = pos
        v = F32(unscaled(T)) - F32(shift[c].item())
        if use_res and np.isfinite(T) and abs(T) < 1e6:
            r = float(np.sign(T)) * RES_R
            res[pos] = r
            v = v - F32(r)
        part[b, y, x, (G - 1) * Cc + c] = float(v)   # the LAST slice: every earlier partial sum is exactly 0
    return dict(part=part, G=G, scale=torch.ones(Cc), shift=shift, res=res, relu=relu, planted=('out', pos))


def bblock_case(cfg, B, T, site, ch, pos=None):
    """conv1 has all-zero weights (the block input reaches the intermediate through nothing), conv2 is a centre-tap 0.25 copy with
    scale 1.  site 'mid': zero input, T / s in conv1's shift, conv2's shift 0 -> the output is a quarter of the clamped intermediate
    (below half the limit at the block's other site).  site 'out': conv1's shift 0 (the intermediate is 0), r at `pos` of the block
    input -- the residual -- and T / s - r in conv2's shift."""
    Cc, H, W = cfg[:3]
    g = torch.Generator().manual_seed(Cc + H + W)
    x = torch.zeros(B, H, W, Cc)
    w1 = torch.zeros(Cc, Cc, 3, 3)
    w2 = torch.zeros(Cc, Cc, 3, 3)
    w2[torch.arange(Cc), torch.arange(Cc), 1, 1] = 0.25
    s1, s2 = torch.rand(Cc, generator=g) + 0.5, torch.ones(Cc)
    b1, b2 = (base_shift(Cc), torch.zeros(Cc)) if site == 'mid' else (torch.zeros(Cc), base_shift(Cc))
    planted = (site, (slice(None), slice(None), slice(None), ch))
    if T is not None:
        if site == 'mid':
            b1[ch] = unscaled(T)
        elif np.isfinite(T) and abs(T) < 1e6:
            planted = (site, (pos[0], pos[1], pos[2], ch))
            r = float(np.sign(T)) * RES_R
            b2[ch] = float(F32(unscaled(T)) - F32(r))
            x[pos[0], pos[1], pos[2], ch] = r
        else:
            b2[ch] = unscaled(T)
    return dict(x=x, w1=w1, s1=s1, b1=b1, w2=w2, s2=s2, b2=b2, planted=planted)


def stem_case(cfg, B, T, ch):
    """All-zero weights (every accumulator is exactly 0 whatever the image holds), T / s in the shift."""
    H, W, _ = cfg
    g = torch.Generator().manual_seed(H + W)
    shift = base_shift(64)
    if T is not None:
        shift[ch] = unscaled(T)
    return dict(img=torch.rand(B, H, W, 3, generator=g) * 255.0, w=torch.zeros(64, 3, 3, 3), scale=torch.ones(64), shift=shift,
                planted=('out', (slice(None), slice(None), slice(None), ch)))


def restate(kind, c):
    """-> (sites, output) of a case dict."""
    if kind in ('conv_in', 'conv_out'):
        return restate_conv(c['x'].numpy(), c['w'], c['scale'], c['shift'], None if c['res'] is None else c['res'].numpy(), c['relu'],
                            c['relu_from'], c['stride'], kind == 'conv_in', kind == 'conv_out')
    if kind == 'bblock':
        return restate_bblock(c['x'].numpy(), c['w1'], c['s1'], c['b1'], c['w2'], c['s2'], c['b2'])
    if kind == 'fusesum':
        return restate_fusesum([t.numpy() for t in c['terms']], c['shifts'], c['relu'])
    if kind == 'ksum':
        return restate_ksum(c['part'].numpy(), c['G'], c['scale'], c['shift'], None if c['res'] is None else c['res'].numpy(), c['relu'])
    if kind == 'stem':
        return restate_stem(c['img'].numpy(), c['w'], c['scale'], c['shift'])
    raise KeyError(kind)


def all_cases(B=3):
    """Every (kind, form, site, site-behind-ReLU, config, make(T) -> case dict, label) of the tables: what both test files walk.
    make(None) is the unplanted baseline."""
    out = []
    for cfg in CONV_IN:
        for pn, pos in positions(B, cfg[4], cfg[5], cfg[0]):
            out.append(('conv_in', 'float', 'in', False, cfg, (lambda T, cfg=cfg, pos=pos: conv_in_case(cfg, B, 0.0 if T is None else T, pos)), pn))
    for cfg in CONV_OUT:
        cin, cout, k, s, H, W, relu, use_res, relu_from = cfg
        Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
        for ch in (0, cout - 1):
            site_relu = bool(relu) and ch >= relu_from
            for pn, pos in (positions(B, Ho, Wo, cout) if use_res else [('channel', None)]):
                out.append(('conv_out', 'float', 'out', site_relu, cfg,
                            (lambda T, cfg=cfg, ch=ch, pos=pos: conv_out_case(cfg, B, T, ch, pos)), 'ch%d_%s' % (ch, pn)))
    for cfg in FUSESUM:
        for pn, pos in positions(B, cfg[0], cfg[1], cfg[2]):
            out.append(('fusesum', 'float', 'out', bool(cfg[3]), cfg, (lambda T, cfg=cfg, pos=pos: fusesum_case(cfg, B, T, pos)), pn))
    for cfg in KSUM:
        for pn, pos in positions(B, cfg[0], cfg[1], cfg[2]):
            out.append(('ksum', 'float', 'out', bool(cfg[4]), cfg, (lambda T, cfg=cfg, pos=pos: ksum_case(cfg, B, T, pos)), pn))
    for cfg in BBLOCK:
        Cc, H, W = cfg[:3]
        for ch in (0, Cc - 1):
            out.append(('bblock', 'packed', 'mid', True, cfg, (lambda T, cfg=cfg, ch=ch: bblock_case(cfg, B, T, 'mid', ch)), 'mid_ch%d' % ch))
        for pn, pos in positions(B, H, W, Cc):
            out.append(('bblock', 'packed', 'out', True, cfg,
                        (lambda T, cfg=cfg, pos=pos: bblock_case(cfg, B, T, 'out', pos[3], pos[:3])), 'out_' + pn))
    for cfg in STEM:
        for ch in (0, 63):
            out.append(('stem', 'float', 'out', True, cfg, (lambda T, cfg=cfg, ch=ch: stem_case(cfg, B, T, ch)), 'ch%d' % ch))
    return out


# ---- ops driven through the lowering helpers of tests/test_gpu_parity.py --------------------------------------------------------
# The fused ops whose programs plan.py lowers from several convs (their packed constants are the lowering's business) run with the
# helpers' own random weights, ALL-ZERO activations -- every accumulator is exactly 0, so a site sees its BatchNorm shift alone --
# and the planted value in the shift of one channel (every pixel of that channel is planted); the shifts in front of the planted
# site are zeroed where they would reach it.  (kind, form, site, gain): the op's output channel shows gain * the clamped value.
LOWERED = [
    ('seam1x1', 'float', 't', 1.0), ('seam1x1', 'float', 'u', 1.0),                 # conv_h2x.hip: both tracked after the clamp
    ('seam1x1_ds', 'float', 't', 1.0), ('seam1x1_ds', 'float', 'u', 1.0),           # ... with the folded downsample conv
    ('fuseup', 'float', 'out', 1.0),                                                # conv_fup.hip: h2_pack
    ('stem2', 'packed', 'mid', 0.25), ('stem2', 'packed', 'out', 1.0),              # stem2.hip: conv2 a centre-tap 0.25 copy for 'mid'
    ('stem7p', 'float', 'out', 1.0),                                                # stem7p.hip: tracked before the clamp, behind the pool
]
SEAM_SHAPES = [(1, 8, 24), (3, 16, 4)]                     # (B, H, W) of tests/test_conv_shapes.py SEAM
FUSEUP_SHAPES = [(32, 1, 1, 8, 64, 3), (64, 2, 2, 24, 64, 3), (128, 1, 3, 12, 32, 3), (32, 1, 1, 8, 64, 1), (64, 2, 2, 24, 64, 1)]      # (CO, NUP, ND, H, W, B): its FUSEUP's tile shapes, B = 3 and 1
STEM2_SHAPES = [(1, 64, 128), (3, 64, 64)]                 # (B, H, W): the smallest maps the fused stem takes
STEM7P_SHAPES = [(1, 64, 64), (3, 64, 96)]                 # (B, H, W): multiples of 32


def channel_value(T, gain=1.0):
    """What the planted channel of such an op holds (all of these sites sit behind a ReLU): gain * the H2-rounded clamp of
    relu(T / s).  None for a NaN (0 in every kernel here, but left unspecified)."""
    if np.isnan(T):
        return None
    return float(gain * h2_round(min(max(T, 0.0), L) / S))


def restate_stem2(img, w1, s1, b1, w2, s2, b2):
    """The fused stem: t = relu(bn1(conv 3x3 s2 of x / 255 * 2 - 1)) split into pieces (site 'mid'), y = relu(bn2(conv 3x3 s2 t)),
    stored as H2 (site 'out')."""
    x = np.asarray(img, dtype=np.float64) / 255.0 * 2.0 - 1.0
    sites = {}
    sites['mid'], t = clamp_site(_conv64(x, w1, 2) * s1.double().numpy() + b1.double().numpy(), True)
    sites['out'], y = clamp_site(_conv64(t, w2, 2) * s2.double().numpy() + b2.double().numpy(), True)
    return sites, y


def restate_stem7p(img, w, scale, shift):
    """ImageNet normalisation, conv 7x7 s2 p3, BN, ReLU, MaxPool2d(3, 2, 1), stored as H2 (site 'out', behind the pool)."""
    x = (np.asarray(img, dtype=np.float64) / 255.0 - np.array([0.485, 0.456, 0.406])) / np.array([0.229, 0.224, 0.225])
    m = np.fmax(_conv64(x, w, 2) * scale.double().numpy() + shift.double().numpy(), 0.0)
    p = F.max_pool2d(torch.from_numpy(m).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    sites = {}
    sites['out'], y = clamp_site(p, True)
    return sites, y


def _bn64(y, scale, shift):
    return y * scale.double().numpy() + shift.double().numpy()


def restate_seam1x1(m, x, wt, st, bt, wu, su, bu, down=None):
    """The Bottleneck seam as conv_h2x.hip runs it: t = relu(bn_t(conv1x1 m) + r) split into pieces and stored (site 't'), u =
    relu(bn_u(conv1x1 t)) split and stored (site 'u').  r is the H2 tensor x, or -- down = (w, scale, shift): the folded downsample
    -- bn_d(conv1x1 x), added in float32 without ever being split.  -> (sites, t, u)."""
    r = np.asarray(x, dtype=np.float64) if down is None else _bn64(_conv64(np.asarray(x, dtype=np.float64), down[0], 1), down[1], down[2])
    sites = {}
    sites['t'], t = clamp_site(_bn64(_conv64(np.asarray(m, dtype=np.float64), wt, 1), st, bt) + r, True)
    sites['u'], u = clamp_site(_bn64(_conv64(t, wu, 1), su, bu), True)
    return sites, t, u


def restate_fuseup(directs, srcs, ws, scs, shs):
    """conv_fup.hip: y = relu(sum of the direct tensors + sum_k up_{2^k}(bn_k(conv1x1 x_k))), x_k = srcs[k - 1] at 1 / 2^k of the
    resolution, stored as H2 (site 'out')."""
    y = 0.0
    for d in directs:
        y = y + np.asarray(d, dtype=np.float64)
    for k, (xk, w, sc, sh) in enumerate(zip(srcs, ws, scs, shs), 1):
        y = y + _bn64(_conv64(np.asarray(xk, dtype=np.float64), w, 1), sc, sh).repeat(1 << k, 1).repeat(1 << k, 2)
    sites = {}
    sites['out'], y = clamp_site(y, True)
    return sites, y
