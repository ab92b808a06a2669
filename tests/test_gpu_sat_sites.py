"""Every fp16-piece clamp site ALONE: threshold, sign, NaN, region (run with -m gpu on the MI355X box).

The f16x2 kernels clamp beyond 65504 / 2^act_shift when they split a value into fp16 pieces; the API re-runs a call in float32 when
the net's device counter moved, so a site that clamps without reporting hands out wrong maps silently.  The
whole-net tests pass as soon as ANY of hundreds of launches reports.  Here each op is a net of its own (romp_net_create /
romp_net_write_buffer / romp_net_forward), ONE of its sites sees a planted value (tests/sat_cases.py: the tables, the planting that
makes the kernel's arithmetic exact, the float64 restatement), and per planted value the counter (romp_net_saturated), the op's
column of romp_net_range_scan and the stored bytes must be what the site's form promises:

  float form   beyond the limit: counter >= 1, only this op's scan column non-zero, the stored value decodes to exactly +-65504 / s;
               below it (pred(65504) included): counter 0, column 0, the value itself (22 bits); exactly the limit: either;
  packed form  the same, but anything in (65488, 65504] may report (one fp16 ulp: the high piece rounds to 0x7BFF);
  behind ReLU  a negative value is 0, not a clamp: counter 0;
  NaN          reported by an input-side split and by an output site without ReLU (it is stored as the finite -65504 / s there,
               exactly, while the float32 kernels propagate it); in front of a ReLU the float32 kernels give 0 too (fmaxf) -- the two programs agree, nothing is asserted about the
               counter there.  Every packed-form site forms its pieces from relu(...): a NaN planted in front of one is 0 when it
               gets there, so the same holds for them (sat_report_pk would report a NaN high piece; no input produces one).

In every case the output is finite, what the planted value cannot reach equals the baseline run bit
for bit, two launches give the same bytes and the same count, and a second net created alongside stays at 0.  Every inequality is
exact by construction: there is no tolerance.  One random case per op compares a layer whose site values cross by a few percent with
the clamped float64 restatement under the op's usual bound.  range_scan_kernel -- the other half of the mechanism -- is driven
alone through one-op nets against numpy.  Every line printed names the op, the kernel variant and the counter."""
import ctypes as C

import numpy as np
import pytest
import torch

import sat_cases as SC
from test_gpu_parity import _conv_variants, _lower_conv_layer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from romp_amd import lib
    lib.load()                       # fail loudly if the HIP extension is missing
    return torch.device('cuda:0')


class Rig:
    """A program as a net of its own, and a bystander net of the same program (its buffers stay zero: in range) beside it."""

    def __init__(self, dev, ops, buf_floats, B):
        from romp_amd import lib as L
        self.L, self.lib, self.dev, self.B, self.n_ops = L, L.load(), dev, B, len(ops)
        self.buf_floats = list(buf_floats)
        arr = (L.RompOp * len(ops))(*ops)
        sizes = (C.c_int64 * len(buf_floats))(*buf_floats)
        self.h, self.other = C.c_void_p(), C.c_void_p()
        self.dummy = torch.zeros(max(16, B * 16), device=dev)
        self.image = self.dummy
        try:
            L.check(self.lib.romp_net_create(C.byref(self.h), arr, len(ops), sizes, len(buf_floats), B))
            L.check(self.lib.romp_net_create(C.byref(self.other), arr, len(ops), sizes, len(buf_floats), B))
        except Exception:
            self.close()
            raise

    def close(self):
        for h in (self.h, self.other):
            if h:
                self.lib.romp_net_destroy(h)
        self.h = self.other = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def st(self):
        return self.L.stream_ptr(self.dev)

    def write(self, buf, t):
        t = t.to(self.dev).contiguous()
        assert t.dtype == torch.float32 and t.numel() == self.buf_floats[buf] * self.B, 'whole buffers only: images lie buf_floats apart'
        self.L.check(self.lib.romp_net_write_buffer(self.h, buf, self.L.ptr(t), t.numel(), self.st()))
        torch.cuda.synchronize()

    def tune(self, variants):
        self.L.check(self.lib.romp_net_set_tuned(self.h, self.B, (C.c_int32 * self.n_ops)(*variants), self.n_ops))

    def forward(self, h=None):
        self.L.check(self.lib.romp_net_forward(h or self.h, self.L.ptr(self.image), self.B, self.L.ptr(self.dummy), self.L.ptr(self.dummy), self.st()))

    def read(self, buf, shape):
        n = int(np.prod(shape))
        out = torch.empty(n, device=self.dev)
        self.L.check(self.lib.romp_net_read_buffer(self.h, buf, self.B, self.L.ptr(out), n, self.st()))
        torch.cuda.synchronize()
        return out.reshape(*shape)                   # (stays on the device: the comparisons run there)

    def counter(self, h=None, reset=1):
        c = C.c_int64(-1)
        self.L.check(self.lib.romp_net_saturated(h or self.h, C.byref(c), reset, self.st()))
        return c.value

    def scan(self):
        """-> (max |x|, non-finite count, saturation events) per op."""
        mx, bad, sat = (C.c_float * self.n_ops)(), (C.c_int32 * self.n_ops)(), (C.c_int32 * self.n_ops)()
        self.L.check(self.lib.romp_net_range_scan(self.h, self.L.ptr(self.image), self.B, self.L.ptr(self.dummy), self.L.ptr(self.dummy), self.st(), mx, bad, sat))
        return list(mx), list(bad), list(sat)

    def run(self, out_buf, shape):
        """Two launches (the same bytes, the same count) and a scan (its columns add up to that count).  -> (raw output as float32
        words, counter of one launch, the scan's saturation columns)."""
        self.counter()
        self.forward()
        raw = self.read(out_buf, shape)
        c1 = self.counter()
        self.forward()
        raw2 = self.read(out_buf, shape)
        c2 = self.counter()
        assert torch.equal(raw.view(torch.int32), raw2.view(torch.int32)), 'two launches differ'
        assert c1 == c2, 'two launches count differently: %d, %d' % (c1, c2)
        cols = self.scan()[2]
        assert sum(cols) == c1 and self.counter() == c1, (cols, c1)
        return raw, c1, cols

    def bystander_is_silent(self):
        self.forward(self.other)
        torch.cuda.synchronize()
        assert self.counter(self.other) == 0, 'the net alongside counted clamps that were not its own'


def _decode(raw, out_h2):
    from romp_amd.plan import decode_h2
    return decode_h2(raw) if out_h2 else raw


def _prep(y, y0, dev):
    """The float64 restatement of a case and of its baseline -> (expected float32 output, the elements the planted value reaches),
    on the device."""
    return torch.from_numpy(y.astype(np.float32)).to(dev), torch.from_numpy(y != y0).to(dev)


def _same_outside(raw, base_raw, out_h2, elems):
    """Is the raw output bit for bit the baseline's outside the elements `elems` (bool, the tensor's shape)?  16-bit pieces of an H2
    tensor (an element's high and low piece), words of a float32 one."""
    if not out_h2:
        return not bool(((raw.view(torch.int32) != base_raw.view(torch.int32)) & ~elems).any())
    d = raw.contiguous().view(torch.int16).reshape(*raw.shape[:-1], -1, 2, 8) != base_raw.contiguous().view(torch.int16).reshape(*raw.shape[:-1], -1, 2, 8)
    return not bool((d & ~elems.reshape(*raw.shape[:-1], -1, 1, 8)).any())


def _judge(tag, T, form, relu, site, reach_ch, raw, base_raw, want, affected, out_h2, count, cols, op_index):
    """The requirements for one planted value.  want / affected: _prep of the float64 restatement; reach_ch: the output channel the
    planted site value reaches (where the result of a NaN at an output-side site is left unspecified)."""
    report, clamps = SC.expect(T, form, relu, site)
    print('%s  T %-12s -> counter %d, scan %s (%s)' % (tag, T, count, cols, report))
    if report == 'zero':
        assert count == 0 and not any(cols), '%s: T = %r is no clamp, counter %d' % (tag, T, count)
    elif report == 'some':
        assert count >= 1, '%s: T = %r went through the clamp unreported' % (tag, T)
        assert cols[op_index] >= 1 and all(c == 0 for i, c in enumerate(cols) if i != op_index), (tag, cols)
    vals = _decode(raw, out_h2)
    assert bool(torch.isfinite(vals).all()), '%s: T = %r left inf / NaN in the output' % (tag, T)
    if np.isnan(T) and site != 'in' and relu:
        # a NaN in front of a ReLU: finite, otherwise unspecified.  Without a ReLU (an input-side split, a no-ReLU output site) the
        # split stores h2_sat's -65504 / s exactly: the restatement's value, compared below
        affected = torch.zeros_like(affected)
        affected[..., reach_ch] = True
    else:
        bad = (vals != want)
        assert not bool(bad.any()), '%s: T = %r: %d values differ from the clamped restatement, first %s got %r want %r' % (
            tag, T, int(bad.sum()), bad.nonzero()[0].tolist(), vals[bad][0].item(), want[bad][0].item())
    assert _same_outside(raw, base_raw, out_h2, affected), '%s: T = %r changed values it cannot reach' % (tag, T)


# ------------------------------------------------------------------------------ ROMP_OP_CONV
def _case_tuple(cfg):
    cin, cout, k, s, H, W, relu, use_res, relu_from = cfg
    return (cin, cout, k, s, H, relu, use_res) + ((relu_from,) if relu_from else ())


def _res_h2(c):
    from romp_amd.plan import encode_h2
    return encode_h2(c['res'])


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('in_fmt', ['h2', 'f32'])
@pytest.mark.parametrize('cfg', SC.CONV_OUT, ids=lambda c: 'c%d_%d_k%d_s%d' % c[:4])
def test_conv_output_site(dev, cfg, in_fmt, B):
    """The epilogues that write an H2 tensor -- generic (h2_pack: float form, tracked before the clamp), direct, conv_h2k, conv_h2g
    (tracked after it) -- through EVERY variant romp_conv_describe accepts, without and with an H2 residual, with a ReLU, without,
    and on the ReLU channels of a merged conv only (relu_from).  in_fmt 'f32': the same layer reading a float32 tensor (all zeros:
    its input-side split sees nothing), which is what brings the float32 MFMA kernels' epilogues in."""
    from romp_amd import lib as L
    cin, cout, k, s, H, W, relu, use_res, relu_from = cfg
    lib = L.load()
    w, scale = SC.conv_weights(cfg)
    P, op, out_h2 = _lower_conv_layer(dev, _case_tuple(cfg), H, W, w, scale, SC.base_shift(cout), 'h2')
    assert out_h2 and op.out_fmt == L.FMT_H2 and (not use_res or op.res_fmt == L.FMT_H2)
    if in_fmt == 'f32':
        op.in_fmt = L.FMT_F32
    shift_dev = P.by_ptr[op.shift].view(-1)
    variants = _conv_variants(lib, op, B)
    assert variants
    buf = C.create_string_buffer(128)
    placements = [c for c in SC.all_cases(B) if c[0] == 'conv_out' and c[4] == cfg]
    assert len(placements) == (6 if use_res else 2)
    memo = {}
    y00 = SC.restate('conv_out', placements[0][5](None))[1]

    def case(i, tname, T):
        if (i, tname) not in memo:
            c = placements[i][5](T)
            y = SC.restate('conv_out', c)[1]
            memo[(i, tname)] = (c, y, _res_h2(c).to(dev) if use_res else None, _prep(y, y00, dev))
        return memo[(i, tname)]
    with Rig(dev, [op], P.buf_floats, B) as rig:
        shape = (B,) + case(0, None, None)[1].shape[1:]
        rig.write(op.in_buf, torch.zeros(B, H, W, cin))
        for v in variants:
            rig.tune([v])
            L.check(lib.romp_conv_describe(C.byref(op), B, v, buf, 128))
            name = buf.value.decode()

            def run(c, res):
                shift_dev[:cout].copy_(c['shift'])
                if use_res:
                    rig.write(op.res_buf, res)
                torch.cuda.synchronize()
                return rig.run(op.out_buf, shape)
            c0, y0, r0, (want0, _) = case(0, None, None)
            base_raw, n0, cols0 = run(c0, r0)
            assert n0 == 0 and torch.equal(_decode(base_raw, True), want0), '%s: the baseline' % name
            for i, (_, form, site, site_relu, _, _, label) in enumerate(placements):
                for tname, T in SC.PLANTED:
                    c, y, res, (want, affected) = case(i, tname, T)
                    raw, count, cols = run(c, res)
                    _judge('conv %s (variant %d, in %s) B=%d %s' % (name, v, in_fmt, B, label), T, form, site_relu, site,
                           c['planted'][1][3], raw, base_raw, want, affected, True, count, cols, 0)
        shift_dev[:cout].copy_(c0['shift'])          # (the two nets share the layer's constants)
        rig.bystander_is_silent()


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('cfg', SC.CONV_IN, ids=lambda c: 'c%d_%d_k%d_s%d' % c[:4])
def test_conv_input_site(dev, cfg, B):
    """write_pieces (conv_split.h): the f16x2 kernels split a float32 input while they stage it -- the layer's only site here (float32
    output).  Single planted elements: the first of image 0, the last of the last image (B = 3: in a persistent workgroup's last
    work item -- the running maximum is reset per item), one of the last row.  The conv copies a channel with weight 0.5: the output
    shows the clamped value exactly.  A NaN becomes -65504 / s there and must be reported (the float32 kernels propagate it)."""
    from romp_amd import lib as L
    cin, cout, k, s, H, W = cfg
    lib = L.load()
    c0 = SC.conv_in_case(cfg, B, 0.0, (0, 0, 0, 0))
    P, op, _ = _lower_conv_layer(dev, (cin, cout, k, s, H, False, False), H, W, c0['w'], c0['scale'], c0['shift'], 'f32')
    assert op.in_fmt == L.FMT_F32 and op.out_fmt == L.FMT_F32 and op.weight_h2
    buf = C.create_string_buffer(128)
    variants = []
    for v in _conv_variants(lib, op, B):
        L.check(lib.romp_conv_describe(C.byref(op), B, v, buf, 128))
        if 'h2' in buf.value.decode():               # (the float32 / bf16x3 kernels split nothing into fp16 pieces: no site)
            variants.append((v, buf.value.decode()))
    assert variants
    placements = [c for c in SC.all_cases(B) if c[0] == 'conv_in' and c[4] == cfg]
    assert len(placements) == 3
    y0 = SC.restate('conv_in', c0)[1]
    shape = (B,) + y0.shape[1:]
    memo = {}
    with Rig(dev, [op], P.buf_floats, B) as rig:
        for v, name in variants:
            rig.tune([v])
            rig.write(op.in_buf, c0['x'])
            base_raw, n0, _ = rig.run(op.out_buf, shape)
            assert n0 == 0 and not bool(base_raw.any())
            for i, (_, form, site, _, _, make, label) in enumerate(placements):
                for tname, T in SC.PLANTED:
                    if (i, tname) not in memo:
                        c = make(T)
                        memo[(i, tname)] = (c['x'].to(dev), _prep(SC.restate('conv_in', c)[1], y0, dev))
                    x, (want, affected) = memo[(i, tname)]
                    rig.write(op.in_buf, x)
                    raw, count, cols = rig.run(op.out_buf, shape)
                    _judge('conv %s (variant %d, float32 input) B=%d %s' % (name, v, B, label), T, form, False, 'in', None, raw, base_raw,
                           want, affected, False, count, cols, 0)
        rig.bystander_is_silent()


# ------------------------------------------------------------------------------ FUSESUM, KSUM
def _keep(dev, *ts):
    return [t.to(dev).contiguous() for t in ts]


def _fusesum_h2_op(H, W, Cc, relu):
    """tests/test_gpu_conv_shapes.py's fuse-sum op -- three terms at shifts 0, 1, 2 in buffers 0 .. 2, output buffer 3 -- with float32
    terms of Cc channels each, an H2 output and the ReLU as given."""
    from romp_amd import lib as L
    from test_gpu_conv_shapes import _fusesum_op
    op = _fusesum_op(H, W, Cc, (L.FMT_F32,) * 3, L.FMT_H2, 0, Cc)
    op.relu = relu
    assert op.act_shift == SC.ACT_SHIFT and op.out_fmt == L.FMT_H2
    return op


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('cfg', SC.FUSESUM, ids=lambda c: '%dx%dx%d_relu%d' % c)
def test_fusesum_site(dev, cfg, B):
    """fusesum_kernel<1> (W and C / 8 powers of two) and <0> (the form with divisions): three float32 terms at shifts 0, 1, 2 into
    an H2 tensor (h2_pack: float form, tracked before the clamp), with and without the ReLU."""
    from romp_amd import lib as L
    H, W, Cc, relu = cfg
    op = _fusesum_h2_op(H, W, Cc, relu)
    sizes = [H * W * Cc, H * W * Cc // 4, H * W * Cc // 16, H * W * Cc]
    placements = [c for c in SC.all_cases(B) if c[0] == 'fusesum' and c[4] == cfg]
    c0 = placements[0][5](None)
    y0 = SC.restate('fusesum', c0)[1]
    shape = (B, H, W, Cc)
    with Rig(dev, [op], sizes, B) as rig:
        for k in range(3):
            rig.write(k, c0['terms'][k])
        base_raw, n0, _ = rig.run(3, shape)
        assert n0 == 0
        for _, form, site, site_relu, _, make, label in placements:
            for tname, T in SC.PLANTED:
                c = make(T)
                rig.write(0, c['terms'][0])
                raw, count, cols = rig.run(3, shape)
                _judge('fusesum<%d> %dx%dx%d relu %d B=%d %s' % (not (W & (W - 1)) and not ((Cc // 8) & (Cc // 8 - 1)), H, W, Cc, relu, B, label),
                       T, form, site_relu, site, c['planted'][1][3], raw, base_raw, *_prep(SC.restate('fusesum', c)[1], y0, dev), True, count, cols, 0)
        rig.bystander_is_silent()


def _ksum_op(dev, cfg, scale, shift):
    from romp_amd import lib as L
    H, W, Cc, G, relu, use_res = cfg
    consts = _keep(dev, scale, shift)
    op = L.RompOp()
    op.kind, op.in_buf, op.res_buf, op.out_buf = L.OP_KSUM, 0, (1 if use_res else L.BUF_NONE), 2
    op.H, op.W, op.Cin, op.Cout, op.groups, op.relu = H, W, G * Cc, Cc, G, relu
    op.in_cstride, op.out_cstride, op.res_cstride = G * Cc, Cc, Cc
    op.out_fmt, op.res_fmt, op.act_shift = L.FMT_H2, (L.FMT_H2 if use_res else L.FMT_F32), SC.ACT_SHIFT
    op.scale, op.shift = consts[0].data_ptr(), consts[1].data_ptr()
    return op, [H * W * G * Cc, H * W * Cc, H * W * Cc], consts


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('cfg', SC.KSUM, ids=lambda c: '%dx%dx%d_g%d_relu%d_res%d' % c)
def test_ksum_site(dev, cfg, B):
    """ksum_kernel, the split-K tail (h2_pack: float form, tracked before the clamp): the planted value arrives in the LAST of G
    float32 partial tensors (G = 9: the second round of the eight-slice loop), with and without ReLU / H2 residual."""
    from romp_amd.plan import encode_h2
    H, W, Cc, G, relu, use_res = cfg
    placements = [c for c in SC.all_cases(B) if c[0] == 'ksum' and c[4] == cfg]
    c0 = placements[0][5](None)
    op, sizes, consts = _ksum_op(dev, cfg, c0['scale'], c0['shift'])
    y0 = SC.restate('ksum', c0)[1]
    shape = (B, H, W, Cc)
    with Rig(dev, [op], sizes, B) as rig:
        def run(c):
            rig.write(0, c['part'])
            if use_res:
                rig.write(1, encode_h2(c['res']))
            return rig.run(2, shape)
        base_raw, n0, _ = run(c0)
        assert n0 == 0
        for _, form, site, site_relu, _, make, label in placements:
            for tname, T in SC.PLANTED:
                c = make(T)
                raw, count, cols = run(c)
                _judge('ksum %dx%dx%d G=%d relu %d res %d B=%d %s' % (H, W, Cc, G, relu, use_res, B, label), T, form, site_relu, site, c['planted'][1][3],
                       raw, base_raw, *_prep(SC.restate('ksum', c)[1], y0, dev), True, count, cols, 0)
        rig.bystander_is_silent()


# ------------------------------------------------------------------------------ the fused BasicBlocks
def _lower_block(dev, Cc, H, W, impl, ws, scs, shs, monkeypatch):
    """test_gpu_parity._fused_basic_block's program with given constants -> (program, the block's two ops [NOP, BBLOCK], its input
    and output activations).  The producer conv only makes the lowering see an H2 input; the tests write that tensor themselves."""
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math
    monkeypatch.setenv('ROMP_FUSE_BLOCKS', 'all')
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    a0 = P.conv('c0', Act(L.BUF_IMAGE, Cc, H, W, Cc), [ws[0]], [scs[0]], [shs[0]], 3, 1, True)
    a1 = P.conv('c1', a0, [ws[1]], [scs[1]], [shs[1]], 3, 1, True)
    a2 = P.conv('c2', a1, [ws[2]], [scs[2]], [shs[2]], 3, 1, True, res=a0)
    ops = P.op_array()
    kind = L.OP_BBLOCK32 if Cc == 32 else L.OP_BBLOCK64
    assert P.fused_blocks == 1 and [o.kind for o in P.ops] == [L.OP_CONV, L.OP_NOP, kind]
    if impl == 'v1':
        ops[1].flags &= ~L.OPF_WAVE16
        ops[2].flags &= ~L.OPF_WAVE16
    else:
        assert ops[1].weight_aux and ops[2].weight_aux and (ops[1].flags & ops[2].flags & L.OPF_WAVE16)
    return P, [ops[1], ops[2]], a0, a2


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('cfg', SC.BBLOCK, ids=lambda c: 'c%d_%dx%d_%s_run%d' % c)
def test_bblock_sites(dev, cfg, B, monkeypatch):
    """bblock32_kernel (conv_h2b.hip, 'v1') and the row-pipelined / strip kernels of conv_h2c.h ('r'; run > 1: the halo-carrying
    form): the PACKED form at both of a block's sites -- the intermediate (after conv1's ReLU) and the output (after the residual
    add and the ReLU) -- one at a time.  Both sit behind a ReLU: negatives are 0 and silent."""
    from romp_amd.plan import encode_h2
    Cc, H, W, impl, run_len = cfg
    monkeypatch.setenv('ROMP_BBLOCK_RUN', str(run_len))
    assert run_len == 0 or (impl == 'r' and H % 8 == 0 and (H // 8) % run_len == 0), 'the launcher takes the strip form only for runs that divide the 8-row tile rows'
    placements = [c for c in SC.all_cases(B) if c[0] == 'bblock' and c[4] == cfg]
    assert len(placements) == 5
    cm = placements[0][5](None)
    P, ops, a0, a2 = _lower_block(dev, Cc, H, W, impl, [cm['w1'], cm['w1'], cm['w2']], [cm['s1'], cm['s1'], cm['s2']],
                                  [cm['b1'], cm['b1'], cm['b2']], monkeypatch)
    b1_dev, b2_dev = P.by_ptr[ops[0].shift].view(-1), P.by_ptr[ops[1].shift].view(-1)
    shape = (B, H, W, Cc)
    with Rig(dev, ops, P.buf_floats, B) as rig:
        def run(c):
            b1_dev[:Cc].copy_(c['b1'])
            b2_dev[:Cc].copy_(c['b2'])
            rig.write(a0.buf, encode_h2(c['x']))
            return rig.run(a2.buf, shape)
        base = {}
        for _, form, site, site_relu, _, make, label in placements:
            if site not in base:
                c0 = make(None)
                base[site] = (run(c0), SC.restate('bblock', c0)[1])
                assert base[site][0][1] == 0
            (base_raw, _, _), y0 = base[site]
            for tname, T in SC.PLANTED:
                c = make(T)
                raw, count, cols = run(c)
                _judge('bblock%d %s run %d %dx%d B=%d %s' % (Cc, impl, run_len, H, W, B, label), T, form, site_relu, site,
                       c['planted'][1][3], raw, base_raw, *_prep(SC.restate('bblock', c)[1], y0, dev), True, count, cols, 1)
        b1_dev[:Cc].copy_(cm['b1'])                  # (the two nets share the block's constants)
        b2_dev[:Cc].copy_(cm['b2'])
        rig.bystander_is_silent()


# ------------------------------------------------------------------------------ STEM
def _stem_op(dev, c, H, W, kernel):
    from romp_amd import lib as L
    from romp_amd.plan import Program, set_conv_math
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    P.stem('stem', c['w'], c['scale'], c['shift'], H, W)
    op = P.ops[0]
    assert not (op.flags & L.OPF_STEM_VALU)
    op.out_fmt, op.act_shift = L.FMT_H2, SC.ACT_SHIFT
    if kernel == 'valu':
        op.flags |= L.OPF_STEM_VALU
    return P, op


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('cfg', SC.STEM, ids=lambda c: '%dx%d_%s' % c)
def test_stem_site(dev, cfg, B):
    """stem_mfma_kernel (float form, tracked after the clamp) and stem_conv_kernel (ROMP_OPF_STEM_VALU; h2_pack) writing the H2
    tensor: all-zero weights, the planted value in the BatchNorm shift (behind the stem's ReLU)."""
    H, W, kernel = cfg
    placements = [c for c in SC.all_cases(B) if c[0] == 'stem' and c[4] == cfg]
    c0 = placements[0][5](None)
    P, op = _stem_op(dev, c0, H, W, kernel)
    shift_dev = P.by_ptr[op.shift].view(-1)
    y0 = SC.restate('stem', c0)[1]
    shape = (B, H // 2, W // 2, 64)
    with Rig(dev, [op], P.buf_floats, B) as rig:
        rig.image = c0['img'].to(dev).contiguous()

        def run(c):
            shift_dev[:64].copy_(c['shift'])
            torch.cuda.synchronize()
            return rig.run(op.out_buf, shape)
        base_raw, n0, _ = run(c0)
        assert n0 == 0
        for _, form, site, site_relu, _, make, label in placements:
            for tname, T in SC.PLANTED:
                c = make(T)
                raw, count, cols = run(c)
                _judge('stem %s %dx%d B=%d %s' % (kernel, H, W, B, label), T, form, site_relu, site, c['planted'][1][3], raw, base_raw,
                       *_prep(SC.restate('stem', c)[1], y0, dev), True, count, cols, 0)
        shift_dev[:64].copy_(c0['shift'])            # (the two nets share the layer's constants)
        rig.bystander_is_silent()


# ------------------------------------------------------------------------------ the random case of each op
# Unit-scale data through an epilogue (or into an input-side split) scaled by M: |site value| crosses 65504 / s = 4094 at two standard
# deviations -- a few percent of the values, checked per case -- and the output is compared with the clamped float64 restatement under
# the op's usual bound (tests/test_gpu_parity.py: 3e-5 of the reference's largest magnitude for single layers, 5e-5 for the fused
# blocks).  A clamp at a wrong limit or on the wrong side of the ReLU misses that by orders of magnitude.
M = 2047.0


def _crossing(sites, site):
    v = sites[site]
    frac = float((np.abs(v) > SC.L).mean())
    assert 0.003 < frac < 0.2, 'the random case must cross at a few percent of the site values (%g)' % frac
    for k, o in sites.items():
        assert k == site or float(np.abs(o).max()) < SC.L, 'site %s must stay in range' % k
    return frac


def _close(tag, raw, out_h2, y, count, frac, bound):
    want = torch.from_numpy(y.astype(np.float32)).to(raw.device)
    err = float((_decode(raw, out_h2) - want).abs().max()) / float(want.abs().max())
    print('%s: %.1f %% of the site values cross -> counter %d, relative err %.3e' % (tag, 100 * frac, count, err))
    assert count >= 1, tag
    assert err < bound, (tag, err)


@pytest.mark.parametrize('in_fmt', ['h2', 'f32'])
@pytest.mark.parametrize('cfg', [SC.CONV_OUT[0], SC.CONV_OUT[2], SC.CONV_OUT[3], SC.CONV_OUT[4], SC.CONV_OUT[5]], ids=lambda c: 'c%d_%d_k%d_s%d' % c[:4])
def test_conv_output_site_random(dev, cfg, in_fmt):
    from romp_amd import lib as L
    from romp_amd.plan import encode_h2
    cin, cout, k, s, H, W, relu, use_res, relu_from = cfg
    B = 3
    lib = L.load()
    g = torch.Generator().manual_seed(cin + cout + k)
    w, scale = SC.conv_weights(cfg)
    scale, shift = scale * M, torch.randn(cout, generator=g) * 0.1 * M
    x = torch.from_numpy(SC.h2_round(torch.randn(B, H, W, cin, generator=g).numpy())).float()
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    res = torch.from_numpy(SC.h2_round((torch.randn(B, Ho, Wo, cout, generator=g) * 300.0).numpy())).float() if use_res else None
    sites, y = SC.restate_conv(x.numpy(), w, scale, shift, None if res is None else res.numpy(), relu, relu_from, s, False, True)
    frac = _crossing(sites, 'out')
    P, op, out_h2 = _lower_conv_layer(dev, _case_tuple(cfg), H, W, w, scale, shift, 'h2')
    assert out_h2
    if in_fmt == 'f32':
        op.in_fmt = L.FMT_F32
    buf = C.create_string_buffer(128)
    with Rig(dev, [op], P.buf_floats, B) as rig:
        rig.write(op.in_buf, encode_h2(x) if in_fmt == 'h2' else x)
        if use_res:
            rig.write(op.res_buf, encode_h2(res))
        for v in _conv_variants(lib, op, B):
            rig.tune([v])
            L.check(lib.romp_conv_describe(C.byref(op), B, v, buf, 128))
            raw, count, cols = rig.run(op.out_buf, (B, Ho, Wo, cout))
            _close('conv %s (variant %d, in %s) random' % (buf.value.decode(), v, in_fmt), raw, True, y, count, frac, 3e-5)


@pytest.mark.parametrize('cfg', SC.CONV_IN, ids=lambda c: 'c%d_%d_k%d_s%d' % c[:4])
def test_conv_input_site_random(dev, cfg):
    from romp_amd import lib as L
    cin, cout, k, s, H, W = cfg
    B = 3
    lib = L.load()
    g = torch.Generator().manual_seed(cin + cout + k)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1 * M
    x = torch.randn(B, H, W, cin, generator=g) * M
    sites, y = SC.restate_conv(x.numpy(), w, scale, shift, None, False, 0, s, True, False)
    frac = _crossing(sites, 'in')
    P, op, _ = _lower_conv_layer(dev, (cin, cout, k, s, H, False, False), H, W, w, scale, shift, 'f32')
    buf = C.create_string_buffer(128)
    with Rig(dev, [op], P.buf_floats, B) as rig:
        rig.write(op.in_buf, x)
        ran = 0
        for v in _conv_variants(lib, op, B):
            L.check(lib.romp_conv_describe(C.byref(op), B, v, buf, 128))
            if 'h2' not in buf.value.decode():
                continue
            rig.tune([v])
            raw, count, cols = rig.run(op.out_buf, (B,) + y.shape[1:])
            _close('conv %s (variant %d, float32 input) random' % (buf.value.decode(), v), raw, False, y, count, frac, 3e-5)
            ran += 1
        assert ran


@pytest.mark.parametrize('cfg', SC.FUSESUM, ids=lambda c: '%dx%dx%d_relu%d' % c)
def test_fusesum_site_random(dev, cfg):
    from romp_amd import lib as L
    H, W, Cc, relu = cfg
    B = 3
    g = torch.Generator().manual_seed(H + W + Cc)
    ts = [torch.randn(B, H >> k, W >> k, Cc, generator=g) * (M / 3 ** 0.5) for k in range(3)]
    sites, y = SC.restate_fusesum([t.numpy() for t in ts], [0, 1, 2], relu)
    frac = _crossing(sites, 'out')
    op = _fusesum_h2_op(H, W, Cc, relu)
    with Rig(dev, [op], [H * W * Cc, H * W * Cc // 4, H * W * Cc // 16, H * W * Cc], B) as rig:
        for k in range(3):
            rig.write(k, ts[k])
        raw, count, cols = rig.run(3, (B, H, W, Cc))
        _close('fusesum %dx%dx%d relu %d random' % cfg, raw, True, y, count, frac, 3e-5)


@pytest.mark.parametrize('cfg', SC.KSUM, ids=lambda c: '%dx%dx%d_g%d_relu%d_res%d' % c)
def test_ksum_site_random(dev, cfg):
    from romp_amd.plan import encode_h2
    H, W, Cc, G, relu, use_res = cfg
    B = 3
    g = torch.Generator().manual_seed(H + W + Cc + G)
    part = torch.randn(B, H, W, G * Cc, generator=g) * (M / G ** 0.5)
    scale, shift = torch.rand(Cc, generator=g) * 0.5 + 0.75, torch.randn(Cc, generator=g) * 0.1 * M
    res = torch.from_numpy(SC.h2_round((torch.randn(B, H, W, Cc, generator=g) * 300.0).numpy())).float() if use_res else None
    sites, y = SC.restate_ksum(part.numpy(), G, scale, shift, None if res is None else res.numpy(), relu)
    frac = _crossing(sites, 'out')
    op, sizes, consts = _ksum_op(dev, cfg, scale, shift)
    with Rig(dev, [op], sizes, B) as rig:
        rig.write(0, part)
        if use_res:
            rig.write(1, encode_h2(res))
        raw, count, cols = rig.run(2, (B, H, W, Cc))
        _close('ksum %dx%dx%d G=%d relu %d res %d random' % cfg, raw, True, y, count, frac, 3e-5)


@pytest.mark.parametrize('site', ['mid', 'out'])
@pytest.mark.parametrize('cfg', SC.BBLOCK, ids=lambda c: 'c%d_%dx%d_%s_run%d' % c)
def test_bblock_sites_random(dev, cfg, site, monkeypatch):
    """Real weights; 'mid': conv1's BatchNorm scaled by M and conv2's weights by 1 / M (the intermediate crosses, the output is
    unit-scale); 'out': conv2's BatchNorm scaled by M."""
    from romp_amd.plan import encode_h2
    Cc, H, W, impl, run_len = cfg
    B = 3
    monkeypatch.setenv('ROMP_BBLOCK_RUN', str(run_len))
    assert run_len == 0 or (impl == 'r' and H % 8 == 0 and (H // 8) % run_len == 0)
    g = torch.Generator().manual_seed(Cc + H + W + len(site))
    x = torch.from_numpy(SC.h2_round(torch.randn(B, H, W, Cc, generator=g).numpy())).float()
    ws = [torch.randn(Cc, Cc, 3, 3, generator=g) / (Cc * 9) ** 0.5 for _ in range(2)]
    sc = [torch.rand(Cc, generator=g) + 0.5 for _ in range(2)]
    sh = [torch.randn(Cc, generator=g) * 0.2 for _ in range(2)]
    if site == 'mid':
        sc[0], sh[0], ws[1] = sc[0] * M, sh[0] * M, ws[1] / 1024.0
    else:
        sc[1], sh[1] = sc[1] * M, sh[1] * M
    sites, y = SC.restate_bblock(x.numpy(), ws[0], sc[0], sh[0], ws[1], sc[1], sh[1])
    frac = _crossing(sites, site)
    P, ops, a0, a2 = _lower_block(dev, Cc, H, W, impl, [ws[0], ws[0], ws[1]], [sc[0], sc[0], sc[1]], [sh[0], sh[0], sh[1]], monkeypatch)
    with Rig(dev, ops, P.buf_floats, B) as rig:
        rig.write(a0.buf, encode_h2(x))
        raw, count, cols = rig.run(a2.buf, (B, H, W, Cc))
        assert cols[0] == 0
        _close('bblock%d %s run %d %dx%d site %s random' % (Cc, impl, run_len, H, W, site), raw, True, y, count, frac, 5e-5)


@pytest.mark.parametrize('cfg', SC.STEM, ids=lambda c: '%dx%d_%s' % c)
def test_stem_site_random(dev, cfg):
    H, W, kernel = cfg
    B = 3
    g = torch.Generator().manual_seed(H + W)
    c = dict(img=torch.rand(B, H, W, 3, generator=g) * 255.0, w=torch.randn(64, 3, 3, 3, generator=g) * 0.3,
             scale=(torch.rand(64, generator=g) + 0.5) * M, shift=torch.randn(64, generator=g) * 0.1 * M)
    sites, y = SC.restate_stem(c['img'].numpy(), c['w'], c['scale'], c['shift'])
    frac = _crossing(sites, 'out')
    P, op = _stem_op(dev, c, H, W, kernel)
    with Rig(dev, [op], P.buf_floats, B) as rig:
        rig.image = c['img'].to(dev).contiguous()
        raw, count, cols = rig.run(op.out_buf, (B, H // 2, W // 2, 64))
        _close('stem %s %dx%d random' % (kernel, H, W), raw, True, y, count, frac, 3e-5)


# ------------------------------------------------------------------------------ range_scan_kernel alone
# The other half of the mechanism: calibration decides from its max |x| which tensors may be H2 at all, RompNet.range_scan names
# clamping ops from its columns.  Driven through romp_net_range_scan on one-op nets against numpy: max |x| over the FINITE values of
# the op's output region -- exact; an H2 region's is decode_h2's maximum, the same two-term float32 sum -- and the number of
# non-finite ones.
def _scan_expect(vals):
    """(max |x| over the finite values, number of non-finite values) of a float32 tensor."""
    fin = torch.isfinite(vals)
    return (float(vals[fin].abs().max()) if bool(fin.any()) else 0.0), int((~fin).sum())


def _copy_op(H, W, Cc, cstride, coff, out_fmt):
    """A fuse sum of ONE float32 term: the op's output region -- channels [coff, coff + Cc) of a cstride-wide tensor -- is the term."""
    from romp_amd import lib as L
    from test_gpu_conv_shapes import _fusesum_op
    op = _fusesum_op(H, W, Cc, (L.FMT_F32,) * 3, out_fmt, 0, Cc)
    op.relu, op.n_terms, op.out_buf, op.out_cstride, op.out_coff = 0, 1, 1, cstride, coff
    return op


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('fmt', ['f32', 'h2'])
def test_range_scan_channel_slice(dev, fmt, B):
    """A channel slice (out_coff 8, 16 of 40 channels) whose neighbouring channels hold larger decoys and NaN words, which must not
    be counted; the maximum at the first element, at the last element of the last image, negative; NaN / inf inside the region
    counted exactly with max |x| unaffected (a float32 region: an op never writes non-finite pieces into an H2 one)."""
    from romp_amd import lib as L
    H, W, Cc, cs, coff = 5, 6, 16, 40, 8
    h2 = fmt == 'h2'
    op = _copy_op(H, W, Cc, cs, coff, L.FMT_H2 if h2 else L.FMT_F32)
    g = torch.Generator().manual_seed(3 + B)
    decoy = torch.full((B, H, W, cs), 1.0e6)
    decoy[..., ::3] = float('nan')
    plants = [('first', (0, 0, 0, 0), 3000.5), ('last', (B - 1, H - 1, W - 1, Cc - 1), 3500.25), ('negative', (B - 1, H - 1, W - 1, Cc - 1), -3900.125),
              ('middle', (B // 2, 2, 3, 9), -2222.0)]
    with Rig(dev, [op], [H * W * Cc, H * W * cs], B) as rig:
        for name, pos, v in plants + ([] if h2 else [('nonfinite', (0, 1, 1, 1), 1234.5)]):
            t = torch.rand(B, H, W, Cc, generator=g) * 200.0 - 100.0
            t[pos] = v
            n_bad = 0
            if name == 'nonfinite':
                for i, bad in enumerate([float('nan'), float('inf'), -float('inf'), float('nan'), float('inf'), float('nan')]):
                    t[(B - 1) * (i % 2), i % H, (2 * i) % W, (5 * i + 2) % Cc] = bad
                n_bad = 6
            rig.write(0, t)
            rig.write(1, decoy)
            mx, bad, sat = rig.scan()
            region = rig.read(1, (B, H, W, cs))[..., coff:coff + Cc]
            vals = _decode(region.contiguous(), h2)
            want_mx, want_bad = _scan_expect(vals)
            print('range scan %s slice B=%d %s: max |x| %r (numpy %r), non-finite %d (numpy %d), counter %d' % (fmt, B, name, mx[0], want_mx, bad[0], want_bad, sat[0]))
            assert want_mx == abs(v) and want_bad == n_bad, 'the planted value must be the region\'s maximum'
            assert mx[0] == want_mx and bad[0] == want_bad and sat[0] == 0


@pytest.mark.parametrize('fmt', ['f32', 'h2'])
def test_range_scan_whole_buffer(dev, fmt):
    """An op for which op_out_region has no dense region (here: a max-pool) is scanned as its whole arena buffer -- every float of
    every image, in the H2 reading every octet -- with the values the op did not write included: inf and NaN pieces are counted,
    the maximum is taken over the rest."""
    from romp_amd import lib as L
    from romp_amd.plan import encode_h2
    B, H, W, Cc, tail = 3, 4, 8, 8, 64
    h2 = fmt == 'h2'
    op = L.RompOp()
    op.kind, op.in_buf, op.res_buf, op.out_buf = L.OP_MAXPOOL, 0, L.BUF_NONE, 1
    op.H, op.W, op.Cin, op.Cout, op.in_cstride, op.out_cstride = H, W, Cc, Cc, Cc, Cc
    op.out_fmt, op.act_shift = (L.FMT_H2 if h2 else L.FMT_F32), SC.ACT_SHIFT
    n_out = (H // 2) * (W // 2) * Cc
    n_buf = n_out + tail                                            # per image; the pool packs its B outputs at the buffer's start
    g = torch.Generator().manual_seed(11)
    with Rig(dev, [op], [H * W * Cc, n_buf], B) as rig:
        rig.write(0, torch.zeros(B, H, W, Cc))                      # the pool writes zeros
        t = torch.rand(B * n_buf, generator=g) * 100.0
        t[-1] = -3333.0                                             # the last float of the last image
        first = B * n_out + 8                                       # the first float the pool leaves alone, and an octet to spare
        buf = encode_h2(t.reshape(-1, 8)).reshape(-1) if h2 else t.clone()
        if h2:
            words = buf.view(torch.int16).reshape(-1, 2, 8)         # (octet, piece, channel)
            words[first // 8, 0, 3] = 0x7C00                        # +inf high piece
            words[first // 8 + 9, 1, 0] = 0x7E00                    # NaN low piece
            words[B * n_buf // 8 - 2, 0, 7] = -1024                 # 0xFC00: -inf high piece
        else:
            buf[first + 5], buf[first + 77], buf[-9] = float('inf'), float('nan'), -float('inf')
        rig.write(1, buf)
        mx, bad, sat = rig.scan()
        got = rig.read(1, (B * n_buf,))
        assert not bool(got[:B * n_out].view(torch.int32).any()), 'the pool of zeros'
        vals = _decode(got.reshape(-1, 8), h2)
        want_mx, want_bad = _scan_expect(vals)
        print('range scan %s whole buffer: max |x| %r (numpy %r), non-finite %d (numpy %d)' % (fmt, mx[0], want_mx, bad[0], want_bad))
        assert want_mx == 3333.0 and want_bad == 3
        assert mx[0] == want_mx and bad[0] == want_bad


def test_range_scan_grouped_conv_region(dev):
    """A grouped conv's region is (groups - 1) * out_gstride + Cout channels: the maximum sits in the LAST channel of the second
    group, the tensor is a slice of a wider buffer of decoys."""
    from romp_amd import lib as L
    from romp_amd.plan import Program, Act, set_conv_math
    B, H, W, Cg, cs, coff = 3, 13, 32, 128, 320, 32
    g = torch.Generator().manual_seed(5)
    ws = [torch.randn(Cg, Cg, 3, 3, generator=g) / (Cg * 9) ** 0.5 for _ in range(2)]
    scs = [torch.rand(Cg, generator=g) + 0.5 for _ in range(2)]
    shs = [torch.randn(Cg, generator=g) * 0.1 for _ in range(2)]
    shs[1][Cg - 1] = -777.0
    P = Program(dev)
    set_conv_math(P, 'f32')
    P.buf_floats += [2 * Cg * H * W, cs * H * W]
    P.conv('grouped', Act(0, 2 * Cg, H, W, 2 * Cg), ws, scs, shs, 3, 1, False, out=Act(1, 2 * Cg, H, W, cs, coff), groups=2)
    op = P.ops[0]
    assert op.groups == 2 and op.out_gstride == Cg and op.Cout == Cg and op.out_cstride == cs and op.out_coff == coff
    with Rig(dev, [op], P.buf_floats, B) as rig:
        rig.write(0, torch.randn(B, H, W, 2 * Cg, generator=g))
        decoy = torch.full((B, H, W, cs), 1.0e6)
        decoy[..., 1::2] = float('nan')
        rig.write(1, decoy)
        mx, bad, sat = rig.scan()
        out = rig.read(1, (B, H, W, cs))
        want_mx, want_bad = _scan_expect(out[..., coff:coff + 2 * Cg])
        print('range scan grouped conv: max |x| %r (numpy %r), non-finite %d' % (mx[0], want_mx, bad[0]))
        assert 700.0 < want_mx < 850.0 and want_bad == 0 and float(out[..., coff + 2 * Cg - 1].abs().max()) == want_mx
        assert bool((out[..., :coff] == 1.0e6).logical_or(torch.isnan(out[..., :coff])).all()), 'the conv wrote outside its slice'
        assert mx[0] == want_mx and bad[0] == 0


def test_range_scan_stem_output_sizes(dev, monkeypatch):
    """The output regions of the stem kernels: ROMP_OP_STEM writes H / 2 x W / 2, ROMP_OP_STEM2 (whose H x W is conv2's input) half of
    that again.  The image is dark except the bottom-right corner of the last frame and every weight is positive: the maximum is in
    the last rows of the last image, where a region of the wrong size does not reach."""
    from romp_amd import lib as L
    from romp_amd.plan import Program, set_conv_math
    B, H, W = 3, 64, 128
    g = torch.Generator().manual_seed(9)
    img = torch.zeros(B, H, W, 3)
    img[B - 1, H - 16:, W - 16:] = 255.0
    w1, w2, w3 = torch.rand(64, 3, 3, 3, generator=g) * 0.3, torch.rand(64, 64, 3, 3, generator=g) / (64 * 9), torch.rand(64, 64, 1, 1, generator=g) / 64
    sc = [torch.rand(64, generator=g) + 0.5 for _ in range(3)]
    sh = [torch.zeros(64) for _ in range(3)]
    for fuse in ('1', '0'):
        monkeypatch.setenv('ROMP_FUSE_STEM2', fuse)
        P = Program(dev)
        set_conv_math(P, 'f16x2')
        a = P.stem('stem.conv1', w1, sc[0], sh[0], H, W)
        b = P.conv('stem.conv2', a, [w2], [sc[1]], [sh[1]], 3, 2, True)
        P.conv('reader', b, [w3], [sc[2]], [sh[2]], 1, 1, True)
        ops = P.op_array()
        kinds = [o.kind for o in P.ops]
        assert kinds[:2] == ([L.OP_NOP, L.OP_STEM2] if fuse == '1' else [L.OP_STEM, L.OP_CONV])
        with Rig(dev, list(ops), P.buf_floats, B) as rig:
            rig.image = img.to(dev).contiguous()
            mx, bad, sat = rig.scan()
            for i, (act, hh, ww) in ([(1, (b, H // 4, W // 4))] if fuse == '1' else [(0, (a, H // 2, W // 2)), (1, (b, H // 4, W // 4))]):
                out = _decode(rig.read(act.buf, (B, hh, ww, 64)), P.ops[i].out_fmt == L.FMT_H2)
                want_mx, want_bad = _scan_expect(out)
                where = (out.abs() == want_mx).nonzero()[0].tolist()
                print('range scan %s: max |x| %r (numpy %r) at %s' % (P.names[i], mx[i], want_mx, where))
                assert want_mx > 0 and where[0] == B - 1 and where[1] >= hh - hh // 4, 'the maximum must sit in the last rows of the last image'
                assert mx[i] == want_mx and bad[i] == 0 and sum(sat) == 0


# ------------------------------------------------------------------------------ the ops behind the lowering helpers
def _channel_sweep(tag, rig, form, gain, plant_dev, nch, out_buf, shape, op_index):
    """tests/sat_cases.py LOWERED: all-zero activations, the planted value in `plant_dev[ch]` (a BatchNorm shift on the device) for
    the first and the last channel.  The planted channel holds gain * the clamped value at every pixel, exactly; every other
    channel is the baseline's bit for bit; counter and scan column per form."""
    saved = plant_dev.clone()
    base_raw, n0, _ = rig.run(out_buf, shape)
    assert n0 == 0, '%s: the baseline counted %d' % (tag, n0)
    for ch in (0, nch - 1):
        reach = torch.zeros(shape, dtype=torch.bool, device=base_raw.device)
        reach[..., ch] = True
        for tname, T in SC.PLANTED:
            plant_dev.copy_(saved)
            plant_dev[ch] = SC.unscaled(T)
            torch.cuda.synchronize()
            raw, count, cols = rig.run(out_buf, shape)
            report, _ = SC.expect(T, form, True)
            print('%s ch %d  T %-12s -> counter %d, scan %s (%s)' % (tag, ch, T, count, cols, report))
            if report == 'zero':
                assert count == 0 and not any(cols), '%s: T = %r is no clamp, counter %d' % (tag, T, count)
            elif report == 'some':
                assert count >= 1, '%s: T = %r went through the clamp unreported' % (tag, T)
                assert cols[op_index] >= 1 and all(c == 0 for i, c in enumerate(cols) if i != op_index), (tag, cols)
            vals = _decode(raw, True)
            assert bool(torch.isfinite(vals).all()), '%s: T = %r left inf / NaN' % (tag, T)
            want = SC.channel_value(T, gain)
            if want is not None:
                got = vals[..., ch]
                assert bool((got == want).all()), '%s: T = %r: channel %d holds %r .. %r, want %r' % (tag, T, ch, got.min().item(), got.max().item(), want)
            assert _same_outside(raw, base_raw, True, reach), '%s: T = %r changed channels it cannot reach' % (tag, T)
    plant_dev.copy_(saved)
    torch.cuda.synchronize()
    rig.bystander_is_silent()


@pytest.mark.parametrize('site', ['t', 'u'])
@pytest.mark.parametrize('ds', [0, 1])
@pytest.mark.parametrize('B,H,W', SC.SEAM_SHAPES)
def test_seam1x1_sites(dev, B, H, W, ds, site, monkeypatch):
    """seam1x1_kernel (conv_h2x.hip; float form, tracked after the clamp), without and with the folded downsample conv: site 't'
    (64 -> 256 + residual + ReLU) and site 'u' (256 -> 64 + ReLU; conv 't''s shift zeroed so that nothing reaches it)."""
    from romp_amd import lib as L
    from test_gpu_parity import _seam1x1, _seam1x1_downsample
    P = _seam1x1_downsample(dev, B, H, monkeypatch, W=W, run=False)[0] if ds else _seam1x1(dev, B, H, monkeypatch, W=W, run=False)
    i = [o.kind for o in P.ops].index(L.OP_SEAM1X1)
    first = i - 2 if ds else i - 1
    assert all(P.ops[j].kind == L.OP_NOP for j in range(first, i)) and bool(P.ops[i].flags & L.OPF_SEAM_DS) == bool(ds)
    a, u = P.ops[i - 1], P.ops[i]
    sh_t, sh_u = P.by_ptr[a.shift].view(-1), P.by_ptr[u.shift].view(-1)
    if ds:
        P.by_ptr[P.ops[first].shift].zero_()          # the downsample's shift joins conv 't''s in float32: keep the planted sum exact
    if site == 'u':
        sh_t.zero_()
    torch.cuda.synchronize()
    ops = [P.ops[j] for j in range(first, i + 1)]
    with Rig(dev, ops, P.buf_floats, B) as rig:
        if site == 't':
            _channel_sweep('seam1x1%s %dx%d B=%d site t' % ('_ds' if ds else '', H, W, B), rig, 'float', 1.0, sh_t, 256, a.out_buf, (B, H, W, 256), len(ops) - 1)
        else:
            _channel_sweep('seam1x1%s %dx%d B=%d site u' % ('_ds' if ds else '', H, W, B), rig, 'float', 1.0, sh_u, 64, u.out_buf, (B, H, W, 64), len(ops) - 1)


@pytest.mark.parametrize('CO,NUP,ND,H,W,B', SC.FUSEUP_SHAPES)
def test_fuseup_site(dev, CO, NUP, ND, H, W, B):
    """fuseup_kernel (conv_fup.hip; h2_pack: float form, tracked before the clamp), its three tile shapes: zero terms, the shifts of
    its up-convs zero but the planted channel of the first."""
    from romp_amd import lib as L
    from test_gpu_parity import _fuseup
    P = _fuseup(dev, CO, NUP, ND, H, B, W=W, run=False)
    i = [o.kind for o in P.ops].index(L.OP_FUSEUP)
    F = P.ops[i]
    sh = P.by_ptr[F.shift]
    assert tuple(sh.shape) == (NUP, CO)
    sh.zero_()
    torch.cuda.synchronize()
    with Rig(dev, [F], P.buf_floats, B) as rig:
        _channel_sweep('fuseup CO=%d NUP=%d ND=%d %dx%d B=%d' % (CO, NUP, ND, H, W, B), rig, 'float', 1.0, sh.view(-1), CO, F.out_buf, (B, H, W, CO), 0)


@pytest.mark.parametrize('site', ['mid', 'out'])
@pytest.mark.parametrize('B,H,W', SC.STEM2_SHAPES)
def test_stem2_sites(dev, B, H, W, site, monkeypatch):
    """stem2_kernel (stem2.hip; the packed form at both places that form pieces): the stem's weights all zero, conv2 a centre-tap 0.25
    copy.  'mid': the planted value in the stem's shift, the output shows a quarter of the clamped intermediate; 'out': in conv2's."""
    from romp_amd import lib as L
    from romp_amd.plan import Program, set_conv_math
    monkeypatch.setenv('ROMP_FUSE_STEM2', '1')
    g = torch.Generator().manual_seed(B + H)
    w2 = torch.zeros(64, 64, 3, 3)
    w2[torch.arange(64), torch.arange(64), 1, 1] = 0.25
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    a = P.stem('stem.conv1', torch.zeros(64, 3, 3, 3), torch.ones(64), SC.base_shift(64) if site == 'mid' else torch.zeros(64), H, W)
    b = P.conv('stem.conv2', a, [w2], [torch.ones(64)], [torch.zeros(64) if site == 'mid' else SC.base_shift(64)], 3, 2, True)
    P.conv('reader', b, [torch.randn(64, 64, 1, 1, generator=g) / 8.0], [torch.ones(64)], [torch.zeros(64)], 1, 1, True)
    ops = P.op_array()
    assert P.fused_stem2 == 1 and [o.kind for o in P.ops[:2]] == [L.OP_NOP, L.OP_STEM2]
    plant = P.by_ptr[P.ops[0 if site == 'mid' else 1].shift].view(-1)
    with Rig(dev, [P.ops[0], P.ops[1]], P.buf_floats, B) as rig:
        rig.image = (torch.rand(B, H, W, 3, generator=g) * 255.0).to(dev).contiguous()
        _channel_sweep('stem2 %dx%d B=%d site %s' % (H, W, B, site), rig, 'packed', 0.25 if site == 'mid' else 1.0, plant, 64, b.buf,
                       (B, H // 4, W // 4, 64), 1)


def _lower_stem7p(dev, w, scale, shift, H, W, monkeypatch):
    from romp_amd import lib as L
    from romp_amd.plan import Program, set_conv_math
    from romp_amd.resnet_plan import _stem7, _maxpool
    monkeypatch.delenv('ROMP_STEM', raising=False)
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    y = _maxpool(P, 'pool', _stem7(P, 'stem', w, scale, shift, H, W))
    P.op_array()
    assert P.fused_stem7p == 1 and [o.kind for o in P.ops] == [L.OP_NOP, L.OP_STEM7P] and P.ops[1].out_fmt == L.FMT_H2
    return P, y


@pytest.mark.parametrize('B,H,W', SC.STEM7P_SHAPES)
def test_stem7p_site(dev, B, H, W, monkeypatch):
    """stem7p_kernel (stem7p.hip; float form, tracked before the clamp): all-zero weights, the planted value in the BatchNorm shift --
    ReLU and the 3x3 max-pool hand it on unchanged -- and the split behind the pool sees it at every pixel of the channel."""
    g = torch.Generator().manual_seed(B + W)
    P, y = _lower_stem7p(dev, torch.zeros(64, 3, 7, 7), torch.ones(64), SC.base_shift(64), H, W, monkeypatch)
    with Rig(dev, [P.ops[0], P.ops[1]], P.buf_floats, B) as rig:
        rig.image = torch.randint(0, 256, (B, H, W, 3), generator=g).float().to(dev).contiguous()
        _channel_sweep('stem7p %dx%d B=%d' % (H, W, B), rig, 'float', 1.0, P.by_ptr[P.ops[1].shift].view(-1), 64, y.buf, (B, H // 4, W // 4, 64), 1)


def test_range_scan_stem7p_output_size(dev, monkeypatch):
    """ROMP_OP_STEM7P's region is H / 4 x W / 4 of the image it is given (as test_range_scan_stem_output_sizes: the maximum sits in
    the last rows of the last image)."""
    B, H, W = 3, 64, 96
    g = torch.Generator().manual_seed(4)
    img = torch.zeros(B, H, W, 3)
    img[B - 1, H - 16:, W - 16:] = 255.0
    P, y = _lower_stem7p(dev, torch.rand(64, 3, 7, 7, generator=g) * 0.08, torch.rand(64, generator=g) + 0.5, torch.zeros(64), H, W, monkeypatch)
    with Rig(dev, [P.ops[0], P.ops[1]], P.buf_floats, B) as rig:
        rig.image = img.to(dev).contiguous()
        mx, bad, sat = rig.scan()
        out = _decode(rig.read(y.buf, (B, H // 4, W // 4, 64)), True)
        want_mx, want_bad = _scan_expect(out)
        where = (out.abs() == want_mx).nonzero()[0].tolist()
        print('range scan stem7p: max |x| %r (numpy %r) at %s' % (mx[1], want_mx, where))
        assert want_mx > 0 and where[0] == B - 1 and where[1] >= H // 4 - H // 16
        assert mx[1] == want_mx and bad[1] == 0 and sum(sat) == 0


@pytest.mark.parametrize('site', ['mid', 'out'])
def test_stem2_sites_random(dev, site, monkeypatch):
    """Real weights; 'mid': the stem's BatchNorm scaled by M and conv2's weights by 1 / 1024; 'out': conv2's BatchNorm scaled by 2 M."""
    from romp_amd import lib as L
    from romp_amd.plan import Program, set_conv_math
    monkeypatch.setenv('ROMP_FUSE_STEM2', '1')
    B, H, W = 3, 64, 128
    g = torch.Generator().manual_seed(17 + len(site))
    img = torch.rand(B, H, W, 3, generator=g) * 255.0
    w1, w2 = torch.randn(64, 3, 3, 3, generator=g) * 0.3, torch.randn(64, 64, 3, 3, generator=g) / (64 * 9) ** 0.5
    sc = [torch.rand(64, generator=g) + 0.5 for _ in range(2)]
    sh = [torch.randn(64, generator=g) * 0.2 for _ in range(2)]
    if site == 'mid':
        sc[0], sh[0], w2 = sc[0] * M, sh[0] * M, w2 / 1024.0
    else:
        sc[1], sh[1] = sc[1] * (2 * M), sh[1] * (2 * M)
    sites, y = SC.restate_stem2(img.numpy(), w1, sc[0], sh[0], w2, sc[1], sh[1])
    frac = _crossing(sites, site)
    P = Program(dev)
    set_conv_math(P, 'f16x2')
    a = P.stem('stem.conv1', w1, sc[0], sh[0], H, W)
    b = P.conv('stem.conv2', a, [w2], [sc[1]], [sh[1]], 3, 2, True)
    P.conv('reader', b, [torch.randn(64, 64, 1, 1, generator=g) / 8.0], [torch.ones(64)], [torch.zeros(64)], 1, 1, True)
    P.op_array()
    assert P.fused_stem2 == 1 and [o.kind for o in P.ops[:2]] == [L.OP_NOP, L.OP_STEM2]
    with Rig(dev, [P.ops[0], P.ops[1]], P.buf_floats, B) as rig:
        rig.image = img.to(dev).contiguous()
        raw, count, cols = rig.run(b.buf, (B, H // 4, W // 4, 64))
        _close('stem2 %dx%d site %s random' % (H, W, site), raw, True, y, count, frac, 3e-5)


def test_stem7p_site_random(dev, monkeypatch):
    B, H, W = 3, 64, 96
    g = torch.Generator().manual_seed(23)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g).float()
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.08
    scale, shift = (torch.rand(64, generator=g) + 0.5) * (M / 2), torch.randn(64, generator=g) * 0.1 * M
    sites, y = SC.restate_stem7p(img.numpy(), w, scale, shift)
    frac = _crossing(sites, 'out')
    P, act = _lower_stem7p(dev, w, scale, shift, H, W, monkeypatch)
    with Rig(dev, [P.ops[0], P.ops[1]], P.buf_floats, B) as rig:
        rig.image = img.to(dev).contiguous()
        raw, count, cols = rig.run(act.buf, (B, H // 4, W // 4, 64))
        _close('stem7p %dx%d random' % (H, W), raw, True, y, count, frac, 3e-5)


# ------------------------------------------------------------------------------ the random case of SEAM1X1 and FUSEUP
# Built on the lowering helpers of tests/test_gpu_parity.py (run=False: the program only).  The helpers keep their constants to
# themselves: _replay_* draws them again from the same seeded generator, in the same order, and the tests check the draw against
# the BatchNorm constants the program holds before they rely on it.  The activations are random (every accumulator is non-zero at
# the clamp), the BatchNorm in front of the site under test is scaled by K = 2048 IN the program (a power of two: exact).
K = 2048.0


def _h2r(t):
    return torch.from_numpy(SC.h2_round(t.numpy())).float()


def _replay_seam(B, H, W, ds):
    """The (w, scale, shift) triples _seam1x1 / _seam1x1_downsample draw -> {'d': the downsample (ds only), 't', 'u'}."""
    g = torch.Generator().manual_seed((11 if ds else 7) * B + H)
    torch.randn(B, H, W, 64, generator=g)                    # the helper's input comes first
    dims = [(64, 64), (64, 64), (64, 256), (64, 256), (256, 64), (64, 64)] if ds else [(64, 256), (256, 64), (64, 256), (256, 64), (64, 64)]
    ws = [torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5 for ci, co in dims]
    sc = [torch.rand(co, generator=g) + 0.5 for _, co in dims]
    sh = [torch.randn(co, generator=g) * 0.2 for _, co in dims]
    pick = dict(d=2, t=3, u=4) if ds else dict(t=2, u=3)
    return {k: (ws[i], sc[i], sh[i]) for k, i in pick.items()}


def _same_bn(P, op, wsb):
    """Does the program hold the replayed BatchNorm of this layer?"""
    n = wsb[1].numel()
    return torch.equal(P.by_ptr[op.scale].view(-1)[:n].cpu(), wsb[1]) and torch.equal(P.by_ptr[op.shift].view(-1)[:n].cpu(), wsb[2])


def _scale_bn(P, op, wsb, f_scale, f_shift):
    """Multiply a layer's BatchNorm by powers of two in the program (the f16x2 scale and the shift its kernels read) and in `wsb`."""
    P.by_ptr[op.scale_h2].mul_(f_scale)
    P.by_ptr[op.shift].mul_(f_shift)
    return (wsb[0], wsb[1] * f_scale, wsb[2] * f_shift)


@pytest.mark.parametrize('site', ['t', 'u'])
@pytest.mark.parametrize('ds', [0, 1])
@pytest.mark.parametrize('B,H,W', SC.SEAM_SHAPES)
def test_seam1x1_sites_random(dev, B, H, W, ds, site, monkeypatch):
    """Random m and residual (the H2 tensor x, or with ds the downsample conv's input) through the helpers' random weights.  't': conv
    t's BatchNorm times K, conv u's scale over 1024 (u stays in range); 'u': conv u's BatchNorm times K.  Both stored tensors
    against the clamped float64 restatement, 5e-5 of its largest magnitude as in _seam1x1."""
    from romp_amd import lib as L
    from romp_amd.plan import encode_h2
    from test_gpu_parity import _seam1x1, _seam1x1_downsample
    P = _seam1x1_downsample(dev, B, H, monkeypatch, W=W, run=False)[0] if ds else _seam1x1(dev, B, H, monkeypatch, W=W, run=False)
    i = [o.kind for o in P.ops].index(L.OP_SEAM1X1)
    first = i - 2 if ds else i - 1
    a, u = P.ops[i - 1], P.ops[i]
    c = _replay_seam(B, H, W, ds)
    assert _same_bn(P, a, c['t']) and _same_bn(P, u, c['u']) and (not ds or _same_bn(P, P.ops[first], c['d'])), 'the replay must be the helper\'s draw'
    if site == 't':
        c['t'], c['u'] = _scale_bn(P, a, c['t'], K, K), _scale_bn(P, u, c['u'], 1.0 / 1024.0, 1.0)
    else:
        c['u'] = _scale_bn(P, u, c['u'], K, K)
    g = torch.Generator().manual_seed(B + H + W + ds)
    m, x = _h2r(torch.randn(B, H, W, 64, generator=g)), _h2r(torch.randn(B, H, W, 64 if ds else 256, generator=g))
    sites, t_ref, u_ref = SC.restate_seam1x1(m.numpy(), x.numpy(), *c['t'], *c['u'], down=c['d'] if ds else None)
    frac = _crossing(sites, site)
    ops = [P.ops[j] for j in range(first, i + 1)]
    with Rig(dev, ops, P.buf_floats, B) as rig:
        rig.write(a.in_buf, encode_h2(m))
        rig.write(P.ops[first].in_buf if ds else a.res_buf, encode_h2(x))
        raw_u, count, cols = rig.run(u.out_buf, (B, H, W, 64))
        raw_t = rig.read(a.out_buf, (B, H, W, 256))
        tag = 'seam1x1%s %dx%d B=%d site %s random' % ('_ds' if ds else '', H, W, B, site)
        assert cols[:-1] == [0] * (len(ops) - 1)
        _close(tag + ' (t)', raw_t, True, t_ref, count, frac, 5e-5)
        _close(tag + ' (u)', raw_u, True, u_ref, count, frac, 5e-5)


def _replay_fuseup(CO, NUP, ND, H, W, B):
    """The up-convs _fuseup draws -> [(w, scale, shift) of up-conv k's channel slice [16 : 16 + CO)], k = 1 .. NUP."""
    g = torch.Generator().manual_seed(CO + 10 * NUP + H)
    torch.randn(B, H, W, 32, generator=g)

    def mk(co, ci, k):
        return (torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5, torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g) * 0.2)
    mk(CO, 32, 3)
    for k in range(1, NUP + 1):
        mk(CO << k, CO << (k - 1), 3)
    for d in range(1, ND):
        mk(CO, CO, 1)
    return [tuple(v[16:16 + CO].contiguous() for v in mk(CO + 32, CO << k, 1)) for k in range(1, NUP + 1)]


@pytest.mark.parametrize('CO,NUP,ND,H,W,B', SC.FUSEUP_SHAPES)
def test_fuseup_site_random(dev, CO, NUP, ND, H, W, B):
    """Random direct terms and up-conv sources through the helper's random up-convs, their BatchNorms times K: a few percent of the
    sums cross; against the clamped float64 restatement, 5e-5 of its largest magnitude as in _fuseup."""
    from romp_amd import lib as L
    from romp_amd.plan import encode_h2
    from test_gpu_parity import _fuseup
    P = _fuseup(dev, CO, NUP, ND, H, B, W=W, run=False)
    F = P.ops[[o.kind for o in P.ops].index(L.OP_FUSEUP)]
    ups = _replay_fuseup(CO, NUP, ND, H, W, B)
    sh = P.by_ptr[F.shift]
    assert all(torch.equal(sh[k].cpu(), ups[k][2]) for k in range(NUP)), 'the replay must be the helper\'s draw'
    assert list(F.term_shift)[:F.n_terms] == [0] * ND + list(range(1, NUP + 1)) and not any(F.term_coff)
    P.by_ptr[F.scale_h2].mul_(K)
    sh.mul_(K)
    ups = [(w, sc * K, b * K) for w, sc, b in ups]
    g = torch.Generator().manual_seed(CO + NUP + ND + B)
    directs = [_h2r(torch.randn(B, H, W, CO, generator=g)) for _ in range(ND)]
    srcs = [_h2r(torch.randn(B, H >> k, W >> k, CO << k, generator=g)) for k in range(1, NUP + 1)]
    sites, y = SC.restate_fuseup([d.numpy() for d in directs], [s.numpy() for s in srcs], *zip(*ups))
    frac = _crossing(sites, 'out')
    with Rig(dev, [F], P.buf_floats, B) as rig:
        for j, t in enumerate(directs + srcs):
            assert F.term_cstride[j] == t.shape[-1] and F.term_fmt[j] == L.FMT_H2
            rig.write(F.term_buf[j], encode_h2(t))
        raw, count, cols = rig.run(F.out_buf, (B, H, W, CO))
        _close('fuseup CO=%d NUP=%d ND=%d %dx%d B=%d random' % (CO, NUP, ND, H, W, B), raw, True, y, count, frac, 5e-5)
