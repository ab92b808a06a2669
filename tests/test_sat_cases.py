"""The clamp-site case tables (tests/sat_cases.py) are sound, shown without the kernels: in the float64 restatement every case
crosses the fp16 limit at exactly its planted elements, sees the planted value there exactly, and keeps every other site value --
and the whole unplanted baseline -- below half the limit; the expected outputs are finite; the tables cover every op kind, both
signs, both forms, sites with and without a ReLU; and the conv layers chosen reach every kernel family's epilogue."""
import ctypes as C

import numpy as np
import pytest

import sat_cases as SC

B = 3
CASES = SC.all_cases(B)


def _id(c):
    kind, form, site, relu, cfg, make, label = c
    return '%s_%s_%s' % (kind, '_'.join(str(v) for v in cfg), label)


def test_planted_values_are_exact_float32_neighbours():
    assert SC.pred(SC.L) < SC.L < SC.succ(SC.L) and SC.succ(SC.L) - SC.L == 2.0 ** -8 and SC.L - SC.pred(SC.L) == 2.0 ** -8
    names = [n for n, _ in SC.PLANTED]
    assert len(set(names)) == len(names) == 17
    for n, T in SC.PLANTED:
        u = SC.unscaled(T)
        assert np.isnan(T) or u * SC.S == T, n                 # the division by s is exact
    # fp16 rounds 65488 (a tie) down to 65472 and its successor up to 65504: the packed form's one-ulp band starts right above 65488
    assert float(np.float16(65488.0)) == 65472.0 and float(np.float16(np.float32(SC.succ(65488.0)))) == 65504.0
    assert float(np.float16(np.float32(SC.pred(SC.L)))) == 65504.0
    # what an H2 tensor holds for the in-range ones is the value itself to 22 bits; 65488 and the limit exactly
    assert SC.h2_round(65488.0 / SC.S) * SC.S == 65488.0 and SC.h2_round(SC.L / SC.S) * SC.S == SC.L
    assert abs(SC.h2_round(SC.pred(SC.L) / SC.S) * SC.S - SC.pred(SC.L)) <= 2.0 ** -8


def test_expectations_follow_the_three_forms():
    E = SC.expect
    for form in ('float', 'packed'):
        for T in (SC.succ(SC.L), 65520.0, 1e30, SC.INF):
            assert E(T, form, True) == ('some', True) and E(T, form, False) == ('some', True)
            assert E(-T, form, True) == ('zero', False)                                # ReLU, not a clamp
        assert E(65488.0, form, True) == ('zero', False) and E(-65488.0, form, False) == ('zero', False)
        assert E(SC.L, form, True)[0] == 'any'
    assert E(-65520.0, 'float', False) == ('some', True)
    assert E(SC.pred(SC.L), 'float', True)[0] == 'zero' and E(SC.pred(SC.L), 'packed', True)[0] == 'any'
    assert E(SC.succ(65488.0), 'float', False)[0] == 'zero' and E(SC.succ(65488.0), 'packed', True)[0] == 'any'
    assert E(SC.NAN, 'float', False, 'in')[0] == 'some' and E(SC.NAN, 'packed', True)[0] == 'any' and E(SC.NAN, 'float', True)[0] == 'any'
    assert E(SC.NAN, 'float', False)[0] == 'some'                  # no ReLU in front: h2_sat's -65504 where float32 propagates


def test_tables_cover_every_kind_sign_and_form():
    kinds = {c[0] for c in CASES}
    assert kinds == {'conv_in', 'conv_out', 'fusesum', 'ksum', 'bblock', 'stem'}
    assert {c[1] for c in CASES} == {'float', 'packed'}
    for kind in ('conv_out', 'fusesum', 'ksum'):                # a ReLU and a no-ReLU epilogue
        assert {c[3] for c in CASES if c[0] == kind} == {True, False}, kind
    assert any(cfg[8] > 0 for cfg in SC.CONV_OUT) and any(cfg[7] for cfg in SC.CONV_OUT) and any(not cfg[7] for cfg in SC.CONV_OUT)
    assert {c[2] for c in CASES if c[0] == 'bblock'} == {'mid', 'out'}
    assert {cfg[3] for cfg in SC.BBLOCK} == {'r', 'v1'} and any(cfg[4] > 1 for cfg in SC.BBLOCK) and {cfg[0] for cfg in SC.BBLOCK} == {32, 64}
    assert {cfg[2] for cfg in SC.STEM} == {'mfma', 'valu'}
    pow2 = {(cfg[1] & (cfg[1] - 1)) == 0 and ((cfg[2] // 8) & (cfg[2] // 8 - 1)) == 0 for cfg in SC.FUSESUM}
    assert pow2 == {True, False}                                # both forms of the fuse-sum kernel
    assert any(t > 0 for _, t in SC.PLANTED) and any(t < 0 for _, t in SC.PLANTED)
    # the fused ops that run behind the lowering helpers: both sites of each, and every planted value has a finite expectation
    assert {k for k, _, _, _ in SC.LOWERED} == {'seam1x1', 'seam1x1_ds', 'fuseup', 'stem2', 'stem7p'}
    assert {(k, s) for k, _, s, _ in SC.LOWERED} >= {('seam1x1', 't'), ('seam1x1', 'u'), ('seam1x1_ds', 't'), ('seam1x1_ds', 'u'), ('stem2', 'mid'), ('stem2', 'out')}
    for _, form, _, gain in SC.LOWERED:
        for n, T in SC.PLANTED:
            v = SC.channel_value(T, gain)
            assert (v is None) == bool(np.isnan(T)) and (v is None or (np.isfinite(v) and 0.0 <= v <= gain * SC.L / SC.S)), n
            if v is not None and T > SC.L:
                assert v == gain * SC.L / SC.S
            if v is not None and T < 0:
                assert v == 0.0 and SC.expect(T, form, True)[0] == 'zero'


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_case_crosses_the_limit_exactly_where_planted(case):
    kind, form, site, relu, cfg, make, label = case
    sites0, y0 = SC.restate(kind, make(None))
    for v in sites0.values():
        assert np.abs(v).max() < SC.L / 2, 'the unplanted baseline must stay far inside the range'
    assert np.isfinite(y0).all()
    for name, T in SC.PLANTED:
        c = make(T)
        sites, y = SC.restate(kind, c)
        where, idx = c['planted']
        assert where == site
        planted = np.zeros(sites[site].shape, dtype=bool)
        planted[idx] = True
        assert planted.any()
        for sname, v in sites.items():
            with np.errstate(invalid='ignore'):
                crossing = ~(np.abs(v) <= SC.L)                  # beyond the limit, or NaN
            mine = planted if sname == site else np.zeros(v.shape, dtype=bool)
            seen = v[mine]
            if sname == site:
                if np.isnan(T):
                    assert (relu and (seen == 0).all()) or np.isnan(seen).all(), (name, sname)
                else:
                    assert (seen == (0.0 if (relu and T < 0) else T)).all(), (name, sname, seen[:4], T)
            # (a NaN or a negative value behind a ReLU is 0 at the site)
            crosses = (not relu) if np.isnan(T) else (abs(T) > SC.L and not (relu and T < 0))
            want = mine if crosses else np.zeros(v.shape, dtype=bool)
            assert np.array_equal(crossing, want), (name, sname, int(crossing.sum()), int(want.sum()))
            assert np.abs(v[~mine]).max(initial=0.0) < SC.L / 2, (name, sname)
        assert np.isfinite(y).all(), name
        assert np.abs(y).max() <= SC.L / SC.S


def test_conv_layers_reach_every_family():
    """The H2 conv layers of the table are offered, between them, kernels of every family (so every epilogue runs); the float32-input
    layers are offered f16x2 kernels (whose staging loop holds the input-side site)."""
    from romp_amd import lib as L
    from test_conv_shapes import FAMILIES
    from test_gpu_parity import _conv_variants, _lower_conv_layer
    lib = L.load()
    buf = C.create_string_buffer(128)
    seen = set()
    for cfg in SC.CONV_OUT:
        cin, cout, k, s, H, W, relu, use_res, relu_from = cfg
        case = (cin, cout, k, s, H, relu, use_res) + ((relu_from,) if relu_from else ())
        w, scale = SC.conv_weights(cfg)
        _, op, out_h2 = _lower_conv_layer('cpu', case, H, W, w, scale, SC.base_shift(cout), 'h2')
        assert out_h2
        for in_fmt in (L.FMT_H2, L.FMT_F32):                    # (a float32 input: the float32 MFMA kernels write H2 tensors too)
            op.in_fmt = in_fmt
            for Bn in (1, 3):
                for v in _conv_variants(lib, op, Bn):
                    L.check(lib.romp_conv_describe(C.byref(op), Bn, v, buf, 128))
                    seen.add(buf.value.decode().split('_k')[0])
    assert set(FAMILIES) <= seen, sorted(set(FAMILIES) - seen)
    for cfg in SC.CONV_IN:
        cin, cout, k, s, H, W = cfg
        c = SC.conv_in_case(cfg, 1, 0.0, (0, 0, 0, 0))
        _, op, _ = _lower_conv_layer('cpu', (cin, cout, k, s, H, False, False), H, W, c['w'], c['scale'], c['shift'], 'f32')
        names = []
        for v in _conv_variants(lib, op, 3):
            L.check(lib.romp_conv_describe(C.byref(op), 3, v, buf, 128))
            names.append(buf.value.decode())
        assert any('h2' in n for n in names), (cfg, names)


def test_seam_and_fuseup_restatements_are_the_helpers_formulas_in_range():
    """restate_seam1x1 / restate_fuseup on unit-scale data, where nothing clamps: the formulas of test_gpu_parity._seam1x1 /
    _seam1x1_downsample / _fuseup in float64, up to the 22-bit rounding of the stored tensors."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(1)
    mk = lambda co, ci: (torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5, torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g) * 0.2)
    nchw = lambda t: t.permute(0, 3, 1, 2).double()
    bn = lambda t, wsb: F.conv2d(t, wsb[0].double()) * wsb[1].double().view(1, -1, 1, 1) + wsb[2].double().view(1, -1, 1, 1)
    m, x, x0 = torch.randn(2, 4, 4, 64, generator=g), torch.randn(2, 4, 4, 256, generator=g), torch.randn(2, 4, 4, 64, generator=g)
    ct, cu, cd = mk(256, 64), mk(64, 256), mk(256, 64)
    for down, r in ((None, nchw(x)), (cd, bn(nchw(x0), cd))):
        sites, t, u = SC.restate_seam1x1(m.numpy(), (x if down is None else x0).numpy(), *ct, *cu, down=down)
        rt = torch.relu(bn(nchw(m), ct) + r)
        ru = torch.relu(bn(rt, cu))
        assert max(np.abs(v).max() for v in sites.values()) < SC.L
        assert np.abs(t - rt.permute(0, 2, 3, 1).numpy()).max() < 1e-5 and np.abs(u - ru.permute(0, 2, 3, 1).numpy()).max() < 1e-5
    d, s1 = torch.randn(2, 4, 8, 32, generator=g), torch.randn(2, 2, 4, 64, generator=g)
    up = mk(32, 64)
    sites, y = SC.restate_fuseup([d.numpy()], [s1.numpy()], [up[0]], [up[1]], [up[2]])
    ref = torch.relu(nchw(d) + bn(nchw(s1), up).repeat_interleave(2, 2).repeat_interleave(2, 3)).permute(0, 2, 3, 1).numpy()
    assert np.abs(sites['out']).max() < SC.L and np.abs(y - ref).max() < 1e-5
