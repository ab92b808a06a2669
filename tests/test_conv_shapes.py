"""Non-square feature maps and partial row tiles, the part that needs no device: the case tables of tests/test_gpu_conv_shapes.py, the
check that they are not vacuous (romp_conv_describe offers a non-square map exactly the kernel variants it offers the square map of
the same width, and the 13-row and 3-row maps between them reach every kernel family), and the lowering of the fused chains on
non-square maps (plan.py must fuse them: the kinds the GPU tests then run)."""
import ctypes as C

import pytest
import torch

from test_gpu_parity import CONV_CASES, _conv_variants, _fused_basic_block, _fuseup, _lower_conv_layer, _seam1x1, _seam1x1_downsample

# ---- single conv layers --------------------------------------------------------------------------------------------------------
# Input maps (H, W) by (ksize, stride).  Output rows: 13 and 3 (no multiple of any tile height above 1: a partial tile after full
# ones / a map smaller than every tile), 20 (the 4-row tiles exact, the 8- / 16- / 32-row tiles partial behind at least one full
# tile), 24 x 48 (three tile columns of the 16-column variants, the 32-column ones not eligible).  25 x 64 under stride 2: an odd
# input height, the last 3x3 tap row is exactly iy == H.
SPATIAL = {
    (3, 1): [(13, 32), (20, 64), (3, 32), (24, 48)],
    (1, 1): [(13, 32), (20, 64), (3, 32), (24, 48)],
    (3, 2): [(26, 64), (25, 64), (40, 128), (6, 64)],         # (24 x 48 outputs: stride 1 only)
    (1, 2): [(26, 64), (25, 64), (40, 128), (6, 64)],
}

# (Cin, Cout, ksize, stride) -> the channel configurations of CONV_CASES that between them reach every kernel family
CHANNELS = [
    (32, 32, 3, 1), (64, 64, 3, 1), (128, 128, 3, 1), (256, 256, 3, 1), (256, 32, 3, 1), (32, 256, 3, 1), (16, 16, 3, 1),
    (64, 64, 3, 2), (32, 64, 3, 2), (64, 128, 3, 2), (128, 256, 3, 2), (256, 64, 3, 2), (32, 96, 3, 2),
    (64, 64, 1, 1), (64, 256, 1, 1), (256, 64, 1, 1), (256, 128, 1, 1), (128, 96, 1, 1), (64, 142, 1, 1), (64, 1, 1, 1), (32, 16, 1, 1),
    (128, 512, 1, 1), (512, 128, 1, 1), (1024, 256, 1, 1), (2048, 512, 1, 1),
    (64, 64, 1, 2), (256, 512, 1, 2), (512, 1024, 1, 2),
]


def _channel_case(cin, cout, k, s):
    """The CONV_CASES entry with these channels (its ReLU / residual / relu_from flags; its square size is not used)."""
    hits = [c for c in CONV_CASES if c[:4] == (cin, cout, k, s)]
    assert hits, (cin, cout, k, s)
    return hits[0]


# one list in run order: formats and batch sizes of a (case, H, W) follow each other, so that its reference is computed once
SHAPE_CASES = [(_channel_case(*ch), H, W) for ch in CHANNELS for (H, W) in SPATIAL[ch[2:]]]
SHAPE_PARAMS = [(case, H, W, fmt, B) for (case, H, W) in SHAPE_CASES for fmt in ('f32', 'h2') for B in (1, 3)]


def shape_id(v):
    case, H, W = v[:3]
    return 'c%d_%d_k%d_s%d_%dx%d' % (case[:4] + (H, W)) + ''.join('_%s' % t for t in v[3:])


FAMILIES = ['conv_mfma', 'conv_pp', 'conv_h2', 'conv_h2o', 'conv_h2d', 'conv_h2do', 'conv_h2r', 'conv_h2s', 'conv_h2k', 'conv_h2g']


def conv_weights(case):
    cin, cout, k, s = case[:4]
    g = torch.Generator().manual_seed(cin * 1000 + cout + 10 * k + s)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    return w, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1


def same_variants_as_square(lib, dev, case, H, W, fmt, B, wsb, op):
    """variant_ok does not look at the row count: the non-square map must be offered exactly what the square map of its width is.
    -> the variant indices."""
    got = _conv_variants(lib, op, B)
    _, sq, _ = _lower_conv_layer(dev, case, W, W, *wsb, fmt)
    want = _conv_variants(lib, sq, B)
    assert got == want, 'variants for %dx%d %s differ from the %dx%d map: %s' % (H, W, got, W, W, want)
    return got


def test_nonsquare_maps_keep_every_variant():
    """Every case of the GPU sweep is offered the same kernel variants as the square map of its width, at least one of them; and the
    13-row and the 3-row maps each reach every kernel family the library has."""
    from romp_amd import lib as L
    lib = L.load()
    buf = C.create_string_buffer(128)
    seen = {13: set(), 3: set()}
    for case, H, W in SHAPE_CASES:
        k, s = case[2:4]
        Ho = (H + 2 * (k // 2) - k) // s + 1
        wsb = conv_weights(case)
        for fmt in ('f32', 'h2'):
            _, op, _ = _lower_conv_layer('cpu', case, H, W, *wsb, fmt)
            vs = same_variants_as_square(lib, 'cpu', case, H, W, fmt, 3, wsb, op)
            assert len(vs) >= 1, (case, H, W, fmt)
            for v in vs:
                L.check(lib.romp_conv_describe(C.byref(op), 3, v, buf, 128))
                if Ho in seen:
                    seen[Ho].add(buf.value.decode().split('_k')[0])
    want = set(FAMILIES) | ({'conv_bx3', 'conv_bxd'} if L.has_bf16x3() else set())
    for rows, fams in seen.items():
        assert want <= fams, 'the %d-row maps never reach %s' % (rows, sorted(want - fams))


# ---- fused chains --------------------------------------------------------------------------------------------------------------
# (B, H, W, channels)
BBLOCK_R = [(2, 16, 48, 32), (2, 48, 16, 32), (3, 8, 48, 64), (2, 24, 16, 64)]
BBLOCK_V1 = [(1, 16, 48, 32), (1, 48, 16, 32)]
# + the strip form's run length (None: the launcher's own choice; (3, 8, 48, 64) is one tile row)
BBLOCK_STRIP = [(2, 24, 16, 64, 3), (3, 8, 48, 64, None), (2, 32, 48, 32, 2)]
# (CO, NUP, ND, H, W, B): the narrowest source map keeps 16 columns for its producer conv
FUSEUP = [(32, 3, 1, 24, 128, 2), (32, 1, 1, 8, 64, 3), (64, 2, 2, 24, 64, 3), (64, 1, 2, 64, 32, 2), (128, 1, 3, 12, 32, 3)]
# (B, H, W): B * H * W a multiple of 64
SEAM = [(1, 8, 24), (3, 16, 4), (2, 4, 48)]


def _every_conv_has_a_kernel(P, B):
    """The ordinary convs of a lowered chain (producers and readers of the fused ops) must be runnable on the map they were given."""
    from romp_amd import lib as L
    lib = L.load()
    buf = C.create_string_buffer(128)
    for op, name in zip(P.ops, P.names):
        if op.kind == L.OP_CONV:
            assert lib.romp_conv_describe(C.byref(op), B, -1, buf, 128) == 0, (name, op.H, op.W, lib.romp_last_error())


@pytest.mark.parametrize('B,H,W,Cc', BBLOCK_R + BBLOCK_V1 + [c[:4] for c in BBLOCK_STRIP])
def test_basic_blocks_fuse_on_nonsquare_maps(B, H, W, Cc, monkeypatch):
    assert H % (16 if Cc == 32 else 8) == 0 and W % 16 == 0          # the plan's fusing condition
    _every_conv_has_a_kernel(_fused_basic_block('cpu', B, H, Cc, 'r', monkeypatch, W=W, run=False), B)


@pytest.mark.parametrize('CO,NUP,ND,H,W,B', FUSEUP)
def test_up_sums_fuse_on_nonsquare_maps(CO, NUP, ND, H, W, B):
    assert (W >> NUP) >= 16
    _every_conv_has_a_kernel(_fuseup('cpu', CO, NUP, ND, H, B, W=W, run=False), B)


@pytest.mark.parametrize('B,H,W', SEAM)
def test_seams_fuse_on_nonsquare_maps(B, H, W, monkeypatch):
    assert B * H * W % 64 == 0
    for P in [_seam1x1('cpu', B, H, monkeypatch, W=W, run=False)] + _seam1x1_downsample('cpu', B, H, monkeypatch, W=W, run=False):
        _every_conv_has_a_kernel(P, B)
