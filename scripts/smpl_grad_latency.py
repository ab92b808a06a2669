"""Latency of smpl_backward (include/romp_hip_smpl_grad.h) beside smpl_forward and beside what a user would otherwise run:
float32 autograd through the torch restatement of the layer (tests/test_smpl_grad.py smpl_torch) on the device.  Device
events around each call, median of --calls calls after --warmup; the library is called through its C ABI on preallocated
tensors, so the figures are device time of the calls and hold no allocation.

    python scripts/smpl_grad_latency.py [--out profiles/smpl_grad_latency.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from romp_amd import lib as L  # noqa: E402
from romp_amd.smpl import SMPL  # noqa: E402
from romp_amd.synthetic import make_smpl_model  # noqa: E402
from test_smpl_grad import smpl_torch  # noqa: E402

NV, NB = 6890, 10
CONST_BYTES = 4 * (207 * NV * 3 + NV * 3 * NB + NV * 24 + NV * 3 + 26 * NV)      # posedirs, shapedirs, weights, template, regressors
GRAD_BYTES = 4 * (NV * 3 + 71 * 3)                                               # gradient read per person
PART_BYTES = 4 * 108 * (288 + NB + 207)                                          # partial rows per person, written then read


def timed(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--calls', type=int, default=50)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    model = make_smpl_model(0)
    smpl = SMPL(model).to(dev)
    dmodel = {k: v.to(dev) for k, v in model.items()}
    h, ctx = L.load(), smpl._context()
    lines = ['# SMPL layer, root_align on, gradients through verts and joints; device events, median of %d calls after %d warm-up, us (%s)'
             % (a.calls, a.warmup, torch.cuda.get_device_name(0)),
             '# torch_f32: forward + backward of the float32 torch restatement on the device (autograd), the alternative without smpl_backward',
             '# bytes: what one smpl_backward call moves by construction (constants once + gradients, gV twice for root_align, + partial rows written and read) '
             'against the algorithmic minimum (constants once + gradients)',
             '%4s %12s %12s %14s %16s %12s %12s' % ('N', 'forward_us', 'backward_us', 'fwd+bwd_us', 'torch_f32_us', 'moved_MB', 'minimum_MB')]
    print('\n'.join(lines), flush=True)
    for n in (1, 64):
        g = torch.Generator().manual_seed(n)
        betas = torch.randn(n, NB, generator=g).to(dev)
        poses = (0.4 * torch.randn(n, 72, generator=g)).to(dev)
        gv, gj = torch.randn(n, NV, 3, generator=g).to(dev), torch.randn(n, 71, 3, generator=g).to(dev)
        verts, joints = torch.empty(n, NV, 3, device=dev), torch.empty(n, 71, 3, device=dev)
        gb, gp = torch.empty_like(betas), torch.empty_like(poses)
        st = L.stream_ptr(dev)

        def fwd():
            L.check(h.smpl_forward(ctx, L.ptr(betas), NB, L.ptr(poses), n, 1, L.ptr(verts), L.ptr(joints), st))

        def bwd():
            L.check(h.smpl_backward(ctx, L.ptr(betas), NB, L.ptr(poses), n, 1, L.ptr(gv), L.ptr(gj), L.ptr(gb), L.ptr(gp), st))

        def both():
            fwd()
            bwd()

        def torch_f32():
            b, p = betas.clone().requires_grad_(True), poses.clone().requires_grad_(True)
            v, j = smpl_torch(dmodel, b, p, True, torch.float32)
            ((gv * v).sum() + (gj * j).sum()).backward()

        tf, tb, tfb, tt = (timed(f, a.warmup, a.calls) for f in (fwd, bwd, both, torch_f32))
        moved = CONST_BYTES + n * (GRAD_BYTES + 4 * NV * 3 + 2 * PART_BYTES)      # root_align: gV is read a second time
        least = CONST_BYTES + n * GRAD_BYTES
        lines.append('%4d %12.1f %12.1f %14.1f %16.1f %12.2f %12.2f' % (n, tf, tb, tfb, tt, moved / 1e6, least / 1e6))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
