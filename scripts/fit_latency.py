"""Latency of one step of a keypoint fit (romp_amd.fitting.KeypointFitter: smpl_forward, romp_fit_reproject, smpl_backward,
romp_fit_adam) beside the same step as it can be written without include/romp_hip_fit.h: the HIP SMPL autograd node, the
reprojection loss and the priors in torch ops, torch.optim.Adam.  Device events around each step, median of --calls steps
after --warmup, the variants taking turns, both at N = 1 and N = 64 in one run.  Also the share of the fused step that is
the SMPL layer itself (smpl_forward + smpl_backward from joint gradients alone, timed in the same run), and the kernels
launched per step of each variant, counted with torch.profiler over --count steps of their own after every timing is taken.

    python scripts/fit_latency.py [--out profiles/fit_latency.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from romp_amd import lib as L  # noqa: E402
from romp_amd.fitting import KeypointFitter  # noqa: E402
from romp_amd.smpl import SMPL  # noqa: E402
from romp_amd.synthetic import make_smpl_model  # noqa: E402

W_BETAS = W_POSE = 1e-4
LR = 0.02


def timed(fns, warmup, calls):
    """Median device time of one call of each function, us; the functions take turns, so a drift of the machine meets all alike."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    ts = [[] for _ in fns]
    for _ in range(calls):
        for fn, t in zip(fns, ts):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) * 1e3)
    return [statistics.median(t) for t in ts]


def launches(fn, steps):
    """Kernels per call of fn, counted by the profiler over `steps` calls; None when this build's profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()
                and 'memset' not in e.name.lower())
        return n / steps if n else None
    except Exception as exc:  # noqa: BLE001
        print('# profiler: %s' % exc, flush=True)
        return None


def torch_step(smpl, betas, poses, cam, poses0, kp, conf, opt):
    """One step of the same fit (weak camera, every joint, squared distance, the same priors) without the fused entries."""
    opt.zero_grad()
    _, joints, _ = smpl(betas, poses)
    uv = joints[:, :, :2] * cam[:, None, 0:1] + cam[:, None, 1:]
    vis = (conf > 0) & (kp[:, :, 0] > -1.99) & (kp[:, :, 1] > -1.99)
    e = ((uv - kp) ** 2).sum(-1)
    data = torch.where(vis, conf * conf * e, torch.zeros((), device=e.device)).sum(1) / (vis.float().sum(1) + 1e-4)
    prior = W_BETAS * (betas ** 2).sum(1) + W_POSE * ((poses - poses0)[:, 3:] ** 2).sum(1)
    (data + prior).sum().backward()
    opt.step()


def variants(smpl, n, dev):
    """-> (fused step, torch step, layer alone, which Adam the torch step runs) for n persons, each on tensors of its own."""
    h, ctx = L.load(), smpl._context()
    g = torch.Generator().manual_seed(n)
    betas0 = torch.randn(n, 10, generator=g).to(dev)
    poses0 = (0.3 * torch.randn(n, 72, generator=g)).to(dev)
    cam0 = torch.tensor([0.9, 0.05, -0.03]).repeat(n, 1).to(dev)
    kp = (0.5 * torch.randn(n, 71, 2, generator=g)).to(dev)
    conf = (0.2 + 0.8 * torch.rand(n, 71, generator=g)).to(dev)

    run = KeypointFitter(smpl, steps=0, lr=LR, w_betas=W_BETAS, w_pose=W_POSE).start(betas0, poses0, cam0, kp, conf)
    count = [0]

    def fused():
        count[0] += 1
        run.evaluate(0)
        run.update(count[0])

    gj = torch.randn(n, 71, 3, generator=g).to(dev)
    verts, joints = torch.empty(n, 6890, 3, device=dev), torch.empty(n, 71, 3, device=dev)
    gb, gp = torch.empty_like(betas0), torch.empty_like(poses0)
    st = L.stream_ptr(dev)

    def layer():
        L.check(h.smpl_forward(ctx, L.ptr(betas0), 10, L.ptr(poses0), n, 0, L.ptr(verts), L.ptr(joints), st))
        L.check(h.smpl_backward(ctx, L.ptr(betas0), 10, L.ptr(poses0), n, 0, None, L.ptr(gj), L.ptr(gb), L.ptr(gp), st))

    b, p, c = (t.clone().requires_grad_(True) for t in (betas0, poses0, cam0))
    try:
        opt, kind = torch.optim.Adam([b, p, c], lr=LR, fused=True), 'fused=True'
        torch_step(smpl, b, p, c, poses0, kp, conf, opt)
        torch.cuda.synchronize()
    except Exception as exc:  # noqa: BLE001
        print('# Adam(fused=True) is not available here (%s): the default implementation runs' % str(exc).splitlines()[0], flush=True)
        b, p, c = (t.clone().requires_grad_(True) for t in (betas0, poses0, cam0))
        opt, kind = torch.optim.Adam([b, p, c], lr=LR), 'default (foreach)'

    def unfused():
        torch_step(smpl, b, p, c, poses0, kp, conf, opt)

    return fused, unfused, layer, kind


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--count', type=int, default=5)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    smpl = SMPL(make_smpl_model(0)).to(dev)
    lines = ['# one step of a keypoint fit (betas, poses, weak camera; 71 keypoints with confidences; L2 priors); device events, median of %d '
             'steps after %d warm-up, us (%s, torch %s)' % (a.calls, a.warmup, torch.cuda.get_device_name(0), torch.__version__),
             '# fused: KeypointFitter (smpl_forward + romp_fit_reproject + smpl_backward + romp_fit_adam), no autograd',
             '# torch: the SMPL autograd node (smpl_forward / smpl_backward) + the loss and priors in torch ops + torch.optim.Adam(%s)',
             '# layer: smpl_forward + smpl_backward (joint gradients only) alone; share = layer / fused',
             '# launches: kernels per step counted by torch.profiler (n/a: no device events from this build)',
             '%4s %10s %10s %8s %10s %8s %16s %16s' % ('N', 'fused_us', 'torch_us', 'ratio', 'layer_us', 'share', 'fused_launches', 'torch_launches')]
    adam_kind = None
    rows = []
    for n in (1, 64):
        fused, unfused, layer, adam_kind = variants(smpl, n, dev)
        tf, tt, tl = timed((fused, unfused, layer), a.warmup, a.calls)
        print('N %d: fused %.1f us, torch %.1f us, layer %.1f us' % (n, tf, tt, tl), flush=True)
        rows.append((n, tf, tt, tl, fused, unfused))
    fmt = lambda v: 'n/a' if v is None else '%.1f' % v
    for i, (n, tf, tt, tl, fused, unfused) in enumerate(rows):       # the profiler only after every timing is taken
        lf, lt = launches(fused, a.count), launches(unfused, a.count)
        rows[i] = '%4d %10.1f %10.1f %8.2f %10.1f %8.2f %16s %16s' % (n, tf, tt, tt / tf, tl, tl / tf, fmt(lf), fmt(lt))
    lines[2] = lines[2] % adam_kind
    lines += rows
    print('\n'.join(lines), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
