"""Latency of one step of a clip fit with the temporal smoothness terms (include/romp_hip_fit_clip.h) at 64 rows (8 tracks x 8
frames) and 512 rows (64 tracks x 8 frames), four columns:

  (a) parent   the fitter step of the parent commit (smpl_forward, romp_fit_reproject, smpl_backward, romp_fit_adam), from a
               checkout of that commit with its own library, loaded beside this tree as a second package;
  (b) off      this tree's KeypointFitter with links = None: the same four entries;
  (c) on       this tree with links and every smoothness term on (joints, camera, betas, rotations): (b) plus two
               romp_fit_temporal launches;
  (d) torch    the objective of (c) in torch ops around the HIP SMPL autograd node (gathers along the links, Rodrigues in
               torch), torch.optim.Adam.

The method is that of scripts/fit_prior_latency.py, whose helpers are used: device events around each step, median of --calls
steps after --warmup; (a) and (b) take turns with each other, then (c) and (d); --repeats repeats give the spread; kernels per
step are counted with torch.profiler after every timing is taken.  (b) against (a) is reported, not gated on.

    git worktree add ../romp_parent HEAD~1 && (cd ../romp_parent && python -m romp_amd.build)   # or any checkout of the parent
    python scripts/fit_clip_latency.py --parent ../romp_parent [--out profiles/fit_clip_latency.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from fit_latency import launches  # noqa: E402
from fit_prior_latency import clock_mhz, load_parent, timed  # noqa: E402
from romp_amd.clip import clip_links  # noqa: E402
from romp_amd.fitting import KeypointFitter  # noqa: E402
from romp_amd.smpl import SMPL  # noqa: E402
from romp_amd.synthetic import make_smpl_model  # noqa: E402

W_BETAS = W_POSE = 1e-4
LR = 0.02
FRAMES = 8
SMOOTH = dict(w_smooth_pose=0.05, w_smooth_joints=(0.2, 0.5), w_smooth_cam=(0.3, 0.1), w_smooth_betas=0.4, sigma_smooth=0.3)


def rodrigues(rv):
    """The layer's formula (the 1e-8 included) in torch ops: (M,3) -> (M,3,3)."""
    angle = ((rv + 1e-8) ** 2).sum(1, keepdim=True).sqrt()
    d = rv / angle
    c, s = torch.cos(angle)[:, :, None], torch.sin(angle)[:, :, None]
    z = torch.zeros_like(d[:, 0])
    K = torch.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).reshape(-1, 3, 3)
    return torch.eye(3, device=rv.device)[None] + s * K + (1 - c) * (K @ K)


def rho(e, sigma):
    return e if sigma <= 0 else (sigma * sigma) * e / (sigma * sigma + e)


def torch_step(smpl, betas, poses, cam, poses0, kp, conf, idx, opt):
    """One step of the objective of (c) without the fused entries.  idx = (pv, nx, has_pv, has_both): for every row the linked
    rows (itself where there is none) and the masks of the terms, made once from the tables."""
    pv, nx, has_pv, has_both = idx
    sig = SMOOTH['sigma_smooth']
    opt.zero_grad()
    _, joints, _ = smpl(betas, poses)
    zero = torch.zeros((), device=joints.device)
    uv = joints[:, :, :2] * cam[:, None, 0:1] + cam[:, None, 1:]
    vis = (conf > 0) & (kp[:, :, 0] > -1.99) & (kp[:, :, 1] > -1.99)
    total = torch.where(vis, conf * conf * ((uv - kp) ** 2).sum(-1), zero).sum(1) / (vis.float().sum(1) + 1e-4)
    total = total + W_BETAS * (betas ** 2).sum(1) + W_POSE * ((poses - poses0)[:, 3:] ** 2).sum(1)
    for x, (w_vel, w_acc) in ((joints.reshape(joints.shape[0], -1), SMOOTH['w_smooth_joints']), (cam, SMOOTH['w_smooth_cam']),
                              (betas, (SMOOTH['w_smooth_betas'], 0.))):
        total = total + w_vel * torch.where(has_pv, rho(((x - x[pv]) ** 2).sum(1), sig), zero)
        if w_acc > 0:
            total = total + w_acc * torch.where(has_both, rho(((x[pv] - 2 * x + x[nx]) ** 2).sum(1), sig), zero)
    R = rodrigues(poses.reshape(-1, 3)).reshape(poses.shape[0], -1)
    total = total + SMOOTH['w_smooth_pose'] * torch.where(has_pv, rho(((R - R[pv]) ** 2).sum(1), sig), zero)
    total.sum().backward()
    opt.step()


def variants(smpl, parent, tracks, dev):
    """-> {column: its step functions} for tracks x FRAMES rows in frame-major order, each on tensors of its own, and which Adam
    (d) runs.  (a) and (b) come twice, allocated a, b, b, a, as in scripts/fit_prior_latency.py."""
    n = tracks * FRAMES
    g = torch.Generator().manual_seed(n)
    frame = torch.arange(FRAMES).repeat_interleave(tracks)
    track = torch.arange(tracks).repeat(FRAMES)
    t = frame.float()[:, None] / (FRAMES - 1)
    per_track = lambda *s: torch.randn(tracks, *s, generator=g)[track]
    betas0 = (per_track(10) + 0.05 * torch.randn(n, 10, generator=g)).to(dev)
    poses0 = (0.3 * per_track(72) + 0.2 * t * per_track(72) + 0.05 * torch.randn(n, 72, generator=g)).to(dev)
    cam0 = (torch.tensor([0.9, 0.05, -0.03]) + 0.1 * t * per_track(3)).to(dev)
    kp = (0.5 * torch.randn(n, 71, 2, generator=g)).to(dev)
    conf = (0.2 + 0.8 * torch.rand(n, 71, generator=g)).to(dev)
    links = clip_links(track.to(dev), frame.to(dev))
    prev, nxt = links[0].long(), links[1].long()
    rows = torch.arange(n, device=dev)
    idx = (torch.where(prev >= 0, prev, rows), torch.where(nxt >= 0, nxt, rows), prev >= 0, (prev >= 0) & (nxt >= 0))

    def stepper(run):
        count = [0]

        def step():
            count[0] += 1
            run.evaluate(0)
            run.update(count[0])
        return step

    args = dict(steps=0, lr=LR, w_betas=W_BETAS, w_pose=W_POSE)

    def make_old():
        p_fit, p_smpl = parent
        return stepper(p_fit.KeypointFitter(p_smpl.SMPL(make_smpl_model(0)).to(dev), **args).start(betas0, poses0, cam0, kp, conf))

    def make_off():
        return stepper(KeypointFitter(SMPL(make_smpl_model(0)).to(dev), **dict(args, **SMOOTH)).start(betas0, poses0, cam0, kp, conf, links=None))

    old = [make_old()] if parent is not None else []
    off = [make_off(), make_off()]
    old += [make_old()] if parent is not None else []
    on = stepper(KeypointFitter(smpl, **dict(args, **SMOOTH)).start(betas0, poses0, cam0, kp, conf, links=links))
    b, p, c = (x.clone().requires_grad_(True) for x in (betas0, poses0, cam0))
    try:
        opt, kind = torch.optim.Adam([b, p, c], lr=LR, fused=True), 'fused=True'
        torch_step(smpl, b, p, c, poses0, kp, conf, idx, opt)
        torch.cuda.synchronize()
    except Exception as exc:  # noqa: BLE001
        print('# Adam(fused=True) is not available here (%s): the default implementation runs' % str(exc).splitlines()[0], flush=True)
        b, p, c = (x.clone().requires_grad_(True) for x in (betas0, poses0, cam0))
        opt, kind = torch.optim.Adam([b, p, c], lr=LR), 'default (foreach)'

    def unfused():
        torch_step(smpl, b, p, c, poses0, kp, conf, idx, opt)

    return {'parent': old, 'off': off, 'on': [on], 'torch': [unfused]}, kind


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a checkout of the parent commit with its library built')
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--count', type=int, default=5)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    parent = load_parent(a.parent) if a.parent else None
    smpl = SMPL(make_smpl_model(0)).to(dev)
    names = ('parent', 'off', 'on', 'torch')
    lines = ['# one step of a clip fit (betas, poses, weak camera; 71 keypoints with confidences; L2 priors; rows = tracks x %d frames, frame-major); device events, '
             'median of %d steps after %d warm-up per repeat, %d repeats, (a) and (b) taking turns and (c) and (d) taking turns, us (%s, torch %s, engine clock read '
             'once the loops are done, the device idle again: %s)' % (FRAMES, a.calls, a.warmup, a.repeats, torch.cuda.get_device_name(0), torch.__version__, 'CLOCK'),
             '# (a) parent: the parent commit\'s KeypointFitter step on its own library (%s)' % ('loaded beside this tree' if parent else 'NOT MEASURED: no --parent'),
             '# (b) off: this tree, the smoothness weights set but links = None (smpl_forward + romp_fit_reproject + smpl_backward + romp_fit_adam)',
             '# (c) on: this tree with links and the joints, camera, betas and rotation terms on: (b) + romp_fit_temporal twice',
             '# (d) torch: the objective of (c) in torch ops around the SMPL autograd node + torch.optim.Adam(%s)',
             '# each cell: median over the repeats (lowest .. highest repeat); launches: kernels per step counted by torch.profiler']
    rows, kind, verdicts = [], None, []
    for tracks in (8, 64):
        n = tracks * FRAMES
        fns, kind = variants(smpl, parent, tracks, dev)
        live = [(nm, fns[nm][0]) for nm in names if fns[nm]]
        reps = {nm: [] for nm, _ in live}
        pair = fns['parent'][:1] + fns['off'] + fns['parent'][1:]      # a, b, b, a
        groups = [[(nm, fn) for fn in pair for nm in ('parent', 'off') if fn in fns[nm]], [('on', fns['on'][0]), ('torch', fns['torch'][0])]]
        for r in range(a.repeats):
            for group in groups:
                ts = timed([fn for _, fn in group], a.warmup, a.calls)
                for nm in dict(group):
                    reps[nm].append(statistics.mean(t for (g, _), t in zip(group, ts) if g == nm))
            print('rows %d repeat %d: %s' % (n, r, ', '.join('%s %.1f' % (nm, reps[nm][-1]) for nm, _ in live)), flush=True)
        rows.append((n, reps, dict(live)))
    lines[0] = lines[0].replace('CLOCK', clock_mhz() or 'n/a')
    fmt = lambda v: 'n/a' if v is None else '%.1f' % v
    cell = lambda t: 'n/a' if not t else '%.1f (%.1f .. %.1f)' % (statistics.median(t), min(t), max(t))
    lines.append('%4s %26s %26s %26s %26s   %s' % ('rows', '(a) parent_us', '(b) off_us', '(c) on_us', '(d) torch_us', 'launches a / b / c / d'))
    for n, reps, live in rows:
        counts = [fmt(launches(live[nm], a.count)) if nm in live else 'n/a' for nm in names]
        lines.append('%4d %26s %26s %26s %26s   %s' % (n, cell(reps.get('parent')), cell(reps['off']), cell(reps['on']), cell(reps['torch']),
                                                       ' / '.join(counts)))
        b_med, c_med, d_med = (statistics.median(reps[k]) for k in ('off', 'on', 'torch'))
        if 'parent' in reps:
            lo, hi = min(reps['parent']), max(reps['parent'])
            where = 'within' if lo <= b_med <= hi else ('below' if b_med < lo else 'above')
            verdicts.append('# rows %d: (b) %.1f us is %s the spread of (a) over %d repeats, %.1f .. %.1f us' % (n, b_med, where, a.repeats, lo, hi))
        verdicts.append('# rows %d: (c) %.1f us against (d) %.1f us (%.2fx)' % (n, c_med, d_med, d_med / c_med))
    lines[4] = lines[4] % kind
    lines += verdicts
    print('\n'.join(lines), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
