"""Latency of one step of a keypoint fit with SMPLify's terms (include/romp_hip_fit_priors.h) at N = 1 and N = 64, four columns:

  (a) parent   the fitter step of the parent commit (smpl_forward, romp_fit_reproject, smpl_backward, romp_fit_adam), from a
               checkout of that commit with its own library, loaded beside this tree as a second package;
  (b) off      this tree's KeypointFitter with every new argument at its default: the same four entries;
  (c) on       this tree with the mixture (M = 8, D = 69), the angle prior and 71 3-D joints on: (b) plus romp_fit_joints3d and
               romp_fit_pose_prior;
  (d) torch    the objective of (c) in torch ops around the HIP SMPL autograd node, torch.optim.Adam.

Device events around each step, median of --calls steps after --warmup; inside every repeat (a) and (b) take turns with each
other, then (c) and (d) (the turn starts one place further each round; (a) and (b) come twice, allocated a, b, b, a); --repeats
alternated repeats give the spread of (a) that (b) is held against.  Kernels per step are counted with torch.profiler after
every timing is taken.  Two conditions are printed: (b) lies within the spread of (a), and (c) is below (d).

    git worktree add ../romp_parent HEAD~1 && (cd ../romp_parent && python -m romp_amd.build)   # or any checkout of the parent
    python scripts/fit_prior_latency.py --parent ../romp_parent [--out profiles/fit_prior_latency.txt]
"""
import argparse
import importlib
import importlib.util
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from romp_amd import lib as L  # noqa: E402
from romp_amd.fitting import KeypointFitter, PosePrior  # noqa: E402
from romp_amd.smpl import SMPL  # noqa: E402
from romp_amd.synthetic import make_smpl_model  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from fit_latency import launches  # noqa: E402

W_BETAS = W_POSE = 1e-4
W_GMM, W_ANGLE, W_3D = 1e-2, 1e-2, 1.0
LR = 0.02
ANGLE_COLUMNS, ANGLE_SIGNS = [55, 58, 12, 15], [1., -1., -1., -1.]


def load_parent(path):
    """The package of another checkout under the name romp_amd_parent; its lib.py loads the library next to it."""
    pkg = os.path.join(path, 'romp_amd')
    if not os.path.exists(os.path.join(pkg, 'libromp_hip.so')):
        raise SystemExit('%s has no built library: run `python -m romp_amd.build` in that checkout' % path)
    spec = importlib.util.spec_from_file_location('romp_amd_parent', os.path.join(pkg, '__init__.py'), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules['romp_amd_parent'] = mod
    spec.loader.exec_module(mod)
    fitting, smpl = importlib.import_module('romp_amd_parent.fitting'), importlib.import_module('romp_amd_parent.smpl')
    assert importlib.import_module('romp_amd_parent.lib').LIB_PATH != L.LIB_PATH
    return fitting, smpl


def timed(fns, warmup, calls):
    """Median device time of one call of each function, us; the functions take turns, so a drift of the machine meets all alike,
    and the turn starts one place further every round, so that each follows each other equally often (a step is bound by the
    host issuing its launches, and the one that runs after the long torch step finds the host's caches cold)."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    ts = [[] for _ in fns]
    for i in range(calls):
        order = [(i + k) % len(fns) for k in range(len(fns))]
        for fn, t in ((fns[k], ts[k]) for k in order):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) * 1e3)
    return [statistics.median(t) for t in ts]


def synthetic_prior(dev, M=8, D=69):
    g = torch.Generator().manual_seed(7)
    A = torch.randn(M, D, D, generator=g, dtype=torch.float64)
    covars = 0.05 * (A @ A.transpose(1, 2) / D + torch.eye(D, dtype=torch.float64))
    return PosePrior(0.3 * torch.randn(M, D, generator=g), covars, torch.full((M,), 1.0 / M), dev)


def torch_step(smpl, betas, poses, cam, poses0, kp, conf, t3, c3, prior, angle, opt):
    """One step of the objective of (c) without the fused entries: weak camera, every joint, squared distances."""
    opt.zero_grad()
    _, joints, _ = smpl(betas, poses)
    zero = torch.zeros((), device=joints.device)
    uv = joints[:, :, :2] * cam[:, None, 0:1] + cam[:, None, 1:]
    vis = (conf > 0) & (kp[:, :, 0] > -1.99) & (kp[:, :, 1] > -1.99)
    data = torch.where(vis, conf * conf * ((uv - kp) ** 2).sum(-1), zero).sum(1) / (vis.float().sum(1) + 1e-4)
    vis3 = (c3 > 0) & (t3[:, :, 0] != -2.) & ~torch.isnan(t3).any(-1)
    data3 = torch.where(vis3, c3 * c3 * ((joints - t3) ** 2).sum(-1), zero).sum(1) / (vis3.float().sum(1) + 1e-4)
    d = poses[:, None, 3:] - prior.means[None]
    gmm = (0.5 * (torch.einsum('mij,bmj->bmi', prior.precisions, d) * d).sum(-1) + prior.offsets[None]).min(1).values
    angle = (torch.exp(poses[:, angle[0]] * angle[1]) ** 2).sum(-1)                 # index and signs live on the device
    l2 = W_BETAS * (betas ** 2).sum(1) + W_POSE * ((poses - poses0)[:, 3:] ** 2).sum(1)
    (data + W_3D * data3 + W_GMM * gmm + W_ANGLE * angle + l2).sum().backward()
    opt.step()


def variants(smpl, parent, n, dev):
    """-> {column: its step functions} for n persons, each on tensors of its own, and which Adam (d) runs.  (a) and (b) come
    twice, allocated in the order a, b, b, a, and a column's time is the mean of its two: with one each, whichever was allocated
    first measured about 0.5 us faster on the same nine launches, whichever checkout it came from.  No (a) without a parent."""
    g = torch.Generator().manual_seed(n)
    betas0 = torch.randn(n, 10, generator=g).to(dev)
    poses0 = (0.3 * torch.randn(n, 72, generator=g)).to(dev)
    cam0 = torch.tensor([0.9, 0.05, -0.03]).repeat(n, 1).to(dev)
    kp = (0.5 * torch.randn(n, 71, 2, generator=g)).to(dev)
    conf = (0.2 + 0.8 * torch.rand(n, 71, generator=g)).to(dev)
    t3 = (0.4 * torch.randn(n, 71, 3, generator=g)).to(dev)
    c3 = (0.2 + 0.8 * torch.rand(n, 71, generator=g)).to(dev)
    prior = synthetic_prior(dev)
    angle = (torch.tensor(ANGLE_COLUMNS, device=dev), torch.tensor(ANGLE_SIGNS, device=dev))

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

    def make_off():                                                  # a layer of its own, as (a) has one
        return stepper(KeypointFitter(SMPL(make_smpl_model(0)).to(dev), **args).start(betas0, poses0, cam0, kp, conf))

    old = [make_old()] if parent is not None else []
    off = [make_off(), make_off()]
    old += [make_old()] if parent is not None else []
    on = stepper(KeypointFitter(smpl, pose_prior=prior, w_gmm=W_GMM, w_angle=W_ANGLE, w_3d=W_3D, **args).start(
        betas0, poses0, cam0, kp, conf, joints3d=t3, conf3d=c3))
    b, p, c = (t.clone().requires_grad_(True) for t in (betas0, poses0, cam0))
    try:
        opt, kind = torch.optim.Adam([b, p, c], lr=LR, fused=True), 'fused=True'
        torch_step(smpl, b, p, c, poses0, kp, conf, t3, c3, prior, angle, opt)
        torch.cuda.synchronize()
    except Exception as exc:  # noqa: BLE001
        print('# Adam(fused=True) is not available here (%s): the default implementation runs' % str(exc).splitlines()[0], flush=True)
        b, p, c = (t.clone().requires_grad_(True) for t in (betas0, poses0, cam0))
        opt, kind = torch.optim.Adam([b, p, c], lr=LR), 'default (foreach)'

    def unfused():
        torch_step(smpl, b, p, c, poses0, kp, conf, t3, c3, prior, angle, opt)

    return {'parent': old, 'off': off, 'on': [on], 'torch': [unfused]}, kind


def clock_mhz():
    """The engine clock as the driver reports it now, or None."""
    try:
        import glob
        for f in glob.glob('/sys/class/drm/card*/device/pp_dpm_sclk'):
            for line in open(f):
                if line.strip().endswith('*'):
                    return line.split(':')[1].strip().rstrip('*').strip()
    except Exception:  # noqa: BLE001
        pass
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a checkout of the parent commit with its library built')
    ap.add_argument('--out', default=None)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--count', type=int, default=5)
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit('the spread of (a) needs at least three repeats')
    dev = torch.device('cuda:0')
    parent = load_parent(a.parent) if a.parent else None
    smpl = SMPL(make_smpl_model(0)).to(dev)
    names = ('parent', 'off', 'on', 'torch')
    lines = ['# one step of a keypoint fit (betas, poses, weak camera; 71 keypoints with confidences; L2 priors); device events, median of '
             '%d steps after %d warm-up per repeat, %d repeats, (a) and (b) taking turns and (c) and (d) taking turns, us (%s, torch %s, engine clock read once the loops are done, the device idle again: %s)'
             % (a.calls, a.warmup, a.repeats, torch.cuda.get_device_name(0), torch.__version__, 'CLOCK'),
             '# (a) parent: the parent commit\'s KeypointFitter step on its own library (%s)' % ('loaded beside this tree' if parent else 'NOT MEASURED: no --parent'),
             '# (b) off: this tree, every new argument at its default (smpl_forward + romp_fit_reproject + smpl_backward + romp_fit_adam)',
             '# (c) on: this tree with the mixture (M = 8, D = 69), the angle prior and 71 3-D joints: (b) + romp_fit_joints3d + romp_fit_pose_prior',
             '# (d) torch: the objective of (c) in torch ops around the SMPL autograd node + torch.optim.Adam(%s)',
             '# (a) and (b) run twice each on buffers allocated in the order a, b, b, a, and a repeat\'s figure is the mean of the two medians',
             '# each cell: median over the repeats (lowest .. highest repeat); launches: kernels per step counted by torch.profiler']
    rows, kind, verdicts = [], None, []
    for n in (1, 64):
        fns, kind = variants(smpl, parent, n, dev)
        live = [(nm, fns[nm][0]) for nm in names if fns[nm]]
        reps = {nm: [] for nm, _ in live}
        # (a) and (b) take turns with each other only, and so do (c) and (d): with all four in one turn the parent's library ran
        # one step in four and this tree's three, and its nine kernels measured 5 to 10 us slower than the same nine of (b)
        pair = fns['parent'][:1] + fns['off'] + fns['parent'][1:]      # a, b, b, a
        groups = [[(nm, fn) for fn in pair for nm in ('parent', 'off') if fn in fns[nm]], [('on', fns['on'][0]), ('torch', fns['torch'][0])]]
        for r in range(a.repeats):
            for group in groups:
                ts = timed([fn for _, fn in group], a.warmup, a.calls)
                for nm in dict(group):
                    reps[nm].append(statistics.mean(t for (g, _), t in zip(group, ts) if g == nm))
            print('N %d repeat %d: %s' % (n, r, ', '.join('%s %.1f' % (nm, reps[nm][-1]) for nm, _ in live)), flush=True)
        rows.append((n, reps, dict(live)))
    lines[0] = lines[0].replace('CLOCK', clock_mhz() or 'n/a')       # read right after the timed loops: an idle device reports its floor
    fmt = lambda v: 'n/a' if v is None else '%.1f' % v
    cell = lambda t: 'n/a' if not t else '%.1f (%.1f .. %.1f)' % (statistics.median(t), min(t), max(t))
    lines.append('%4s %26s %26s %26s %26s   %s' % ('N', '(a) parent_us', '(b) off_us', '(c) on_us', '(d) torch_us', 'launches a / b / c / d'))
    for n, reps, live in rows:                                        # the profiler only after every timing is taken
        counts = [fmt(launches(live[nm], a.count)) if nm in live else 'n/a' for nm in names]
        lines.append('%4d %26s %26s %26s %26s   %s' % (n, cell(reps.get('parent')), cell(reps['off']), cell(reps['on']), cell(reps['torch']),
                                                       ' / '.join(counts)))
        b_med, c_med, d_med = (statistics.median(reps[k]) for k in ('off', 'on', 'torch'))
        if 'parent' in reps:
            lo, hi = min(reps['parent']), max(reps['parent'])
            where = 'within' if lo <= b_med <= hi else ('BELOW' if b_med < lo else 'ABOVE')
            verdicts.append('# N %d condition 1: (b) %.1f us is %s the spread of (a) over %d repeats, %.1f .. %.1f us' % (n, b_med, where, a.repeats, lo, hi))
        else:
            verdicts.append('# N %d condition 1: not measured (no --parent)' % n)
        verdicts.append('# N %d condition 2: (c) %.1f us is %s (d) %.1f us (%.2fx)' % (n, c_med, 'below' if c_med < d_med else 'NOT BELOW', d_med, d_med / c_med))
    lines[4] = lines[4] % kind
    lines += verdicts
    print('\n'.join(lines), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
