"""Latency of one step of a scene fit with the depth-order and collision terms (include/romp_hip_fit_scene.h) at 64 rows (8
scenes x 8 persons) and 512 rows (64 scenes x 8 persons), four columns and the new launch alone:

  (a) parent   the fitter step of the parent commit (smpl_forward, romp_fit_reproject, smpl_backward, romp_fit_adam), from a
               checkout of that commit with its own library, loaded beside this tree as a second package;
  (b) off      this tree's KeypointFitter with the scene weights set but scene = None: the same four entries;
  (c) on       this tree with the scene tables, depth labels and both terms on (the layer's 47 default spheres): (b) plus one
               romp_fit_scene launch;
  (d) torch    the objective of (c) in torch ops around the HIP SMPL autograd node (pairwise depth differences and sphere
               distances per scene as dense tensors), torch.optim.Adam;
  (e) scene    the romp_fit_scene launch of (c) alone, both terms.

The method is that of scripts/fit_prior_latency.py, whose helpers are used: device events around each step, median of --calls
steps after --warmup; (a) and (b) take turns with each other, then (c) and (d); --repeats repeats give the spread; kernels per
step are counted with torch.profiler after every timing is taken.  (b) against (a) is reported, not gated on.

    git worktree add ../romp_parent HEAD~1 && (cd ../romp_parent && python -m romp_amd.build)   # or any checkout of the parent
    python scripts/fit_scene_latency.py --parent ../romp_parent [--out profiles/fit_scene_latency.txt]
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
from romp_amd.fitting import KeypointFitter  # noqa: E402
from romp_amd.scene import body_spheres, scene_groups  # noqa: E402
from romp_amd.smpl import SMPL  # noqa: E402
from romp_amd.synthetic import make_smpl_model  # noqa: E402

W_BETAS = W_POSE = 1e-4
LR = 0.02
PERSONS = 8
THRESH = 0.3
SCENE = dict(w_depth_order=2., w_collision=1e-4, depth_loss_type='piecewise', dist_thresh=THRESH)


def torch_step(smpl, betas, poses, cam, poses0, kp, conf, ids, table, opt):
    """One step of the objective of (c) without the fused entries.  The rows are scene-major with PERSONS rows per scene, so
    a scene is a slice of a reshape; ids (scenes, PERSONS) are all labelled; table = (p, q, a, sigma^2) device tensors."""
    p, q, a, s2 = table
    opt.zero_grad()
    _, joints, _ = smpl(betas, poses)
    zero = torch.zeros((), device=joints.device)
    uv = joints[:, :, :2] * cam[:, None, 0:1] + cam[:, None, 1:]
    vis = (conf > 0) & (kp[:, :, 0] > -1.99) & (kp[:, :, 1] > -1.99)
    total = torch.where(vis, conf * conf * ((uv - kp) ** 2).sum(-1), zero).sum(1) / (vis.float().sum(1) + 1e-4)
    total = (total + W_BETAS * (betas ** 2).sum(1) + W_POSE * ((poses - poses0)[:, 3:] ** 2).sum(1)).sum()
    t = 2 * torch.stack([cam[:, 1] / cam[:, 0], cam[:, 2] / cam[:, 0], 1 / cam[:, 0]], 1)
    z = t[:, 2].reshape(-1, PERSONS)
    d, k = z[:, None, :] - z[:, :, None], ids[:, None, :] - ids[:, :, None]           # [scene, i, j]: j minus i
    upper = torch.triu(torch.ones(PERSONS, PERSONS, dtype=torch.bool, device=z.device), 1)[None]
    margin = d - k * THRESH
    active = upper & ((k == 0) | ((k < 0) & (margin > 0)) | ((k > 0) & (margin < 0)))
    term = torch.where(k == 0, d * d, torch.nn.functional.softplus(torch.where(k < 0, d, -d)))
    count = active.sum((1, 2))
    total = total + SCENE['w_depth_order'] * (torch.where(active, term, zero).sum((1, 2)) / count.clamp(min=1)).sum()
    c = ((1 - a)[None, :, None] * joints[:, p] + a[None, :, None] * joints[:, q] + t[:, None]).reshape(-1, PERSONS, p.numel(), 3)
    d2 = ((c[:, :, None, :, None, :] - c[:, None, :, None, :, :]) ** 2).sum(-1)          # [scene, n, m, s, u]
    e = torch.exp(-d2 / (s2[None, None, None, :, None] + s2[None, None, None, None, :]))
    other = ~torch.eye(PERSONS, dtype=torch.bool, device=z.device)[None, :, :, None, None]
    total = total + SCENE['w_collision'] * 0.5 * torch.where(other, e, zero).sum()
    total.backward()
    opt.step()


def variants(smpl, parent, scenes, dev):
    """-> {column: its step functions} for scenes x PERSONS rows in scene-major order, each on tensors of its own, and which
    Adam (d) runs.  (a) and (b) come twice, allocated a, b, b, a, as in scripts/fit_prior_latency.py."""
    n = scenes * PERSONS
    g = torch.Generator().manual_seed(n)
    frame = torch.arange(scenes).repeat_interleave(PERSONS)
    betas0 = torch.randn(n, 10, generator=g).to(dev)
    poses0 = (0.3 * torch.randn(n, 72, generator=g)).to(dev)
    cam0 = torch.cat([0.8 + 0.004 * torch.randn(n, 1, generator=g), 0.04 * torch.randn(n, 2, generator=g)], 1).to(dev)   # t within ~0.1
    kp = (0.5 * torch.randn(n, 71, 2, generator=g)).to(dev)
    conf = (0.2 + 0.8 * torch.rand(n, 71, generator=g)).to(dev)
    ids = torch.randint(0, 4, (n,), generator=g).to(dev)
    groups = scene_groups(frame.to(dev))
    sp = body_spheres(smpl)
    table = (torch.tensor(sp.p, device=dev), torch.tensor(sp.q, device=dev), torch.tensor(sp.a, device=dev),
             (torch.tensor(sp.r, device=dev) / 3) ** 2)

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
        return stepper(KeypointFitter(SMPL(make_smpl_model(0)).to(dev), **dict(args, **SCENE)).start(betas0, poses0, cam0, kp, conf, scene=None,
                                                                                                  depth_ids=ids))

    old = [make_old()] if parent is not None else []
    off = [make_off(), make_off()]
    old += [make_old()] if parent is not None else []
    run = KeypointFitter(smpl, **dict(args, **SCENE)).start(betas0, poses0, cam0, kp, conf, scene=groups, depth_ids=ids)
    assert run.scene_on and run.evaluate != run._evaluate_2d
    on = stepper(run)
    b, p, c = (x.clone().requires_grad_(True) for x in (betas0, poses0, cam0))
    ids2 = ids.reshape(-1, PERSONS)
    try:
        opt, kind = torch.optim.Adam([b, p, c], lr=LR, fused=True), 'fused=True'
        torch_step(smpl, b, p, c, poses0, kp, conf, ids2, table, opt)
        torch.cuda.synchronize()
    except Exception as exc:  # noqa: BLE001
        print('# Adam(fused=True) is not available here (%s): the default implementation runs' % str(exc).splitlines()[0], flush=True)
        b, p, c = (x.clone().requires_grad_(True) for x in (betas0, poses0, cam0))
        opt, kind = torch.optim.Adam([b, p, c], lr=LR), 'default (foreach)'

    def unfused():
        torch_step(smpl, b, p, c, poses0, kp, conf, ids2, table, opt)

    run.evaluate(0)                                                   # the joints the lone launch reads

    def scene_alone():
        run._scene(0)

    return {'parent': old, 'off': off, 'on': [on], 'torch': [unfused], 'scene': [scene_alone]}, kind


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
    names = ('parent', 'off', 'on', 'torch', 'scene')
    lines = ['# one step of a scene fit (betas, poses, weak camera; 71 keypoints with confidences; L2 priors; rows = scenes x %d persons, scene-major); device events, '
             'median of %d steps after %d warm-up per repeat, %d repeats, (a) and (b) taking turns and (c) and (d) taking turns, us (%s, torch %s, engine clock read '
             'once the loops are done, the device idle again: %s)' % (PERSONS, a.calls, a.warmup, a.repeats, torch.cuda.get_device_name(0), torch.__version__, 'CLOCK'),
             '# (a) parent: the parent commit\'s KeypointFitter step on its own library (%s)' % ('loaded beside this tree' if parent else 'NOT MEASURED: no --parent'),
             '# (b) off: this tree, the scene weights set but scene = None (smpl_forward + romp_fit_reproject + smpl_backward + romp_fit_adam)',
             '# (c) on: this tree with the scene tables, depth labels (piecewise) and the collision term on 47 spheres: (b) + romp_fit_scene once',
             '# (d) torch: the objective of (c) in torch ops around the SMPL autograd node + torch.optim.Adam(%s)',
             '# (e) scene: the romp_fit_scene launch of (c) alone',
             '# each cell: median over the repeats (lowest .. highest repeat); launches: kernels per step counted by torch.profiler']
    rows, kind, verdicts = [], None, []
    for scenes in (8, 64):
        n = scenes * PERSONS
        fns, kind = variants(smpl, parent, scenes, dev)
        live = [(nm, fns[nm][0]) for nm in names if fns[nm]]
        reps = {nm: [] for nm, _ in live}
        pair = fns['parent'][:1] + fns['off'] + fns['parent'][1:]      # a, b, b, a
        groups = [[(nm, fn) for fn in pair for nm in ('parent', 'off') if fn in fns[nm]], [('on', fns['on'][0]), ('torch', fns['torch'][0])],
                  [('scene', fns['scene'][0])]]
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
    lines.append('%4s %26s %26s %26s %26s %22s   %s' % ('rows', '(a) parent_us', '(b) off_us', '(c) on_us', '(d) torch_us', '(e) scene_us',
                                                        'launches a / b / c / d / e'))
    for n, reps, live in rows:
        counts = [fmt(launches(live[nm], a.count)) if nm in live else 'n/a' for nm in names]
        lines.append('%4d %26s %26s %26s %26s %22s   %s' % (n, cell(reps.get('parent')), cell(reps['off']), cell(reps['on']), cell(reps['torch']),
                                                            cell(reps['scene']), ' / '.join(counts)))
        b_med, c_med, d_med, e_med = (statistics.median(reps[k]) for k in ('off', 'on', 'torch', 'scene'))
        if 'parent' in reps:
            lo, hi = min(reps['parent']), max(reps['parent'])
            where = 'within' if lo <= b_med <= hi else ('below' if b_med < lo else 'above')
            verdicts.append('# rows %d: (b) %.1f us is %s the spread of (a) over %d repeats, %.1f .. %.1f us' % (n, b_med, where, a.repeats, lo, hi))
        verdicts.append('# rows %d: (c) %.1f us against (d) %.1f us (%.2fx); the scene launch alone, (e) %.1f us, is %.0f %% of the rest of the step (b)'
                        % (n, c_med, d_med, d_med / c_med, e_med, 100 * e_med / b_med))
    lines[4] = lines[4] % kind
    lines += verdicts
    print('\n'.join(lines), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
