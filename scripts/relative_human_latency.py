"""Latency of one RelativeHumanEvaluator.update at the benchmark's call shape -- 32 images, 12 people each (one stranger
prediction and one unmatched ground truth in every fourth image), 14 joints, depth ids 0..3 and ages -1..3 -- next to the same
scoring on the host: download of the predictions, then the numpy restatement of tests/test_eval_metrics.py (match2d_np) and
tests/test_relative_human.py (score_np, summary_np: what the reference's per-image, per-pair evaluation computes).

Median of --calls calls after --warmup, wall clock, each call ending with a device synchronisation.  Per device call the
script also records the library kernels it launches (counted from the C entries called: one kernel each), the aten operators
PyTorch dispatches around them, and the host synchronisations: the call runs under torch.cuda.set_sync_debug_mode('warn') and
the warnings are counted (the library's own entries never synchronise).

    python scripts/relative_human_latency.py [--out profiles/relative_human_latency.txt]
"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from romp_amd import lib as L  # noqa: E402
from romp_amd import relative_human as R  # noqa: E402
from eval_latency import Counted, median_ms  # noqa: E402
from test_eval_metrics import match2d_np, offsets  # noqa: E402
from test_relative_human import score_np, summary_np  # noqa: E402

B, PEOPLE, J = 32, 12, 14


def make_call(dev, seed=0):
    """-> outputs, batch_ids, gts: device tensors of one call."""
    rng = np.random.default_rng(seed)
    g2, gd, ga, gb, p2, pd, pb = [], [], [], [], [], [], []
    for b in range(B):
        for k in range(PEOPLE):
            c = np.array([120.0 + 160.0 * (k % 6), 200.0 + 300.0 * (k // 6)])
            kp = c + rng.standard_normal((J, 2)) * np.array([25.0, 50.0])
            did = int(rng.integers(0, 4))
            if not (b % 4 == 0 and k == PEOPLE - 1):                      # (else: a person nobody predicted)
                p2.append(kp + 12.0 * rng.standard_normal((J, 2))); pd.append(1.0 + 0.5 * did + 0.3 * rng.standard_normal()); pb.append(b)
            g2.append(kp); gd.append(did); ga.append(int(rng.integers(-1, 4))); gb.append(b)
        if b % 4 == 0:                                                     # a stranger
            p2.append(np.array([1500.0, 900.0]) + rng.standard_normal((J, 2)) * 30.0); pd.append(5.0); pb.append(b)
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(np.asarray(a), dt)).to(dev)
    out = {'kp2d': t(p2), 'depth': t(pd)}
    gts = {'kp2d': t(g2), 'depth_id': t(gd, np.int32), 'age': t(ga, np.int32), 'batch_ids': t(gb, np.int64), 'B': B}
    return out, t(pb, np.int64), gts


class CountedEntries(Counted):
    """eval_latency.Counted over a given list of the library's entries."""

    def __init__(self, names):
        super().__init__()
        self.names = list(names)

    def __enter__(self):
        for name in self.names:
            fn = getattr(self._lib, name)
            self._saved[name] = fn

            def counted(*args, _fn=fn):
                self.kernels += 1
                return _fn(*args)
            setattr(self._lib, name, counted)
        self.ops.__enter__()
        return self


def host_scoring(out, bids, gts):
    """Download, then the restatement: match -> score -> summary."""
    p2, pd, pb = out['kp2d'].cpu().numpy(), out['depth'].cpu().numpy(), bids.cpu().numpy()
    g2, gd, ga, gb = (gts[k].cpu().numpy() for k in ('kp2d', 'depth_id', 'age', 'batch_ids'))
    goff = offsets(gb, B)
    gop, pog, _ = match2d_np(p2, offsets(pb, B), g2, np.ones(g2.shape[:2], bool), goff, max_pred=64, max_gt=64)
    pckh, cv, counts = score_np(p2, pd, g2, gd, ga, pog, goff)
    return summary_np(pckh, counts, gop, pog)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'relative_human_latency.txt'))
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host_calls', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    lines = ['# one RelativeHumanEvaluator.update, %d images x %d people, %d joints; median of %d calls after %d warm-up, ms, wall clock to a'
             % (B, PEOPLE, J, a.calls, a.warmup),
             '# device synchronise (%s).  host: download + numpy restatement, median of %d.' % (torch.cuda.get_device_name(0), a.host_calls),
             '# kernels: library launches per device call; aten_ops: PyTorch operators dispatched around them; syncs: host synchronisations',
             '%-14s %6s %6s %6s %10s %10s %8s %8s %6s  %s' % ('arrangement', 'n_pred', 'n_gt', 'pairs', 'device_ms', 'host_ms', 'kernels', 'aten_ops',
                                                            'syncs', 'agreement')]
    out, bids, gts = make_call(dev)
    ev = R.RelativeHumanEvaluator(dev, kp2d_key='kp2d', depth_key='depth')
    ev.update(out, bids, gts)
    dev_summary, host_summary = ev.summary(), host_scoring(out, bids, gts)
    worst, counts = 0.0, set(dev_summary) == set(host_summary)
    for k, v in host_summary.items():
        if isinstance(v, (int, list)):
            counts = counts and dev_summary[k] == v
        elif v == v:
            worst = max(worst, abs(dev_summary[k] - v) / abs(v))
    with CountedEntries(L.EVAL_EXPORTS + L.RH_EXPORTS) as c, warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            ev.update(out, bids, gts)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    # (PyTorch announces the debug mode itself with a 'prototype feature' warning once per process: not a synchronisation)
    sync_warnings = [w for w in caught if 'ynchroniz' in str(w.message) and 'prototype feature' not in str(w.message)]
    for w in sync_warnings:                                                # where a synchronisation came from
        print('sync warning: %s:%d: %s' % (w.filename, w.lineno, w.message), flush=True)
    d_ms = median_ms(lambda: ev.update(out, bids, gts), a.warmup, a.calls)
    h_ms = median_ms(lambda: host_scoring(out, bids, gts), 1, a.host_calls)
    lines.append('%-14s %6d %6d %6d %10.3f %10.1f %8d %8d %6d  %s, summary within %.1e of the host' %
                 ('relative_human', out['kp2d'].shape[0], gts['kp2d'].shape[0], host_summary['pairs_eq'] + host_summary['pairs_ordered'], d_ms, h_ms,
                  c.kernels, c.ops.n, len(sync_warnings), 'counts equal' if counts else 'COUNTS DIFFER', worst))
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
