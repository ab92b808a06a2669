"""Latency of one MeshEvaluator.update at the benchmark's call shape -- 32 images, 12 people each (one stranger prediction
and one unmatched ground truth in every fourth image), 14 joints -- without and with 6890-vertex PVE / PA-PVE, next to the
same scoring on the host: download of the predictions, then the numpy float64 restatement of tests/test_eval_metrics.py
(match2d_np, points_np: what the reference's per-image numpy / torch-CPU evaluation computes).

Median of --calls calls after --warmup, wall clock, each call ending with a device synchronisation.  Per device call the
script also records the library kernels it launches (counted from the C entries called: one kernel each), the aten
operators PyTorch dispatches around them (offsets, joint selection, buffer fills), and the host synchronisations: the call
runs under torch.cuda.set_sync_debug_mode('warn') and the warnings are counted (the library's own entries never synchronise).

    python scripts/eval_latency.py [--out profiles/eval_latency.txt]
"""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from romp_amd import evaluation as E  # noqa: E402
from romp_amd import lib as L  # noqa: E402
from test_eval_metrics import match2d_np, offsets, points_np, summary_np  # noqa: E402

B, PEOPLE, J, V = 32, 12, 14, 6890


def make_call(dev, with_verts, seed=0):
    """-> outputs, batch_ids, gts: device tensors of one call."""
    rng = np.random.default_rng(seed)
    g2, g3, gv, gb, p2, p3, pv, pb = [], [], [], [], [], [], [], []
    for b in range(B):
        for k in range(PEOPLE):
            c = np.array([120.0 + 160.0 * (k % 6), 200.0 + 300.0 * (k // 6)])
            kp = c + rng.standard_normal((J, 2)) * np.array([25.0, 50.0])
            j3 = rng.standard_normal((J, 3)) * np.array([0.2, 0.45, 0.15])
            v3 = rng.standard_normal((V, 3)) * np.array([0.2, 0.45, 0.15]) if with_verts else None
            if not (b % 4 == 0 and k == PEOPLE - 1):                      # (else: a person nobody predicted)
                p2.append(kp + 3.0 * rng.standard_normal((J, 2))); p3.append(j3 + 0.03 * rng.standard_normal((J, 3))); pb.append(b)
                if with_verts:
                    pv.append(v3 + 0.03 * rng.standard_normal((V, 3)))
            g2.append(kp); g3.append(j3); gb.append(b)
            if with_verts:
                gv.append(v3)
        if b % 4 == 0:                                                     # a stranger
            p2.append(np.array([1500.0, 900.0]) + rng.standard_normal((J, 2)) * 30.0); p3.append(rng.standard_normal((J, 3)) * 0.3); pb.append(b)
            if with_verts:
                pv.append(rng.standard_normal((V, 3)) * 0.3)
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(np.asarray(a), dt)).to(dev)
    out = {'kp2d': t(p2), 'joints': t(p3)}
    gts = {'kp2d': t(g2), 'kp3d': t(g3), 'batch_ids': t(gb, np.int64), 'B': B}
    if with_verts:
        out['verts'], gts['verts'] = t(pv), t(gv)
    return out, t(pb, np.int64), gts


class Counted(object):
    """Counts the library's scoring entries (one kernel launch each) and the aten operators dispatched meanwhile."""

    class _Ops(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.n += 1
            return func(*args, **(kwargs or {}))

    def __init__(self):
        self.kernels, self.ops, self._lib, self._saved = 0, self._Ops(), L.load(), {}

    def __enter__(self):
        for name in L.EVAL_EXPORTS:
            fn = getattr(self._lib, name)
            self._saved[name] = fn

            def counted(*args, _fn=fn):
                self.kernels += 1
                return _fn(*args)
            setattr(self._lib, name, counted)
        self.ops.__enter__()
        return self

    def __exit__(self, *exc):
        self.ops.__exit__(*exc)
        for name, fn in self._saved.items():
            setattr(self._lib, name, fn)


def host_scoring(out, bids, gts, with_verts):
    """Download, then the restatement: match -> points (-> points on the vertices) -> summary."""
    p2, p3, pb = out['kp2d'].cpu().numpy(), out['joints'].cpu().numpy(), bids.cpu().numpy()
    g2, g3, gb = gts['kp2d'].cpu().numpy(), gts['kp3d'].cpu().numpy(), gts['batch_ids'].cpu().numpy()
    gop, pog, _ = match2d_np(p2, offsets(pb, B), g2, np.ones(g2.shape[:2], bool), offsets(gb, B), max_pred=64, max_gt=64)
    r = points_np(p3, g3, pog, align_inds=[13])
    nan = np.full(len(pog), np.nan)
    rows = {'mpjpe': r['mpjpe'], 'pa_mpjpe': r['pa_mpjpe'], 'cmu_mpjpe': r['mpjpe_all'], 'pve': nan, 'pa_pve': nan}
    if with_verts:
        rv = points_np(out['verts'].cpu().numpy(), gts['verts'].cpu().numpy(), pog)
        rows['pve'], rows['pa_pve'] = rv['mpjpe'], rv['pa_mpjpe']
    return summary_np(rows, pog, gop)


def median_ms(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_latency.txt'))
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host_calls', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda:0')
    lines = ['# one MeshEvaluator.update, %d images x %d people, %d joints; median of %d calls after %d warm-up, ms, wall clock to a device'
             % (B, PEOPLE, J, a.calls, a.warmup),
             '# synchronise (%s).  host: download + numpy float64 restatement, median of %d.' % (torch.cuda.get_device_name(0), a.host_calls),
             '# kernels: library launches per device call; aten_ops: PyTorch operators dispatched around them; syncs: host synchronisations',
             '%-14s %6s %6s %10s %10s %8s %8s %6s  %s' % ('arrangement', 'n_pred', 'n_gt', 'device_ms', 'host_ms', 'kernels', 'aten_ops', 'syncs', 'agreement')]
    for name, with_verts in (('joints', False), ('joints+verts', True)):
        out, bids, gts = make_call(dev, with_verts)
        ev = E.MeshEvaluator(dev, joints=None, align_inds=[13], kp2d_key='kp2d')
        ev.update(out, bids, gts)
        dev_summary = ev.summary()
        host_summary = host_scoring(out, bids, gts, with_verts)
        worst, counts = 0.0, True
        for k, v in host_summary.items():
            if isinstance(v, int):
                counts = counts and dev_summary[k] == v
            elif v == v:
                worst = max(worst, abs(dev_summary[k] - v) / abs(v))
        with Counted() as c, warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                ev.update(out, bids, gts)
            finally:
                torch.cuda.set_sync_debug_mode('default')
        sync_warnings = [w for w in caught if 'ynchroniz' in str(w.message)]
        syncs = len(sync_warnings)
        for w in sync_warnings:                                            # where a synchronisation came from
            print('sync warning in %s: %s:%d: %s' % (name, w.filename, w.lineno, w.message), flush=True)
        d_ms = median_ms(lambda: ev.update(out, bids, gts), a.warmup, a.calls)
        h_ms = median_ms(lambda: host_scoring(out, bids, gts, with_verts), 1, a.host_calls)
        lines.append('%-14s %6d %6d %10.3f %10.1f %8d %8d %6d  %s, summary within %.1e of the host' %
                     (name, out['joints'].shape[0], gts['kp3d'].shape[0], d_ms, h_ms, c.kernels, c.ops.n, syncs,
                      'counts equal' if counts else 'COUNTS DIFFER', worst))
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
