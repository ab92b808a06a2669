"""Latency of BEV's crowd mode on one MI355X: milliseconds per frame through BEV.forward with --crowd (one pre-processing
launch for all crops, the network in chunks of max_batch, one SMPL-A call, the device merge), against the same crops as K
serial single-image BEV.forward calls (the reference's loop).  Synthetic weights and meshes (oracle generators), a random
frame, the center threshold chosen so that every crop sees a few people.  The engine clock is sampled (rocm-smi, read
only) while the timed loops run.

    python scripts/bev_crowd_latency.py [--iters 20] [--out profiles/bev_crowd_latency.txt]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class ClockSampler(threading.Thread):
    def __init__(self):
        super().__init__(daemon=True)
        self.mhz, self.stop = [], threading.Event()

    def run(self):
        while not self.stop.is_set():
            try:
                s = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=10).stdout
                m = re.search(r'sclk clock level: \S+ \((\d+)Mhz\)', s)
                if m:
                    self.mhz.append(int(m.group(1)))
            except (OSError, subprocess.SubprocessError):
                return
            self.stop.wait(0.5)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from oracle import bev_oracle as BO
    from oracle import romp_oracle as O
    from romp_amd import bev
    dev = torch.device('cuda:0')
    s = bev.bev_settings(['--crowd'])
    s.GPU = 0
    model = bev.BEV(s, state_dict=BO.make_bev_state_dict(0), smpla_model=O.make_synthetic_smpl(0, 11),
                    smil_model=O.make_synthetic_smpl(5, 10))
    sampler = ClockSampler()
    sampler.start()
    lines, rows = [], []
    for H, W in ((720, 2560), (1080, 2160)):
        frame = np.random.RandomState(H).randint(0, 256, (H, W, 3)).astype(np.uint8)
        pl = bev.crowd_pad_length(H, s.overlap_ratio)
        crops = bev.crowd_split_plan(H, W + 2 * pl, s.overlap_ratio)
        padded = np.zeros((H, W + 2 * pl, 3), np.uint8)
        padded[:, pl:pl + W] = frame
        crop_images = [np.ascontiguousarray(padded[t:b, l:r]) for l, r, t, b in crops]
        K = len(crops)
        parser = model.model.centermap_parser
        for thresh in (0.9995, 0.999, 0.995, 0.99, 0.95, 0.9, 0.5):     # a few people per crop
            parser.conf_thresh = thresh
            out = model.model(torch.stack([bev.img_preprocess_device(c, dev)[0][0] for c in crop_images]))
            if out is not None and out['cam'].shape[0] >= 2 * K:
                break
        n_det = 0 if out is None else out['cam'].shape[0]
        res = model(frame)
        n_kept = 0 if res is None else len(res['cam'])
        model.settings.crowd = True
        batched = timed(lambda: model(frame), a.iters)
        model.settings.crowd = False                                    # (the crops have aspect < 2: the normal path anyway)
        serial = timed(lambda: [model(c) for c in crop_images], max(3, a.iters // 4))
        model.settings.crowd = True
        row = {'frame': '%dx%d' % (H, W), 'crops': K, 'center_thresh': thresh, 'detections': n_det, 'merged': n_kept,
               'batched_ms_median': round(batched[0], 2), 'batched_ms_min': round(batched[1], 2),
               'serial_ms_median': round(serial[0], 2), 'serial_ms_min': round(serial[1], 2),
               'speedup': round(serial[0] / batched[0], 2)}
        rows.append(row)
        lines.append('%s: %d crops, %d detections -> %d merged; crowd forward %.2f ms (min %.2f), %d serial single-image '
                     'forwards %.2f ms (min %.2f): %.2fx' % (row['frame'], K, n_det, n_kept, batched[0], batched[1], K, serial[0],
                                                             serial[1], row['speedup']))
    sampler.stop.set()
    sampler.join(timeout=15)
    mhz = sorted(sampler.mhz)
    clock = 'engine clock during the timed loops: %s' % (
        'median %d MHz (min %d, max %d, %d samples)' % (mhz[len(mhz) // 2], mhz[0], mhz[-1], len(mhz)) if mhz else 'not sampled')
    lines.append(clock)
    text = '\n'.join(lines)
    print(text)
    print(json.dumps({'rows': rows, 'sclk_mhz': mhz}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n' + json.dumps({'rows': rows, 'sclk_mhz': mhz}) + '\n')


if __name__ == '__main__':
    main()
