"""ByteTrack-3D association of BEV's video mode on the device (csrc/track.hip, include/romp_hip_track.h).

``DeviceTracker`` is ``tracker.Tracker`` with its state in one device buffer: a frame is ONE launch, nothing is downloaded unless
the caller asks (``update_host``).  ``TrackedSmoother`` adds the OneEuro filters of ``temporal.OneEuroBank`` keyed by the tracker's
table slot: track -> smooth -> one download of the count and the ids.  ``smooth_batch`` does the same for the consecutive frames
of a ``BEV.forward_batch`` call, still in two launches.

One difference from the host classes, by design: a source that has seen more track ids than the filter bank has slots makes
``OneEuroBank`` clear ALL its filters (utils.py:253-254); here a filter lives exactly as long as its track, so nothing is cleared.

``python -m romp_amd.tracking --bench`` times one ``BEV.temporal_optimization`` with the host and with the device tracker.
"""
import ctypes as C

import numpy as np
import torch

from . import lib as L

MAX_DET = 256                                             # rows of one frame (ROMP_TRACK_MAX_DET)


class DeviceTracker(object):
    def __init__(self, device, capacity=256, det_thresh=0.12, low_conf_det_thresh=0.05, track_buffer=60, match_thresh=300,
                 frame_rate=30, first_id=0):
        self.device, self.capacity = torch.device(device), int(capacity)
        self.lib = L.load()
        nbytes = self.lib.romp_track_state_bytes(self.capacity)
        if nbytes < 0:
            L.check(nbytes)
        self.state = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)
        self.max_time_lost = int(frame_rate / 30.0 * track_buffer)
        with torch.cuda.device(self.device):
            L.check(self.lib.romp_track_init(L.ptr(self.state), self.capacity, int(first_id), float(det_thresh), float(low_conf_det_thresh),
                                             float(match_thresh), self.max_time_lost, 60., L.stream_ptr(self.device)))

    def _launch(self, points, scores, frame_rows, flags=None, stride=0):
        """-> one int32 buffer [count (T) | ids (T, cap) | rows (T, cap) | slots (T, cap)] and its four views."""
        frame_rows = [int(n) for n in frame_rows]
        T, cap = len(frame_rows), self.capacity
        if max(frame_rows, default=0) > MAX_DET:
            raise L.RompHipError('DeviceTracker: a frame of %d rows, at most %d' % (max(frame_rows), MAX_DET))
        assert points.dtype == torch.float32 and scores.dtype == torch.float32 and points.shape == (sum(frame_rows), 4) \
            and scores.shape == (sum(frame_rows),) and points.is_cuda
        points, scores = points.contiguous(), scores.contiguous()
        buf = torch.empty(T + 3 * T * cap, dtype=torch.int32, device=self.device)
        count, ids, rows, slots = buf[:T], buf[T:T + T * cap], buf[T + T * cap:T + 2 * T * cap], buf[T + 2 * T * cap:]
        if sum(frame_rows) == 0 and T >= 1:                         # nothing detected in the whole call: every frame is skipped
            count.zero_(); ids.fill_(-1); rows.zero_(); slots.fill_(-1)
        else:
            with torch.cuda.device(self.device):
                L.check(self.lib.romp_track_frames(L.ptr(self.state), L.ptr(points), L.ptr(scores), (C.c_int32 * max(T, 1))(*frame_rows), T,
                                                   L.ptr(count), L.ptr(ids), L.ptr(rows), L.ptr(slots), L.ptr(flags), int(stride),
                                                   L.stream_ptr(self.device)))
        return buf, count, ids.view(T, cap), rows.view(T, cap), slots.view(T, cap)

    def update_frames(self, points, scores, frame_rows):
        """T frames, the rows of frame t after those of frame t-1 -> device int32 (count (T), ids, rows, slots (T, capacity)); no sync."""
        return self._launch(points, scores, frame_rows)[1:]

    def update(self, points, scores):
        """One frame -> device int32 (count (1), ids, rows, slots (capacity)); no sync."""
        count, ids, rows, slots = self.update_frames(points, scores, [points.shape[0]])
        return count, ids[0], rows[0], slots[0]

    def update_host(self, points, scores):
        """One frame -> (ids, rows) lists exactly like Tracker.update; one download."""
        buf = self._launch(points, scores, [points.shape[0]])[0]
        host = buf[:1 + 2 * self.capacity].cpu().numpy()
        n = int(host[0])
        return host[1:1 + n].tolist(), host[1 + self.capacity:1 + self.capacity + n].tolist()

    def tracks(self):
        """-> (tracked, lost): float64 arrays (n, 14) in list order, a row = id, state, confirmed, frame, born, score, mean[8]."""
        rec = torch.empty(self.capacity, 14, dtype=torch.float64, device=self.device)
        cnt = torch.empty(2, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self.lib.romp_track_list(L.ptr(self.state), L.ptr(rec), L.ptr(cnt), L.stream_ptr(self.device)))
        nt, nl = cnt.cpu().tolist()
        rec = rec[:nt + nl].cpu().numpy()
        return rec[:nt], rec[nt:]

    def header(self):
        """The 32 int32 header words of the state (a download)."""
        return self.state[:16].cpu().numpy().view(np.int32)

    @property
    def overflow(self):
        """How many detections should have begun a track and found the table full (a download)."""
        return int(self.header()[5])


class TrackedSmoother(object):
    """The tracker's state and the OneEuro filter states of its table slots."""

    def __init__(self, device, smooth_coeff=3., n_betas=10, capacity=256, **tracker_args):
        self.device, self.smooth_coeff, self.n_betas, self.capacity = torch.device(device), float(smooth_coeff), int(n_betas), int(capacity)
        self.tracker = DeviceTracker(self.device, capacity=self.capacity, **tracker_args)
        self.lib = self.tracker.lib
        self.stride = self.lib.romp_oneeuro_state_floats(self.n_betas)
        self.filters = torch.zeros(self.capacity, self.stride, device=self.device)

    def run(self, points, scores, thetas, betas, cam, frame_rows=None):
        """Track, then smooth: two launches, no sync.  thetas (N,72), betas (N,n_betas), cam (N,3): the raw estimates of the rows of
        `points`.  -> (buf, count, ids, rows, slots, thetas_s, betas_s, cam_s): the int32 outputs of the tracker and the smoothed
        estimates of what it reported, padded: (T * capacity, .) rows, entry k of frame t at row t * capacity + k."""
        frame_rows = [points.shape[0]] if frame_rows is None else list(frame_rows)
        T, cap = len(frame_rows), self.capacity
        assert thetas.shape == (points.shape[0], 72) and betas.shape == (points.shape[0], self.n_betas) and cam.shape == (points.shape[0], 3)
        thetas, betas, cam = thetas.contiguous().float(), betas.contiguous().float(), cam.contiguous().float()
        buf, count, ids, rows, slots = self.tracker._launch(points, scores, frame_rows, self.filters, self.stride)
        f32 = dict(device=self.device, dtype=torch.float32)
        th, be, ca = torch.empty(T * cap, 72, **f32), torch.empty(T * cap, self.n_betas, **f32), torch.empty(T * cap, 3, **f32)
        if points.shape[0]:
            with torch.cuda.device(self.device):
                L.check(self.lib.romp_oneeuro_smooth_frames(L.ptr(self.filters), T, cap, L.ptr(count), L.ptr(rows), L.ptr(slots), self.n_betas,
                                                            self.smooth_coeff, L.ptr(thetas), L.ptr(betas), L.ptr(cam), L.ptr(th), L.ptr(be),
                                                            L.ptr(ca), L.stream_ptr(self.device)))
        return buf, count, ids, rows, slots, th, be, ca

    @staticmethod
    def download(buf, T, cap):
        """The ONE download of a call: -> (counts (T) , ids (T, cap)) as numpy int32."""
        host = buf[:T + T * cap].cpu().numpy()
        return host[:T], host[T:].reshape(T, cap)


def bev_tracking_points(cam, cam_trans, image_scale=128, depth_scale=30):
    """The (N,4) tracking points of BEV.temporal_optimization (bev/main.py:275-277) on the device: float32, the same operations in
    the same order as the numpy expression there."""
    return torch.cat([(cam[:, [2, 1]] + 1) * image_scale, cam_trans[:, [2]] * depth_scale, cam[:, [0]] * image_scale / 2], 1)


def smooth_batch(smoother, outputs):
    """Track and smooth the dict of ``BEV.forward_batch`` whose images are CONSECUTIVE FRAMES of one source (rows batch-major, as
    the parse returns them): the per-frame row counts come from ``pred_batch_ids`` (one small download), then two launches and the
    download of counts and ids.  -> the dict restricted to the rows of tracked persons, frame by frame, in the order the tracker
    reports them, with smoothed smpl_thetas / smpl_betas / cam, plus track_ids (numpy int32) and pred_batch_ids; None when no frame
    reports anybody.  Meshes in the dict (verts, joints) are those of the RAW parameters."""
    bids = outputs['pred_batch_ids']
    N = bids.shape[0]
    frame_rows = torch.bincount(bids).cpu().tolist()
    T, cap = len(frame_rows), smoother.capacity
    points = bev_tracking_points(outputs['cam'], outputs['cam_trans'])
    buf, count, ids, rows, slots, th, be, ca = smoother.run(points, outputs['center_confs'].float(), outputs['smpl_thetas'], outputs['smpl_betas'],
                                                            outputs['cam'], frame_rows)
    counts, ids_h = TrackedSmoother.download(buf, T, cap)
    if int(counts.sum()) == 0:
        return None
    padded = torch.as_tensor(np.concatenate([t * cap + np.arange(n) for t, n in enumerate(counts)]), dtype=torch.long, device=bids.device)
    src = rows.reshape(-1)[padded].long()
    res = {}
    for k, v in outputs.items():
        res[k] = v[src] if torch.is_tensor(v) and v.shape[:1] == (N,) else v
    res['smpl_thetas'], res['smpl_betas'], res['cam'] = th[padded], be[padded], ca[padded]
    res['track_ids'] = np.concatenate([ids_h[t, :n] for t, n in enumerate(counts)]).astype(np.int32)
    return res


# ------------------------------------------------------------------------------------------------ the latency of one frame
def _bench(frames=300, warmup=30, sizes=(1, 8, 64), seed=0):
    """Wall time of one BEV.temporal_optimization (synthetic detections, no network), host tracker against device tracker, the two
    taking turns frame by frame on the same sequence; each call timed from an idle device to an idle device."""
    import time
    from types import SimpleNamespace

    from . import bev, tracker
    dev = torch.device('cuda:0')
    keys = ['smpl_thetas', 'smpl_betas', 'cam', 'cam_trans', 'params_pred', 'center_confs', 'pred_batch_ids']
    lines = []
    for N in sizes:
        rs = np.random.RandomState(seed + N)
        settings = SimpleNamespace(show_largest=False, smooth_coeff=3., device_tracker=False)
        tracker.Track.last_id = 0
        host = SimpleNamespace(settings=settings, tdevice=dev, OE_filters={}, result_keys=keys, tracker=tracker.Tracker())
        devi = SimpleNamespace(settings=SimpleNamespace(show_largest=False, smooth_coeff=3., device_tracker=True), tdevice=dev, OE_filters={},
                               result_keys=keys, device_smoothers={})
        # persons on a grid a good way apart, drifting slowly: every one keeps its track
        g = int(np.ceil(np.sqrt(N)))
        base = np.stack([(np.arange(N) % g + 0.5) / g * 1.6 - 0.8, (np.arange(N) // g + 0.5) / g * 1.6 - 0.8], 1)
        scale = 0.3 + 0.4 * rs.rand(N)
        times = {'host': [], 'device': []}
        for f in range(warmup + frames):
            xy = base + 0.002 * f + 0.0005 * rs.randn(N, 2)
            cam = torch.tensor(np.concatenate([scale[:, None], xy[:, ::-1]], 1), dtype=torch.float32, device=dev)
            out = {'cam': cam, 'cam_trans': bev.denormalize_cam_params_to_trans(cam), 'smpl_thetas': torch.tensor(rs.randn(N, 72) * 0.2, dtype=torch.float32, device=dev),
                   'smpl_betas': torch.tensor(rs.randn(N, 11), dtype=torch.float32, device=dev), 'params_pred': torch.zeros(N, 146, device=dev),
                   'center_confs': torch.full((N,), 0.5, device=dev), 'pred_batch_ids': torch.zeros(N, dtype=torch.long, device=dev)}
            for name, obj in (('host', host), ('device', devi)) if f % 2 == 0 else (('device', devi), ('host', host)):
                o = dict(out)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = bev.BEV.temporal_optimization(obj, o, 0)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert res is not None and len(res['track_ids']) == N
                if f >= warmup:
                    times[name].append(dt * 1e3)
        for name in ('host', 'device'):
            a = np.asarray(times[name])
            lines.append('N = %2d  %-6s tracker: median %.3f ms, p10 %.3f, p90 %.3f (%d frames after %d warm-up)'
                         % (N, name, np.median(a), np.percentile(a, 10), np.percentile(a, 90), len(a), warmup))
    clock = None
    try:
        import glob
        for fn in glob.glob('/sys/class/drm/card*/device/pp_dpm_sclk'):
            for line in open(fn):
                if line.strip().endswith('*'):
                    clock = line.split(':')[1].strip().rstrip('*').strip()
    except Exception:  # noqa: BLE001
        pass
    head = ('one BEV.temporal_optimization, host clock from an idle device to an idle device, host and device tracker taking turns on the '
            'same frames (%s, torch %s, engine clock as the driver reports it after the loops: %s)'
            % (torch.cuda.get_device_name(0), torch.__version__, clock or 'not available'))
    return '\n'.join([head] + lines)


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--bench', action='store_true')
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.bench:
        text = _bench(frames=a.frames)
        print(text)
        if a.out:
            with open(a.out, 'w') as fh:
                fh.write(text + '\n')
