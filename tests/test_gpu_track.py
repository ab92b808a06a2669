"""The device tracker (csrc/track.hip, romp_amd/tracking.py) against the host tracker it mirrors (romp_amd/tracker.py), the fixture
recorded from the reference's classes (golden/tracker_seq.npz) and the sequences of tests/track_cases.py.

Decisions (ids, rows, list order, states) are exact.  Means: 1e-6 absolute -- both sides are float64 on values <= ~1e3, the filter is
contractive, and 1e-6 sits a factor of ten below the 1e-5 perturbation to which tests/test_track_cases.py shows the decisions
insensitive.  The measured maximum is printed (DESIGN.md quotes it).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cases as TC  # noqa: E402

from romp_amd import tracker as HT  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'tracker_seq.npz')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cases():
    return {seq['name']: (seq,) + TC.run_host(seq) for seq in TC.sequences()}


def _tracker(dev, seq, capacity=256):
    from romp_amd.tracking import DeviceTracker
    return DeviceTracker(dev, capacity=capacity, det_thresh=0.12, low_conf_det_thresh=0.05, track_buffer=seq['track_buffer'], match_thresh=300,
                         frame_rate=30)


@pytest.mark.parametrize('case', [0, 1, 2, 3])
def test_golden_sequences(dev, case):
    from romp_amd.tracking import DeviceTracker
    g = np.load(GOLD)
    k = 'c%d_' % case
    points, scores = torch.from_numpy(g[k + 'points']).to(dev), torch.from_numpy(g[k + 'scores']).to(dev)
    trk = DeviceTracker(dev)
    ids_all, inds_all, n_out, at = [], [], [], 0
    for n in g[k + 'n_det'].tolist():
        if n == 0:
            n_out.append(0)
            continue
        ids, inds = trk.update_host(points[at:at + n], scores[at:at + n])
        at += n
        ids_all += ids
        inds_all += inds
        n_out.append(len(ids))
    assert np.array_equal(n_out, g[k + 'n_out'])
    assert np.array_equal(ids_all, g[k + 'ids'])
    assert np.array_equal(inds_all, g[k + 'inds'])
    assert trk.overflow == 0


@pytest.mark.parametrize('n', TC.SIZES)
def test_sequences_frame_by_frame(dev, cases, n):
    seq, outs, lists, _ = cases['n%d_s0' % n]
    trk = _tracker(dev, seq)
    points, scores = torch.from_numpy(seq['points']).to(dev), torch.from_numpy(seq['scores']).to(dev)
    at, worst = 0, 0.
    for f, k in enumerate(seq['n_det']):
        ids, rows = trk.update_host(points[at:at + k], scores[at:at + k])
        at += k
        assert (ids, rows) == (list(outs[f][0]), list(outs[f][1])), (f, ids, rows, outs[f])
        tracked, lost = trk.tracks()
        for got, want in ((tracked, lists[f][0]), (lost, lists[f][1])):
            assert got[:, 0].astype(int).tolist() == [w[0] for w in want], f
            assert got[:, 1].astype(int).tolist() == [w[1] for w in want], f
            if len(want):
                worst = max(worst, float(np.abs(got[:, 6:] - np.stack([w[2] for w in want])).max()))
    print('%s: %d frames, max |mean - host mean| = %.3e' % (seq['name'], len(seq['n_det']), worst))
    assert worst < 1e-6
    assert trk.overflow == 0 and trk.header()[1] == sum(1 for k in seq['n_det'] if k)


def _scratch_free(state):
    """The state bytes without the staging area of the row counts (int32 words 32 .. 32 + 1024), which only a multi-frame call writes."""
    w = state.cpu().numpy().view(np.int32)
    return np.concatenate([w[:32], w[32 + 1024:]])


@pytest.mark.parametrize('n', [16, 57])
def test_one_launch_equals_frame_by_frame(dev, cases, n):
    seq = cases['n%d_s0' % n][0]
    points, scores = torch.from_numpy(seq['points']).to(dev), torch.from_numpy(seq['scores']).to(dev)
    one, many = _tracker(dev, seq), _tracker(dev, seq)
    count, ids, rows, slots = (t.cpu().numpy() for t in one.update_frames(points, scores, seq['n_det']))
    at = 0
    for f, k in enumerate(seq['n_det']):
        c, i, r, s = (t.cpu().numpy() for t in many.update(points[at:at + k], scores[at:at + k]))
        assert c[0] == count[f]
        assert np.array_equal(i, ids[f]) and np.array_equal(s, slots[f])
        assert np.array_equal(r[:c[0]] + at, rows[f, :c[0]])                    # (absolute rows)
        at += k
    assert np.array_equal(_scratch_free(one.state), _scratch_free(many.state))
    assert count.sum() > 0


SHAPES = [(1, 1), (1, 5), (5, 1), (63, 64), (64, 64), (65, 64), (64, 130), (256, 256)]


def _padded_total(cost, limit, pair):
    n, m = cost.shape
    k = int((pair >= 0).sum())
    return float(cost[np.arange(n)[pair >= 0], pair[pair >= 0]].sum() + (n - k) * limit / 2. + (m - k) * limit / 2.)


def _device_assign(dev, cost, limit):
    from romp_amd import lib as L
    h = L.load()
    n, m = cost.shape
    c = torch.from_numpy(np.ascontiguousarray(cost)).to(dev)
    out = torch.full((n,), -7, dtype=torch.int32, device=dev)
    L.check(h.romp_track_assign(L.ptr(c), n, m, float(limit), L.ptr(out), L.stream_ptr(dev)))
    return out.cpu().numpy()


@pytest.mark.parametrize('n,m', SHAPES)
def test_assign_alone(dev, n, m):
    rs = np.random.RandomState(100 * n + m)
    cost, limit = rs.uniform(0, 600, (n, m)), 300.
    pairs, _, _ = HT.assign(cost, limit)
    want = np.full(n, -1)
    want[pairs[:, 0]] = pairs[:, 1]
    best = _padded_total(cost, limit, want)
    if n * m <= 65 * 64:                                  # the optimum is unique by a margin: forbid each chosen pair in turn and re-solve
        for r, c in pairs:
            alt = cost.copy()
            alt[r, c] = 1e9
            p2, _, _ = HT.assign(alt, limit)
            w2 = np.full(n, -1)
            w2[p2[:, 0]] = p2[:, 1]
            assert _padded_total(alt, limit, w2) > best + 1e-9
    got = _device_assign(dev, cost, limit)
    assert np.array_equal(got, want)
    assert abs(_padded_total(cost, limit, got) - best) <= 1e-12 * abs(best)
    # every cost above the limit: nobody is paired
    assert (_device_assign(dev, cost + 300.5, limit) == -1).all()
    assert len(HT.assign(cost + 300.5, limit)[0]) == 0


def test_full_table(dev):
    """Capacity 4, 8 persons far apart: the first four get tracks, the others overflow on every frame; no fault, and the four tracks
    carry the ids the host gives the same persons."""
    rs = np.random.RandomState(5)
    base = np.stack([np.arange(8) * 2000., np.zeros(8), np.full(8, 200.), np.full(8, 40.)], 1)
    seq = {'track_buffer': 4}
    trk = _tracker(dev, seq, capacity=4)
    HT.Track.last_id = 0
    host = HT.Tracker(track_buffer=4)
    for f in range(6):
        pts = (base + f * np.array([3., 2., 0.5, 0.]) + rs.randn(8, 4)).astype(np.float32)
        sc = np.full(8, 0.6, np.float32)
        hi, hr = host.update(pts, sc)
        di, dr = trk.update_host(torch.from_numpy(pts).to(dev), torch.from_numpy(sc).to(dev))
        assert len(di) == 4 and set(zip(di, dr)) <= set(zip(hi, hr)) and sorted(di) == [1, 2, 3, 4], (f, di, dr, hi, hr)
    assert trk.overflow == 6 * 4
    tracked, lost = trk.tracks()
    assert len(tracked) == 4 and len(lost) == 0


def test_smooth_frames_equals_the_bank(dev, cases):
    """romp_oneeuro_smooth_frames after romp_track_frames, frame by frame and as ONE call over the sequence, against OneEuroBank.smooth
    driven with the ids and rows the tracker reports: equal bits."""
    from romp_amd.temporal import OneEuroBank
    from romp_amd.tracking import TrackedSmoother
    seq = cases['n16_s0'][0]
    rs = np.random.RandomState(3)
    N = len(seq['scores'])
    points, scores = torch.from_numpy(seq['points']).to(dev), torch.from_numpy(seq['scores']).to(dev)
    th = torch.from_numpy((rs.randn(N, 72) * 0.3).astype(np.float32)).to(dev)
    be = torch.from_numpy(rs.randn(N, 11).astype(np.float32)).to(dev)
    ca = torch.from_numpy(rs.randn(N, 3).astype(np.float32)).to(dev)
    args = dict(det_thresh=0.12, low_conf_det_thresh=0.05, track_buffer=seq['track_buffer'], match_thresh=300, frame_rate=30)
    cap = 32                                                                    # small enough that slots are begun again within the call
    step, whole, bank = TrackedSmoother(dev, 3., 11, cap, **args), TrackedSmoother(dev, 3., 11, cap, **args), OneEuroBank(dev, 3., 11, 256)
    T = len(seq['n_det'])
    buf, _, _, rows_w, slots_w, th_w, be_w, ca_w = whole.run(points, scores, th, be, ca, seq['n_det'])
    counts_w, ids_w = whole.download(buf, T, cap)
    rows_w, slots_w = rows_w.cpu().numpy(), slots_w.cpu().numpy()
    at, reported, reused = 0, 0, 0
    slot_owner = {}
    for f, k in enumerate(seq['n_det']):
        sl = slice(at, at + k)
        buf, _, _, rows, slots, t1, b1, c1 = step.run(points[sl], scores[sl], th[sl], be[sl], ca[sl])
        counts, ids = step.download(buf, 1, cap)
        n = int(counts[0])
        assert n == counts_w[f] and np.array_equal(ids[0], ids_w[f]) and np.array_equal(slots.cpu().numpy()[0], slots_w[f])
        if n:
            r = rows[0, :n].long()
            want = bank.smooth(ids[0, :n].tolist(), th[sl][r].contiguous(), be[sl][r].contiguous(), ca[sl][r].contiguous())
            for got1, gotw, w in zip((t1, b1, c1), (th_w, be_w, ca_w), want):
                assert torch.equal(got1[:n], w), f
                assert torch.equal(gotw[f * cap:f * cap + n], w), f
            for i, s in zip(ids[0, :n].tolist(), slots_w[f, :n].tolist()):
                reused += slot_owner.get(s, i) != i
                slot_owner[s] = i
        reported += n
        at += k
    assert torch.equal(step.filters, whole.filters)
    assert step.tracker.overflow == 0 and reported > 100 and reused > 0, (reported, reused)
    assert np.array_equal(_scratch_free(step.tracker.state), _scratch_free(whole.tracker.state))


def test_bev_tracking_points(dev):
    from romp_amd.tracking import bev_tracking_points
    rs = np.random.RandomState(0)
    cams, cam_trans = rs.randn(9, 3).astype(np.float32), (rs.randn(9, 3) * 3).astype(np.float32)
    want = np.concatenate([(cams[:, [2, 1]] + 1) * 128, cam_trans[:, [2]] * 30, cams[:, [0]] * 128 / 2], 1)
    got = bev_tracking_points(torch.from_numpy(cams).to(dev), torch.from_numpy(cam_trans).to(dev))
    assert got.dtype == torch.float32 and want.dtype == np.float32 and np.array_equal(got.cpu().numpy(), want)


def test_invalid_arguments_launch_nothing(dev):
    from romp_amd import lib as L
    from romp_amd.tracking import DeviceTracker
    h = L.load()
    trk = DeviceTracker(dev, capacity=8)
    pts = torch.tensor([[10., 10., 100., 30.]], device=dev)
    sc = torch.tensor([0.5], device=dev)
    trk.update(pts, sc)
    torch.cuda.synchronize()
    before = trk.state.clone()
    out = torch.full((4 * 8 + 4,), -9, dtype=torch.int32, device=dev)
    p = L.ptr(out)
    st = L.stream_ptr(dev)
    bad = (C.c_int32 * 2)(1, 257)
    assert h.romp_track_frames(L.ptr(trk.state), L.ptr(pts), L.ptr(sc), bad, 2, p, p, p, p, None, 0, st) == -1
    assert h.romp_track_frames(L.ptr(trk.state), L.ptr(pts), L.ptr(sc), bad, 0, p, p, p, p, None, 0, st) == -1
    assert h.romp_track_frames(L.ptr(trk.state), None, L.ptr(sc), bad, 1, p, p, p, p, None, 0, st) == -1
    assert h.romp_track_frames(L.ptr(trk.state), L.ptr(pts), L.ptr(sc), bad, 1, p, p, p, p, p, 0, st) == -1
    assert h.romp_track_init(L.ptr(trk.state), 0, 0, 0.12, 0.05, 300., 60, 60., st) == -1
    assert h.romp_track_init(L.ptr(trk.state), 8, 0, 0.12, 0.05, -1., 60, 60., st) == -1
    assert h.romp_track_assign(L.ptr(trk.state), 0, 4, 10., p, st) == -1 and b'romp_track_assign' in h.romp_last_error()
    assert h.romp_track_assign(L.ptr(trk.state), 4, 600, 10., p, st) == -1
    assert h.romp_track_list(L.ptr(trk.state), None, p, st) == -1
    assert h.romp_oneeuro_smooth_frames(L.ptr(trk.state), 1, 0, p, p, p, 10, 3., p, p, p, p, p, p, st) == -1
    torch.cuda.synchronize()
    assert torch.equal(trk.state.view(torch.int64), before.view(torch.int64)) and bool((out == -9).all())
    with pytest.raises(L.RompHipError):
        DeviceTracker(dev, capacity=513)
    # a call whose frames are all empty launches nothing and reports nobody
    count, ids, rows, slots = trk.update_frames(pts[:0], sc[:0], [0, 0])
    torch.cuda.synchronize()
    assert count.tolist() == [0, 0] and torch.equal(trk.state.view(torch.int64), before.view(torch.int64))
