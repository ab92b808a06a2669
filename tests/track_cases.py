"""Seeded detection sequences for the tracker tests (a helper, not a conftest): persons moving with constant velocity plus noise,
scripted so that every branch of ``romp_amd.tracker.Tracker.update`` is taken somewhere in the set:

  births after frame 1, deaths, an occlusion shorter and one longer than the buffer, confidence dips into (0.05, 0.12) and below
  0.05, scores exactly float32(0.12) and float32(0.05), a frame with no strong detection, a frame with no detection above 0.05,
  an empty frame, a spurious one-frame detection (a tentative track that is removed), a jump with low-score ghosts on the
  way (a track reported for a row it was not matched to), two persons crossing within 60 px, and a person passing within 60 px
  of an occluded one (a duplicate kill).

``run_host`` replays a sequence through the host tracker and counts those branches by watching its lists.
"""
import numpy as np

from romp_amd import tracker as T

SIZES = (1, 4, 16, 57, 98)
TRACK_BUFFER = 4
F32 = np.float32


def make_sequence(n, seed=0, frames=56, track_buffer=TRACK_BUFFER):
    """-> dict(points (sum N, 4) float32, scores (sum N) float32, n_det (frames) int, track_buffer)."""
    rs = np.random.RandomState(1000 * seed + n)
    extras = 4 if n >= 16 else 0
    nb = n - extras
    g = int(np.ceil(np.sqrt(nb)))
    idx = np.arange(nb)
    pos0 = np.stack([(idx % g) * 420. + 200 + rs.uniform(-60, 60, nb), (idx // g) * 420. + 200 + rs.uniform(-60, 60, nb),
                     150 + 250 * rs.rand(nb), 25 + 35 * rs.rand(nb)], 1)
    vel = rs.randn(nb, 4) * np.array([3., 3., 1., 0.1])
    k = min(nb, 5)
    roles = [{r for r in range(3, 8) if r % k == i % k} | ({1} if i % 8 == 1 and nb > 1 else set()) | ({2} if i % 8 == 2 and nb > 2 else set())
             for i in range(nb)]
    sigma = np.array([1.5, 1.5, 0.5, 0.05])
    short_gap, long_gap = (10, 10 + track_buffer - 1), (30, 30 + track_buffer + 4)
    pts, scs, n_det = [], [], []
    for f in range(frames):
        P, S = [], []
        for i in range(nb):
            r = roles[i]
            if 1 in r and f < 5 + i % 7:
                continue
            if 2 in r and f >= 20 + i % 9:
                continue
            if 3 in r and short_gap[0] <= f < short_gap[1]:
                continue
            if 4 in r and long_gap[0] <= f < long_gap[1]:
                continue
            p = pos0[i] + vel[i] * f + rs.randn(4) * sigma
            s = 0.3 + 0.6 * rs.rand()
            if 5 in r and f in (16, 17):
                s = 0.08 + 0.01 * rs.rand()
            if 5 in r and f == 22:
                s = 0.03
            if 6 in r and f in (9, 41):
                s = float(F32(0.12))
            if 6 in r and f in (13, 43):
                s = float(F32(0.05))
            if 7 in r and f in (7, 20, 45):
                for a in (0.5, 0.75, 0.9):                              # the detection jumps; low-score ghosts part of the way, where
                    P.append(p + a * np.array([40., 40., 0., 0.])); S.append(0.03)   # the filtered position will be
                p = p + np.array([40., 40., 0., 0.])
            P.append(p); S.append(s)
        if extras:
            base = np.array([g * 420. + 400, 300., 200., 40.])
            # C stands still and is occluded for track_buffer frames; D walks past within 30 px of it meanwhile, 100 deeper
            if not 14 <= f < 14 + track_buffer:
                P.append(base + rs.randn(4) * sigma); S.append(0.7)
            P.append(base + np.array([(f - 15.5) * 25., 30., 100., 0.]) + rs.randn(4) * sigma); S.append(0.8)
            # E and F cross each other, both seen, 80 apart in depth
            P.append(base + np.array([(f - 28) * 9., 900. + (f - 28) * 2., 0., 5.]) + rs.randn(4) * sigma); S.append(0.6)
            P.append(base + np.array([-(f - 28) * 9., 900. - (f - 28) * 2., 80., -5.]) + rs.randn(4) * sigma); S.append(0.65)
        if f in (6, 19):                                                   # a spurious strong detection far from everybody
            P.append(np.array([-2500., -2500. - 40 * f, 500., 30.])); S.append(0.5)
        P, S = np.asarray(P, np.float64).reshape(-1, 4), np.asarray(S, np.float64)
        if f == 24:
            S = np.full(len(S), 0.08) + 0.001 * rs.rand(len(S))             # no strong detection, all weak
        if f == 36:
            S = np.full(len(S), 0.02)                                       # nothing above the low threshold
        if f == 26:
            P, S = P[:0], S[:0]                                             # an empty frame
        order = rs.permutation(len(S))
        pts.append(P[order]); scs.append(S[order]); n_det.append(len(S))
    return {'points': np.concatenate(pts).astype(F32), 'scores': np.concatenate(scs).astype(F32), 'n_det': n_det,
            'track_buffer': track_buffer, 'name': 'n%d_s%d' % (n, seed)}


def sequences():
    return [make_sequence(n) for n in SIZES]


def perturbed(seq, rel=1e-5, seed=7):
    rs = np.random.RandomState(seed)
    out = dict(seq)
    out['points'] = (seq['points'].astype(np.float64) * (1 + rel * rs.uniform(-1, 1, seq['points'].shape))).astype(F32)
    return out


def frames_of(seq):
    at = 0
    for n in seq['n_det']:
        yield seq['points'][at:at + n], seq['scores'][at:at + n]
        at += n


def run_host(seq, first_id=0):
    """-> (per-frame (ids, rows), per-frame (tracked, lost) lists of (id, state, mean[8]), branch counts).  Empty frames are skipped
    as the callers of the tracker skip them: ([], []) and the lists of the frame before."""
    T.Track.last_id = first_id
    trk = T.Tracker(det_thresh=0.12, low_conf_det_thresh=0.05, track_buffer=seq['track_buffer'], match_thresh=300, frame_rate=30)
    stats = dict(weak_frames=0, revived=0, removed_tentative=0, timed_out=0, duplicate_kills=0, other_row=0, no_strong=0, empty=0)
    matched = {}
    inner = T.Track.absorb

    def absorb(self, det, frame):
        matched[self.tid] = det.z0.copy()
        return inner(self, det, frame)

    T.Track.absorb = absorb
    outs, lists, known = [], [], {}
    snap = lambda: ([(t.tid, t.state, t.mean.copy()) for t in trk.tracked_stracks], [(t.tid, t.state, t.mean.copy()) for t in trk.lost_stracks])
    try:
        for pts, sc in frames_of(seq):
            if len(sc) == 0:
                stats['empty'] += 1
                outs.append(([], []))
                lists.append(snap())
                continue
            stats['weak_frames'] += bool(((sc > F32(0.05)) & (sc < F32(0.12))).any())
            stats['no_strong'] += not (sc > F32(0.12)).any()
            lost_before = {t.tid for t in trk.lost_stracks}
            tent_before = [t for t in trk.tracked_stracks if not t.confirmed]
            lost_objs = list(trk.lost_stracks)
            timed_before = {t.tid for t in trk.lost_stracks if t.state == T.REMOVED}
            matched.clear()
            ids, rows = trk.update(pts, sc)
            for t in trk.tracked_stracks + trk.lost_stracks:
                known[t.tid] = t
            stats['revived'] += len(lost_before & {t.tid for t in trk.tracked_stracks})
            stats['removed_tentative'] += sum(t.state == T.REMOVED for t in tent_before)
            stats['timed_out'] += sum(t.state == T.REMOVED and t.tid not in timed_before for t in lost_objs)
            listed = {t.tid for t in trk.tracked_stracks + trk.lost_stracks}
            for tid, t in list(known.items()):
                if tid not in listed:
                    if t.state in (T.TRACKED, T.LOST):                   # gone without having been removed: killed as a duplicate
                        stats['duplicate_kills'] += 1
                    del known[tid]
            for tid, row in zip(ids, rows):
                if tid in matched and not np.array_equal(matched[tid], pts[row]):
                    stats['other_row'] += 1
            outs.append((ids, rows))
            lists.append(snap())
    finally:
        T.Track.absorb = inner
    return outs, lists, stats
