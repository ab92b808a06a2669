"""Seeded detection sequences for the tracker tests (a helper, not a conftest): persons moving with constant velocity plus noise,
scripted so that every branch of ``romp_amd.tracker.Tracker.update`` is taken somewhere in the set:

  births after frame 1, deaths, an occlusion shorter and one longer than the buffer, confidence dips into (0.05, 0.12) and below
  0.05, scores exactly float32(0.12) and float32(0.05), a frame with no strong detection, a frame with no detection above 0.05,
  an empty frame, a spurious one-frame detection (a tentative track that is removed), a jump with low-score ghosts on the
  way (a track reported for a row it was not matched to), two persons crossing within 60 px, and a person passing within 60 px
  of an occluded one (a duplicate kill).

``run_host`` replays a sequence through the host tracker and counts those branches by watching its lists.

``edge_sequences``, ``nonfinite_sequences`` and ``longest_call`` (further down) are scripted apart, one path each: a revival after
the time-out and the `dropped` bookkeeping that follows it, a duplicate at equal age, equal rows in the nearest-detection search,
frames and tables at their caps, the longest call, non-finite rows.  ``SIZES`` and ``sequences()`` are not touched by them.
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
    if 'host_points' in seq:
        out['host_points'] = (seq['host_points'].astype(np.float64) * (1 + rel * rs.uniform(-1, 1, seq['points'].shape))).astype(F32)
    return out


def frames_of(seq, host=False):
    """The frames of a sequence; host=True: what the host tracker is given where that differs (`nonfinite_sequences`)."""
    points = seq['host_points'] if host and 'host_points' in seq else seq['points']
    at = 0
    for n in seq['n_det']:
        yield points[at:at + n], seq['scores'][at:at + n]
        at += n


# ------------------------------------------------------------------------------------------------ edge sequences
# Scripted persons a long way apart (>= 1000 in x or y: more than 3 match_thresh, so that no association round can confuse two of
# them), so that each sequence takes ONE path of Tracker.update that `sequences()` never takes; run_host counts those paths.
SIGMA = np.array([1.5, 1.5, 0.5, 0.05])
FAR = 3 * 300.                                                            # (the widest association round: 3 match_thresh)


def _person(x, y, seen, z=200., h=40., vel=(0., 0., 0., 0.), score=0.7):
    return {'pos': np.array([x, y, z, h], np.float64), 'vel': np.asarray(vel, np.float64), 'seen': seen, 'score': score}


def _frames(persons, frames, seed):
    """-> [(points list, scores list)] per frame, the persons in their order; a person is seen in [a, b) for (a, b) in seen."""
    rs = np.random.RandomState(seed)
    out = []
    for f in range(frames):
        P, S = [], []
        for p in persons:
            if any(a <= f < b for a, b in p['seen']):
                P.append(p['pos'] + p['vel'] * f + rs.randn(4) * SIGMA)
                S.append(p['score'])
        out.append((P, S))
    return out


def _pack(name, frames, track_buffer=TRACK_BUFFER, **more):
    pts = [np.asarray(P, np.float64).reshape(-1, 4) for P, _ in frames]
    seq = {'points': np.concatenate(pts).astype(F32), 'scores': np.concatenate([np.asarray(S, np.float64) for _, S in frames]).astype(F32),
           'n_det': [len(S) for _, S in frames], 'track_buffer': track_buffer, 'name': name, 'capacity': 256}
    seq.update(more)
    return seq


def occlusion_gaps(track_buffer=TRACK_BUFFER):
    """Next to a person who is always seen: occlusions of exactly buffer, buffer + 1 and buffer + 2 frames.  After buffer + 1 frames the
    track is marked REMOVED but is still on the lost list, is revived from there with its old id, and when it is lost again (three
    frames later, for good) it is forgotten at once -- minus(lost, removed_stracks) on the host, `dropped` on the device."""
    b, t0 = track_buffer, 6
    persons = [_person(200, 200, [(0, 40)], vel=(2., 1., 0.3, 0.)),
               _person(2200, 200, [(0, t0), (t0 + b, 40)], vel=(-1., 2., 0., 0.)),
               _person(4200, 200, [(0, t0), (t0 + b + 1, t0 + b + 4)], vel=(1., -1., 0.5, 0.)),
               _person(6200, 200, [(0, t0), (t0 + b + 2, 40)], vel=(2., 2., 0., 0.))]
    return _pack('occlusion_gaps', _frames(persons, 26, 11), track_buffer)


def equal_age_duplicate(track_buffer=TRACK_BUFFER):
    """E (born on frame 1, last seen on frame 6: age 5) is occluded; F (born on frame 3, 400 deeper, so never E's detection) walks past
    at 60 px a frame and is first within 60 px of E in (x, y) on frame 8, at age 5 as well: at equal age the LIVE track goes."""
    persons = [_person(200, 200, [(0, 6)]),
               _person(200 - 30 - 7 * 60, 200, [(2, 20)], z=600., vel=(60., 0., 0., 0.)),
               _person(5200, 200, [(0, 20)])]
    return _pack('equal_age_duplicate', _frames(persons, 16, 12), track_buffer)


def repeated_rows(track_buffer=TRACK_BUFFER):
    """Frames that hold the same row twice: the second person's detection and a copy of it with score 0.03, which takes part in no
    association -- only in the nearest-detection search, where the two distances are exactly equal and the FIRST wins (np.argmin).
    The copy comes before the original in frames 5 and 6 (the track is reported for a row it was not matched to), after it in 7 and 8.
    'dup_rows': frame -> the two equal rows."""
    persons = [_person(200, 200, [(0, 12)]), _person(2200, 200, [(0, 12)], vel=(3., 1., 0., 0.)), _person(4200, 200, [(0, 12)])]
    frames = _frames(persons, 12, 13)
    dup = {}
    for f in (5, 6, 7, 8):
        P, S = frames[f]
        at = 1 if f < 7 else 3                                           # before the original (row 1 -> rows 1, 2) or at the end
        P.insert(at, P[1].copy()); S.insert(at, 0.03)
        dup[f] = (1, 2) if f < 7 else (1, 3)
    return _pack('repeated_rows', frames, track_buffer, dup_rows=dup)


def cap_frame(track_buffer=TRACK_BUFFER):
    """Frames of 256 rows, the most a frame may hold, and a table of 512.  Frame 2 loses 100 persons and bears 100 others; those are
    confirmed in frame 3 and join the pool in frame 4, which then holds 256 confirmed + 100 lost tracks: a 356 x 256 matrix.  (Four
    frames: a track born after frame 1 joins the pool two frames later, so three frames cannot take the pool past 256.)"""
    g = 19
    at = lambda i: (500. + 1000. * (i % g), 500. + 1000. * (i // g))     # noqa: E731
    persons = [_person(*at(i), [(0, 1)], z=150. + i % 50, h=30. + i % 20) for i in range(100)]
    persons += [_person(*at(i), [(0, 4)], z=150. + i % 50, h=30. + i % 20, vel=(2., -1., 0.2, 0.)) for i in range(100, 256)]
    persons += [_person(*at(i), [(1, 4)], z=150. + i % 50, h=30. + i % 20, vel=(-1., 2., 0., 0.)) for i in range(256, 356)]
    return _pack('cap_frame', _frames(persons, 4, 14), track_buffer, capacity=512)


def full_table(track_buffer=TRACK_BUFFER):
    """Six persons from frame 1, a seventh from frame 4, and on frame 8 a detection seen once: the eighth and last track, tentative,
    never reported, gone a frame later.  A table of 8 is filled exactly (overflow 0); a table of 7 has no slot for that last birth
    (overflow 1) and, no id being given out after it, everybody else keeps id and row."""
    persons = [_person(200 + 2000 * i, 200, [(0, 14)], vel=(1., 1., 0., 0.)) for i in range(6)]
    persons += [_person(200, 3200, [(3, 14)]), _person(4200, 3200, [(7, 8)])]
    return _pack('full_table', _frames(persons, 14, 15), track_buffer, capacity=8)


def longest_call(track_buffer=TRACK_BUFFER):
    """1024 frames, the most one call may hold, of one person each; every 40 frames the score drops under the low threshold for 3
    frames (lost and revived) or for 9 (timed out, a new track)."""
    frames = _frames([_person(300, 300, [(0, 1024)], vel=(0.5, 0.25, 0.05, 0.))], 1024, 16)
    for f in range(1024):
        k, r = divmod(f, 40)
        if 20 <= r < (23 if k % 2 == 0 else 29):
            frames[f][1][0] = 0.03
    return _pack('longest_call', frames, track_buffer, capacity=4)


BAD_VALUES = ((np.nan, 0), (np.inf, 1), (-np.inf, 2), (np.nan, 3), (np.inf, 0), (-np.inf, 1), (np.nan, None))   # (value, coordinate; None: all four)


def nonfinite_sequences(track_buffer=TRACK_BUFFER):
    """From frame 2 on (a birth on frame 1 would be confirmed at once) every frame holds one row the tracker must keep to itself:

      strong_first / strong_middle   a NaN or +-inf coordinate with a strong score, at row 0 / in the middle of the frame
      low_first                      the same with score 0.03: it takes part in nothing
      nan_score                      a finite point, far from everybody, whose score is NaN: neither strong nor weak

    The host tracker raises on a non-finite point (scipy refuses the matrix), so the device's answer is defined by isolation:
    'host_points' holds the same frames with that row replaced by a finite point farther than 3 match_thresh from everybody and
    from its own earlier positions.  On both sides a strong such row begins a tentative track that nothing can match and that is
    removed a frame later, so ids stay in step.  'bad_row': frame -> the row, -1 where there is none."""
    persons = [_person(200, 200, [(0, 20)], vel=(2., 1., 0.3, 0.)), _person(2200, 200, [(0, 7), (10, 20)]),
               _person(4200, 200, [(0, 20)], vel=(-2., 2., 0., 0.), score=0.4), _person(6200, 200, [(4, 20)]),
               _person(8200, 200, [(0, 13)], vel=(1., 1., 1., 0.1))]
    out = []
    for name, score, where in (('strong_first', 0.6, 0), ('strong_middle', 0.6, 2), ('low_first', 0.03, 0), ('nan_score', np.nan, 0)):
        frames = _frames(persons, 20, 17)
        host, bad_row = [], []
        for f, (P, S) in enumerate(frames):
            H = [p.copy() for p in P]
            if f >= 1:
                far = np.array([-5000. - 3000. * f, -5000., 200., 40.])
                row = far.copy()
                if name != 'nan_score':
                    v, k = BAD_VALUES[f % len(BAD_VALUES)]
                    row[slice(None) if k is None else k] = v
                P.insert(where, row); H.insert(where, far); S.insert(where, score)
            host.append((H, S))
            bad_row.append(where if f >= 1 else -1)
        seq = _pack('nonfinite_' + name, frames, track_buffer, bad_row=bad_row)
        seq['host_points'] = _pack('', host)['points']
        out.append(seq)
    return out


def edge_sequences():
    """The sequences compared frame by frame with the host tracker (tests/test_gpu_track_edges.py); tests/test_track_cases.py shows
    that each takes the path it is named for and holds no near-tie."""
    return [occlusion_gaps(), equal_age_duplicate(), repeated_rows(), cap_frame(), full_table()]


def run_host(seq, first_id=0):
    """-> (per-frame (ids, rows), per-frame (tracked, lost) lists of (id, state, mean[8]), branch counts).  Empty frames are skipped
    as the callers of the tracker skip them: ([], []) and the lists of the frame before."""
    T.Track.last_id = first_id
    trk = T.Tracker(det_thresh=0.12, low_conf_det_thresh=0.05, track_buffer=seq['track_buffer'], match_thresh=300, frame_rate=30)
    stats = dict(weak_frames=0, revived=0, removed_tentative=0, timed_out=0, duplicate_kills=0, other_row=0, no_strong=0, empty=0,
                 revived_after_timeout=0, forgotten_at_once=0, duplicate_equal_age=0)
    matched = {}
    inner, inner_distances = T.Track.absorb, T.distances

    def absorb(self, det, frame):
        matched[self.tid] = det.z0.copy()
        return inner(self, det, frame)

    def distances(a, b, dim=4):                                          # (dim 2: the duplicate test of live against lost tracks)
        d = inner_distances(a, b, dim)
        if dim == 2 and d.size:
            for i, j in zip(*np.where(d < trk.duplicat_dist_thresh)):
                stats['duplicate_equal_age'] += a[i].frame - a[i].born == b[j].frame - b[j].born
        return d

    T.Track.absorb = absorb
    T.distances = distances
    outs, lists, known = [], [], {}
    snap = lambda: ([(t.tid, t.state, t.mean.copy()) for t in trk.tracked_stracks], [(t.tid, t.state, t.mean.copy()) for t in trk.lost_stracks])
    try:
        for pts, sc in frames_of(seq, host=True):
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
            once_removed = [t for t in trk.tracked_stracks if t.tid in {r.tid for r in trk.removed_stracks}]
            matched.clear()
            ids, rows = trk.update(pts, sc)
            # a track marked REMOVED that was still on the lost list and is tracked again; such a track, lost again, is on no list
            stats['revived_after_timeout'] += len(timed_before & {t.tid for t in trk.tracked_stracks})
            stats['forgotten_at_once'] += sum(t.state == T.LOST and t.tid not in {x.tid for x in trk.lost_stracks} for t in once_removed)
            for t in trk.tracked_stracks + trk.lost_stracks:
                known[t.tid] = t
            stats['revived'] += len(lost_before & {t.tid for t in trk.tracked_stracks})
            stats['removed_tentative'] += sum(t.state == T.REMOVED for t in tent_before)
            stats['timed_out'] += sum(t.state == T.REMOVED and t.tid not in timed_before for t in lost_objs)
            listed = {t.tid for t in trk.tracked_stracks + trk.lost_stracks}
            for tid, t in list(known.items()):
                if tid not in listed:
                    if t.state == T.TRACKED or (t.state == T.LOST and t not in once_removed):   # gone without having been removed: killed as a duplicate
                        stats['duplicate_kills'] += 1
                    del known[tid]
            for tid, row in zip(ids, rows):
                if tid in matched and not np.array_equal(matched[tid], pts[row]):
                    stats['other_row'] += 1
            outs.append((ids, rows))
            lists.append(snap())
    finally:
        T.Track.absorb, T.distances = inner, inner_distances
    return outs, lists, stats
