"""The device tracker (csrc/track.hip) on the edge sequences of tests/track_cases.py, each of which takes one path the sequences of
test_gpu_track.py never take (tests/test_track_cases.py counts them on the host): a track revived after its timeout and forgotten at
once when lost again (`dropped`), a duplicate at equal age, two equal rows in the nearest-detection search, frames and tables at
their caps (a 356 x 256 association), a table filled exactly and one slot short, the longest call (T = 1024), and rows with NaN or
+-inf coordinates or a NaN score.

Against the host tracker, as in test_gpu_track.py: decisions (ids, rows, list order, states) exact, means within 1e-6.  The host
raises on a non-finite point, so there the device's answer is defined by isolation: the host gets the same frames with that row
replaced by a finite point far from everybody, and everybody else must come out the same -- and never be reported for that row.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
EDGES = ('occlusion_gaps', 'equal_age_duplicate', 'repeated_rows', 'cap_frame', 'full_table')
NONFINITE = ('nonfinite_strong_first', 'nonfinite_strong_middle', 'nonfinite_low_first', 'nonfinite_nan_score')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cases():
    return {seq['name']: (seq,) + TC.run_host(seq) for seq in TC.edge_sequences() + TC.nonfinite_sequences()}


def _tracker(dev, seq, capacity=None):
    from romp_amd.tracking import DeviceTracker
    return DeviceTracker(dev, capacity=capacity or seq['capacity'], det_thresh=0.12, low_conf_det_thresh=0.05, track_buffer=seq['track_buffer'],
                         match_thresh=300, frame_rate=30)


def _replay(dev, seq, outs, lists, capacity=None, compare_lists=True):
    """Frame by frame against the host's answers -> (tracker, the largest |mean - host mean| over the finite tracks)."""
    trk = _tracker(dev, seq, capacity)
    points, scores = torch.from_numpy(seq['points']).to(dev), torch.from_numpy(seq['scores']).to(dev)
    at, worst = 0, 0.
    for f, k in enumerate(seq['n_det']):
        ids, rows = trk.update_host(points[at:at + k], scores[at:at + k])
        at += k
        assert (ids, rows) == (list(outs[f][0]), list(outs[f][1])), (seq['name'], f, ids, rows, outs[f])
        if not compare_lists:
            continue
        tracked, lost = trk.tracks()
        for got, want in ((tracked, lists[f][0]), (lost, lists[f][1])):
            assert got[:, 0].astype(int).tolist() == [w[0] for w in want], (seq['name'], f)
            assert got[:, 1].astype(int).tolist() == [w[1] for w in want], (seq['name'], f)
            if len(want):
                gap = np.abs(got[:, 6:] - np.stack([w[2] for w in want])).max(1)
                finite = np.isfinite(got[:, 6:]).all(1)
                if 'bad_row' in seq:                                      # the track begun by the isolated row: tentative, never matched, other means
                    assert all(not c and fr == b for c, fr, b in got[~finite][:, 2:5].tolist()), (seq['name'], f)
                else:
                    assert finite.all()
                worst = max(worst, float(gap[finite].max(initial=0.)))
    return trk, worst


@pytest.mark.parametrize('name', EDGES)
def test_edge_sequences_frame_by_frame(dev, cases, name):
    seq, outs, lists, stats = cases[name]
    trk, worst = _replay(dev, seq, outs, lists)
    print('%s: %d frames, max |mean - host mean| = %.3e' % (name, len(seq['n_det']), worst))
    assert worst < 1e-6 and trk.overflow == 0
    if name == 'occlusion_gaps':
        assert stats['revived_after_timeout'] > 0 and stats['forgotten_at_once'] > 0
    if name == 'equal_age_duplicate':
        assert stats['duplicate_equal_age'] > 0
    if name == 'cap_frame':
        tracked, lost = trk.tracks()
        assert len(tracked) == 256 and len(lost) == 100 and trk.capacity == 512


def test_a_table_filled_exactly_and_one_slot_short(dev, cases):
    seq, outs, lists, _ = cases['full_table']
    peak = int(np.argmax([len(t) + len(lo) for t, lo in lists]))
    trk = _tracker(dev, seq)
    points, scores = torch.from_numpy(seq['points']).to(dev), torch.from_numpy(seq['scores']).to(dev)
    at = np.concatenate([[0], np.cumsum(seq['n_det'])])
    for f in range(peak + 1):
        trk.update(points[at[f]:at[f + 1]], scores[at[f]:at[f + 1]])
    tracked, lost = trk.tracks()
    assert len(tracked) + len(lost) == trk.capacity == 8 and trk.overflow == 0            # every slot in use, nobody turned away
    short, _ = _replay(dev, seq, outs, lists, capacity=7, compare_lists=False)            # ids and rows of everybody: the host's
    assert short.overflow == 1
    tracked, lost = short.tracks()
    assert tracked[:, 0].astype(int).tolist() == [1, 2, 3, 4, 5, 6, 7] and len(lost) == 0


@pytest.mark.parametrize('name', NONFINITE)
def test_a_nonfinite_row_stays_alone(dev, cases, name):
    seq, outs, lists, _ = cases[name]
    trk, worst = _replay(dev, seq, outs, lists)        # (ids, rows, list order and states of everybody equal the host's with the row moved away)
    print('%s: %d frames, max |mean - host mean| of the finite tracks = %.3e' % (name, len(seq['n_det']), worst))
    assert worst < 1e-6 and trk.overflow == 0
    for f, (ids, rows) in enumerate(outs):
        assert seq['bad_row'][f] not in rows                              # (and so, by the equality above, not in the device's rows)


def _scratch_free(state):
    """The state bytes without the staging area of the row counts (int32 words 32 .. 32 + 1024), which only a multi-frame call writes."""
    w = state.cpu().numpy().view(np.int32)
    return np.concatenate([w[:32], w[32 + 1024:]])


def test_the_longest_call_equals_1024_calls(dev):
    seq = TC.longest_call()
    T = len(seq['n_det'])
    assert T == 1024 and set(seq['n_det']) == {1}
    points, scores = torch.from_numpy(seq['points']).to(dev), torch.from_numpy(seq['scores']).to(dev)
    one, many = _tracker(dev, seq), _tracker(dev, seq)
    count, ids, rows, slots = (t.cpu().numpy() for t in one.update_frames(points, scores, seq['n_det']))
    steps = [many.update(points[f:f + 1], scores[f:f + 1]) for f in range(T)]
    c, i, r, s = (torch.stack([st[k] for st in steps]).cpu().numpy() for k in range(4))
    assert np.array_equal(c[:, 0], count) and np.array_equal(i, ids) and np.array_equal(s, slots)
    assert np.array_equal(np.where(i >= 0, r + np.arange(T)[:, None], 0), rows)            # (absolute rows)
    assert np.array_equal(_scratch_free(one.state), _scratch_free(many.state))
    assert count.sum() > 800 and len(set(ids[ids >= 0].tolist())) > 5 and one.header()[1] == T
