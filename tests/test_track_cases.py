"""The sequences of tests/track_cases.py on the host tracker alone: they hold no near-tie (a relative 1e-5 perturbation of the points
changes no decision, so an ulp-level difference in a distance or in a 4 x 4 solve cannot legitimately flip one either), and together
they take every branch of Tracker.update.  Also the C seam of the device tracker as far as it goes without a device."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cases as TC  # noqa: E402


@pytest.fixture(scope='module')
def runs():
    return [(seq,) + TC.run_host(seq) for seq in TC.sequences()]


def test_sizes_and_scripted_scores():
    for n, seq in zip(TC.SIZES, TC.sequences()):
        full = [k for k in seq['n_det'] if k]
        assert 30 <= len(seq['n_det']) <= 60 and 0 in seq['n_det'] and max(seq['n_det']) <= 256
        assert abs(np.median(full) - n) <= max(1, 0.15 * n), (n, np.median(full))   # (the "about" of ~16, ~57, ~98)
        assert (seq['scores'] == np.float32(0.12)).any() and (seq['scores'] == np.float32(0.05)).any()
        assert seq['points'].dtype == np.float32 and seq['scores'].dtype == np.float32 and 3 <= seq['track_buffer'] <= 5


def test_no_near_ties(runs):
    for seq, outs, _, _ in runs:
        again, _, _ = TC.run_host(TC.perturbed(seq))
        assert again == outs, seq['name']


def test_every_branch_is_taken(runs):
    total = {}
    for seq, outs, lists, stats in runs:
        print(seq['name'], stats)
        for k, v in stats.items():
            total[k] = total.get(k, 0) + int(v)
        ids = [i for o in outs for i in o[0]]
        assert ids and max(ids) >= 1
    for k in ('weak_frames', 'revived', 'removed_tentative', 'timed_out', 'duplicate_kills', 'other_row', 'no_strong', 'empty'):
        assert total[k] > 0, k
    # births after frame 1 and deaths: more ids than persons ever seen at once, and lost lists that are not empty at the end
    seq, outs, lists, _ = runs[2]
    assert max(max(o[0]) for o in outs if o[0]) > max(seq['n_det'])
    assert any(len(lost) for _, lost in lists)


# ------------------------------------------------------------------------------------------------ the edge sequences
@pytest.fixture(scope='module')
def edges():
    return {seq['name']: (seq,) + TC.run_host(seq) for seq in TC.edge_sequences() + TC.nonfinite_sequences() + [TC.longest_call()]}


def test_edge_sequences_hold_no_near_ties(edges):
    """A relative 1e-5 perturbation changes no decision -- except, in repeated_rows, which of the two EQUAL rows is the nearest."""
    assert len(edges) == 5 + 4 + 1
    for name, (seq, outs, _, _) in edges.items():
        again, _, _ = TC.run_host(TC.perturbed(seq))
        if name != 'repeated_rows':
            assert again == outs, name
            continue
        flipped = 0
        for f, (a, b) in enumerate(zip(again, outs)):
            assert a[0] == b[0], f
            for tid, ra, rb in zip(a[0], a[1], b[1]):
                if ra != rb:
                    assert f in seq['dup_rows'] and tid == 2 and {ra, rb} == set(seq['dup_rows'][f]), (f, tid, ra, rb)
                    flipped += 1
        print('repeated_rows: the perturbation flips %d of %d tied argmins and nothing else' % (flipped, len(seq['dup_rows'])))


def test_occlusions_of_buffer_and_one_and_two_more(edges):
    seq, outs, lists, stats = edges['occlusion_gaps']
    print(seq['name'], stats)
    b = seq['track_buffer']
    assert stats['revived_after_timeout'] == 1 and stats['forgotten_at_once'] == 1 and stats['revived'] == 2 and stats['timed_out'] == 2
    assert [o[0] for o in outs[:6]] == [[1, 2, 3, 4]] * 6 and [o[0] for o in outs[6:6 + b]] == [[1]] * b
    assert outs[6 + b][0] == [1, 2]                                       # back after `buffer` frames: a plain revival
    assert [(i, s) for i, s, _ in lists[6 + b][1]] == [(3, TC.T.REMOVED), (4, TC.T.REMOVED)]   # timed out, on the lost list for one more frame
    assert outs[6 + b + 1][0] == [1, 2, 3] and lists[6 + b + 1][1] == []  # ... from where 3 is revived with its id; 4 is gone,
    assert outs[6 + b + 3][0] == [1, 2, 3, 5]                             # so the last person gets a new id
    assert outs[6 + b + 4][0] == [1, 2, 5] and lists[6 + b + 4][1] == []  # 3 is lost again: on no list from the first frame on
    assert all(o[0] == [1, 2, 5] for o in outs[6 + b + 4:])


def test_at_equal_age_the_live_track_goes(edges):
    seq, outs, lists, stats = edges['equal_age_duplicate']
    print(seq['name'], stats)
    assert stats['duplicate_equal_age'] == 1 and stats['duplicate_kills'] >= 1
    assert [i for i, _, _ in lists[6][0]] == [2, 3] and [i for i, _, _ in lists[6][1]] == [1]
    assert [i for i, _, _ in lists[7][0]] == [2] and [i for i, _, _ in lists[7][1]] == [1]      # 3 (live) went, 1 (lost) stayed


def test_repeated_rows_tie_only_the_argmin(edges):
    seq, outs, _, _ = edges['repeated_rows']
    at = np.concatenate([[0], np.cumsum(seq['n_det'])])
    for f, (i, j) in seq['dup_rows'].items():
        pts, sc = seq['points'][at[f]:at[f + 1]], seq['scores'][at[f]:at[f + 1]]
        assert np.array_equal(pts[i], pts[j]) and i < j and sorted(sc[[i, j]].tolist()) == [np.float32(0.03), np.float32(0.7)]
        assert outs[f][0] == [1, 2, 3] and outs[f][1][1] == i             # the first of the two, as np.argmin
    assert {sc_first for sc_first in (float(seq['scores'][at[f] + i]) for f, (i, j) in seq['dup_rows'].items())} == \
        {float(np.float32(0.03)), float(np.float32(0.7))}                 # the copy comes first in some frames, second in others


def test_cap_sized_frames_and_tables(edges):
    seq, outs, lists, _ = edges['cap_frame']
    assert seq['n_det'] == [256] * 4 and seq['capacity'] == 512
    pool = sum(1 for _ in lists[2][0]) + len(lists[2][1])                 # (after frame 3 every tracked track is confirmed)
    assert pool == 356 and len(lists[2][1]) == 100 and len(outs[3][0]) == 256 and max(outs[3][0]) == 356
    seq, outs, lists, stats = edges['full_table']
    peak = [len(t) + len(lo) for t, lo in lists]
    assert max(peak) == seq['capacity'] == 8 and peak.count(8) == 1 and stats['removed_tentative'] == 1
    assert all(8 not in o[0] for o in outs) and max(max(i for i, _, _ in t) for t, _ in lists) == 8   # the last id, never reported
    seq, outs, _, stats = edges['longest_call']
    assert seq['n_det'] == [1] * 1024 and stats['revived'] > 5 and stats['timed_out'] > 5 and len({i for o in outs for i in o[0]}) > 5


def test_nonfinite_sequences_isolate_one_row(edges):
    for seq in TC.nonfinite_sequences():
        name = seq['name']
        at = np.concatenate([[0], np.cumsum(seq['n_det'])])
        pts, host, sc = seq['points'], seq['host_points'], seq['scores']
        bad_abs = [at[f] + r for f, r in enumerate(seq['bad_row']) if r >= 0]
        assert seq['bad_row'][0] == -1 and len(bad_abs) == len(seq['n_det']) - 1 and np.isfinite(host).all()
        others = np.ones(len(pts), bool)
        others[bad_abs] = False
        assert np.array_equal(pts[others], host[others])
        for k in bad_abs:                                                 # farther than the widest round from every other row of the sequence
            d = np.linalg.norm(host.astype(np.float64) - host[k].astype(np.float64), axis=1)
            d[k] = np.inf
            assert d.min() > TC.FAR, (name, k, d.min())
        if name == 'nonfinite_nan_score':
            assert np.isnan(sc[bad_abs]).all() and np.array_equal(pts, host)
        else:
            assert not np.isfinite(pts[bad_abs]).all(1).any() and np.isfinite(sc).all()
            kinds = pts[bad_abs]
            assert np.isnan(kinds).any() and np.isposinf(kinds).any() and np.isneginf(kinds).any()
            assert all(not np.isfinite(kinds[:, c]).all() for c in range(4))
        seq_, outs, lists, stats = edges[name]
        strong = name.startswith('nonfinite_strong')
        assert stats['removed_tentative'] == (len(bad_abs) - 1 if strong else 0) and stats['revived'] == 1 and stats['timed_out'] == 1
        for f, (ids, rows) in enumerate(outs):
            assert seq['bad_row'][f] not in rows and len(ids) >= 4
    first, middle = TC.nonfinite_sequences()[:2]
    assert set(first['bad_row'][1:]) == {0} and set(middle['bad_row'][1:]) == {2} and min(middle['n_det'][1:]) >= 5


# ------------------------------------------------------------------------------------------------ the C seam
def test_track_symbols_exported():
    from romp_amd import lib
    header = open(os.path.join(ROOT, 'include', 'romp_hip_track.h')).read()
    declared = re.findall(r'^\s*(?:int|void)\s+(\w+)\s*\(', header, re.M)
    assert declared == lib.TRACK_EXPORTS == ['romp_track_state_bytes', 'romp_track_init', 'romp_track_frames', 'romp_track_assign',
                                             'romp_track_list', 'romp_oneeuro_smooth_frames']
    others = (lib.EXPORTS + lib.VIEW_EXPORTS + lib.MAP_EXPORTS + lib.TEXTURE_EXPORTS + lib.EVAL_EXPORTS + lib.RH_EXPORTS +
              lib.CANVAS_EXPORTS + lib.SMPL_GRAD_EXPORTS + lib.FIT_EXPORTS + lib.FIT_PRIOR_EXPORTS)
    assert not set(declared) & set(others) and len(lib.EXPORTS) == 52
    h = lib.load()
    assert h.romp_abi_version() == 7 == lib.ABI_VERSION
    assert len(h.romp_track_frames.argtypes) == 12 and len(h.romp_oneeuro_smooth_frames.argtypes) == 15
    for n in declared:
        assert getattr(h, n).restype is ctypes.c_int, n


def test_the_header_compiles_as_c():
    prog = ('#include "romp_hip_track.h"\nint main(void) { return ROMP_TRACK_MAX_DET == 256 && ROMP_TRACK_MAX_CAPACITY == 512 && '
            'ROMP_TRACK_SLOT_BYTES == 8 * 72 + 4 * 8 ? 0 : 1; }\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, 't.c')
        open(c, 'w').write(prog)
        subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), c, '-o', os.path.join(td, 't')])
        subprocess.check_call([os.path.join(td, 't')])


def test_host_side_validation_needs_no_device():
    """Every argument check comes before any device call: the refusals below run on a machine without a GPU."""
    from romp_amd import lib
    h = lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rows = (ctypes.c_int32 * 2)(3, 257)
    for cap in (0, -1, 513):
        assert h.romp_track_state_bytes(cap) == -1 and b'capacity' in h.romp_last_error()
    assert h.romp_track_state_bytes(1) > 0 and h.romp_track_state_bytes(512) % 8 == 0
    assert h.romp_track_init(None, 4, 0, 0.12, 0.05, 300., 60, 60., None) == -1
    assert h.romp_track_init(p, 0, 0, 0.12, 0.05, 300., 60, 60., None) == -1
    assert h.romp_track_init(p, 4, -1, 0.12, 0.05, 300., 60, 60., None) == -1
    assert h.romp_track_init(p, 4, 0, float('nan'), 0.05, 300., 60, 60., None) == -1
    assert h.romp_track_init(p, 4, 0, 0.12, 0.05, float('inf'), 60, 60., None) == -1
    assert h.romp_track_init(p, 4, 0, 0.12, 0.05, 300., -1, 60., None) == -1
    assert h.romp_track_frames(p, p, p, rows, 2, p, p, p, p, None, 0, None) == -1 and b'257' in h.romp_last_error()
    assert h.romp_track_frames(p, p, p, rows, 0, p, p, p, p, None, 0, None) == -1
    assert h.romp_track_frames(p, None, p, rows, 1, p, p, p, p, None, 0, None) == -1
    assert h.romp_track_frames(p, p, p, rows, 1, p, p, p, p, p, 0, None) == -1 and b'stride' in h.romp_last_error()
    assert h.romp_track_assign(p, 0, 3, 10., p, None) == -1                      # no rows
    assert h.romp_track_assign(p, 3, 0, 10., p, None) == -1
    assert h.romp_track_assign(p, 513, 3, 10., p, None) == -1
    assert h.romp_track_assign(p, 3, 3, float('nan'), p, None) == -1
    assert h.romp_track_assign(None, 3, 3, 10., p, None) == -1
    assert h.romp_track_list(p, None, p, None) == -1
    assert h.romp_oneeuro_smooth_frames(p, 0, 4, p, p, p, 10, 3., p, p, p, p, p, p, None) == -1
    assert h.romp_oneeuro_smooth_frames(p, 1, 513, p, p, p, 10, 3., p, p, p, p, p, p, None) == -1
    assert h.romp_oneeuro_smooth_frames(p, 1, 4, p, p, p, 10, 0., p, p, p, p, p, p, None) == -1
