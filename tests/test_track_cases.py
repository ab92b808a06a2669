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
