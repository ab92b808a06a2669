"""The sequences of tests/temporal_cases.py without a device: the branches of the matrix -> axis-angle step they reach on the float64
path, the float32 oracle's own distance from float64 over them (the envelope E from which tests/test_gpu_temporal.py takes its
bound), the oracle against a fixture recorded from the reference at these edges, the bookkeeping model of the frames kernel
against a plain per-frame bank, and the argument checks of romp_oneeuro_smooth."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_cases as TC  # noqa: E402

from oracle import temporal_oracle as TO  # noqa: E402
from oracle import temporal_ref64 as R64  # noqa: E402


def _t(v):
    return torch.from_numpy(np.array(v))


@pytest.fixture(scope='module')
def path64():
    """name -> per frame the tuple of R64.smooth, smooth_coeff 3 and 16 betas."""
    out = {}
    for c in TC.cases():
        f = R64.make_filters(3.0)
        out[c['name']] = [R64.smooth(f, *x) for x in zip(c['thetas'], c['betas'], c['cam'])]
    return out


def test_table():
    assert TC.NAMES[:len(TC.EDGE_NAMES)] == TC.EDGE_NAMES and len(TC.EDGE_NAMES) == 20 and len(TC.NAMES) == 23
    assert [n for n in TC.NAMES if not TC.aa_elementwise(n)] == ['x_exact_pi', 'alt_0_pix', 'alt_pix_piy', 'alt_pix_piy_piz']
    for c in TC.cases():
        T = len(c['thetas'])
        assert 3 <= T <= 9 and c['thetas'].shape == (T, 72) and c['betas'].shape == (T, 16) and c['cam'].shape == (T, 3)
        assert all(c[k].dtype == np.float32 and np.isfinite(c[k]).all() for k in ('thetas', 'betas', 'cam'))
    rest = TC.case('rest')
    assert all((rest[k] == rest[k][0]).all() for k in ('thetas', 'betas', 'cam'))
    assert max(np.abs(c['betas']).max() for c in TC.cases()) > 8
    assert np.array_equal(TC.case('diag_tie')['thetas'][:, :3], np.float32([[0, 0, 2]] * 3))


def test_coverage_on_the_float64_path(path64):
    """Conditions on the table: all four branches, both signs of q0 inside the first three, the s2 == 0 arm, a quantity under the
    root below 2.1, and a filtered matrix that is far from orthonormal."""
    seen, zero, t_min, skew = set(), False, np.inf, 0.0
    for name, frames in path64.items():
        here = []
        for f, (_, _, _, R, info) in enumerate(frames):
            seen.add((info['branch'], info['q0_negative']))
            zero |= info['s2_zero']
            t_min = min(t_min, info['t'])
            M = R.reshape(3, 3)
            skew = max(skew, np.abs(M @ M.T - np.eye(3)).max())
            here.append('%d%s%s' % (info['branch'], '-' if info['q0_negative'] else '+', 'z' if info['s2_zero'] else ''))
        print('%-18s %s' % (name, ' '.join(here)))
    print('smallest t %.3f, largest |R R^T - I| %.3f' % (t_min, skew))
    for branch in (0, 1, 2):
        assert (branch, False) in seen and (branch, True) in seen, branch
    assert (3, False) in seen and zero and t_min < 2.1 and skew > 0.3
    assert all(i['s2_zero'] for *_, i in path64['zero'])
    for axis, name in enumerate(('x_near_minus_pi', 'y_near_minus_pi', 'z_near_minus_pi')):
        assert (axis, True) in {(i['branch'], i['q0_negative']) for *_, i in path64[name]}, name


def _envelope():
    """The float32 oracle against float64: worst ratio per segment over outputs and state rows, both smooth_coeff, 16 betas."""
    E = dict.fromkeys(TC.SEGMENTS + ('aa',) + tuple('dx_' + k for k in TC.SEGMENTS), 0.0)
    for coeff in (3.0, 1.0):
        for c in TC.cases():
            f32, f64 = TO.make_filters(coeff), R64.make_filters(coeff)
            worst = dict.fromkeys(E, 0.0)
            for x in zip(c['thetas'], c['betas'], c['cam']):
                t, b, cm = TO.smooth(f32, *(_t(v) for v in x))
                r = TC.output_ratios(t.numpy(), b.numpy(), cm.numpy(), R64.smooth(f64, *x), c['name'])
                s = TC.state_ratios(TC.oracle_state_row(f32), R64.state_row(f64), 16)
                for k in worst:
                    worst[k] = max(worst[k], r.get(k, 0.0), s.get(k, 0.0))
            print('coeff %g %-18s ' % (coeff, c['name']) + '  '.join('%s %.2f' % kv for kv in worst.items()))
            for k in E:
                E[k] = max(E[k], worst[k])
    return E


def test_float32_oracle_against_float64():
    """The measured envelope E, per case and in all, in units of 2^-24 * max(1, |ref|); the device bound K of
    tests/test_gpu_temporal.py is 4 E rounded up to a power of two, per kind of lane, and stays below 5e-6.  E is taken over the
    outputs (the root as a rotation matrix and element by element) and the state's x lanes; the state's dx_f lanes are printed
    apart: the oracle's own distance there (20 on the root) must at least stay inside the device bound."""
    E = _envelope()
    e_linear, e_root = max(E['pose'], E['betas'], E['cam']), max(E['root'], E['aa'])
    print('E: ' + '  '.join('%s %.2f' % kv for kv in E.items()) + '   linear %.2f root %.2f' % (e_linear, e_root))
    assert TC.K_LINEAR / 2 < 4 * e_linear <= TC.K_LINEAR and TC.K_ROOT / 2 < 4 * e_root <= TC.K_ROOT
    assert max(TC.K_LINEAR, TC.K_ROOT) * TC.UNIT < 5e-6
    assert E['dx_root'] <= TC.K_ROOT and max(E['dx_pose'], E['dx_betas'], E['dx_cam']) <= TC.K_LINEAR


def test_oracle_matches_reference_edge_fixture(golden_dir):
    """The float32 oracle against what the reference's own create_OneEuroFilter / smooth_results gave on the edge cases
    (oracle/make_golden_temporal_edges.py): that script's 2e-6, scaled by max(1, |value|), and NaN where the reference has NaN."""
    g = np.load(os.path.join(golden_dir, 'temporal_edges.npz'))
    assert sorted(g.files) == sorted('%s/%s' % (n, k) for n in TC.NAMES for k in ('thetas', 'betas', 'cam'))
    worst = 0.0
    for c in TC.cases():
        filters = TO.make_filters(3.0)
        for f, x in enumerate(zip(c['thetas'], c['betas'], c['cam'])):
            for key, a in zip(('thetas', 'betas', 'cam'), TO.smooth(filters, *(_t(v) for v in x))):
                r = g['%s/%s' % (c['name'], key)][f]
                assert np.array_equal(np.isnan(a.numpy()), np.isnan(r)), (c['name'], f, key)
                ok = ~np.isnan(r)
                d = float((np.abs(a.numpy().astype(np.float64) - r) / np.maximum(1, np.abs(r)))[ok].max())
                worst = max(worst, d)
                assert d < 2e-6, (c['name'], f, key, d)
    print('float32 oracle vs reference fixture on the edge cases: %.3e' % worst)


def test_simulate_frames_against_the_bank():
    """The word-0 and word-1 tables, one frame per call, every case a slot, rows and slots shuffled: the model must filter each case
    in the order of its frames -- fresh once, continued after -- and so land on TO.smooth's per-frame results."""
    cs = TC.cases()
    cap = len(cs)
    rs = np.random.RandomState(5)
    slot_of = rs.permutation(cap)
    words, filters, oracle = [0.0] * cap, {}, [TO.make_filters(3.0) for _ in cs]
    worst = 0.0
    for f in range(TC.MAX_FRAMES):
        alive = [i for i, c in enumerate(cs) if len(c['thetas']) > f]
        rs.shuffle(alive)                                                     # input row r holds case alive[r]
        inputs = tuple(np.stack([cs[i][k][f] for i in alive]) for k in ('thetas', 'betas', 'cam'))
        order = rs.permutation(len(alive))                                    # entry k reports input row order[k]
        rows, slots = np.full((1, cap), -7), np.full((1, cap), -7)
        rows[0, :len(alive)], slots[0, :len(alive)] = order, [slot_of[alive[r]] for r in order]
        before = list(words)
        sim = R64.simulate_frames(words, 1, cap, [len(alive)], rows, slots, inputs, filters)
        words = sim['words']
        assert [e[1] for e in sim['entries']] == list(range(len(alive)))
        for (t, k, slot, history, out) in sim['entries']:
            i = alive[order[k]]
            assert t == 0 and slot == slot_of[i] and history == ('fresh' if f == 0 else 'continued') and before[slot] == (f > 0)
            th, be, ca = TO.smooth(oracle[i], *(_t(cs[i][key][f]) for key in ('thetas', 'betas', 'cam')))
            r = TC.output_ratios(th.numpy(), be.numpy(), ca.numpy(), out, cs[i]['name'])
            worst = max(worst, max(r.values()))
            assert r['root'] <= TC.K_ROOT / 4 and r['aa'] <= TC.K_ROOT / 4 and max(r['pose'], r['betas'], r['cam']) <= TC.K_LINEAR / 4
        assert all(words[slot_of[i]] == 1.0 for i in alive)
    assert words == [1.0] * cap
    print('simulate_frames vs the float32 bank: worst ratio %.2f' % worst)


def test_simulate_frames_restart_words():
    """-(t + 1) and -(t + 1.5) in the model, by hand: capacity 1, T = 4."""
    c = TC.case('random_s3')
    inputs = (c['thetas'][:4], c['betas'][:4], c['cam'][:4])
    rows, slots = np.arange(4).reshape(4, 1), np.zeros((4, 1), int)
    run = lambda word, count, filters=None: R64.simulate_frames([word], 4, 1, count, rows, slots, inputs, filters)
    old = R64.make_filters(3.0)
    R64.smooth(old, c['thetas'][8], c['betas'][8], c['cam'][8])
    sim = run(-3.0, [1, 1, 1, 1], {0: R64.clone_filters(old)})
    assert [e[3] for e in sim['entries']] == ['continued', 'continued', 'restarted', 'continued'] and sim['words'] == [1.0]
    assert np.array_equal(sim['entries'][2][4][1], c['betas'][2].astype(np.float64))           # afresh: passed through
    assert not np.array_equal(sim['entries'][0][4][1], c['betas'][0].astype(np.float64))       # on the old history: filtered
    sim = run(-3.5, [1, 1, 1, 1], {0: R64.clone_filters(old)})
    assert [e[3] for e in sim['entries']] == ['fresh', 'continued', 'restarted', 'continued'] and sim['words'] == [1.0]
    assert np.array_equal(sim['entries'][0][4][1], c['betas'][0].astype(np.float64))
    assert [e[3] for e in run(-1.0, [1, 0, 1, 0], {0: old})['entries']] == ['restarted', 'continued']
    assert run(-3.0, [1, 1, 0, 0], {0: R64.clone_filters(old)})['words'] == [0.0]              # begun, not reported yet
    assert run(-3.5, [0, 0, 0, 0])['words'] == [0.0] and run(1.0, [0, 0, 0, 0])['words'] == [1.0] and run(0.0, [0, 0, 0, 0])['words'] == [0.0]
    assert len(run(0.0, [6, 6, 6, 6])['entries']) == 4                                         # a count above the capacity is cut to it


def test_oneeuro_smooth_refuses_bad_arguments_without_a_device():
    from romp_amd import lib
    h = lib.load()
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda state=p, slots=p, N=1, nb=10, coeff=3., th=p, be=p, ca=p: h.romp_oneeuro_smooth(state, slots, N, nb, coeff, th, be, ca, None)
    assert call(N=0) == -1 and b'romp_oneeuro_smooth' in h.romp_last_error()
    assert call(N=-1) == -1
    for nb in (0, 17, -1):
        assert call(nb=nb) == -1, nb
    for coeff in (0., -1., float('nan')):
        assert call(coeff=coeff) == -1, coeff
    for name in ('state', 'slots', 'th', 'be', 'ca'):
        assert call(**{name: None}) == -1, name
    assert not any(buf)
    assert [h.romp_oneeuro_state_floats(nb) for nb in (1, 10, 16)] == [1 + 3 * 82, 1 + 3 * 91, 1 + 3 * 97]
