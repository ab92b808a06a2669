"""The OneEuro smoother kernels (csrc/temporal.hip) alone, through their C entries, against the float64 restatement
oracle/temporal_ref64.py on the sequences of tests/temporal_cases.py (run with -m gpu on the MI355X box).

What the five smoothing tests of test_temporal.py / test_gpu_track.py cannot see: their sequences keep the filtered root matrix in
one of the four branches of rmat_t_to_aa_dev, their reference is float32 under a 2e-5 bound, the frames kernel is only compared with
the bank kernel (both call the same oneeuro_person), its state words occur only as romp_track_frames happens to write them, and
n_betas is 10 or 11.  Here: all four branches with both signs of q0, the zero rotation and filtered matrices far from orthonormal;
n_betas 1, 10, 11 and 16; every state word on slots reported before, after, on both sides of and never around the restart frame;
counts above the capacity and of zero; the out_rows indirection; non-finite inputs; repeatability on a side stream.  State and
outputs lie inside bands of a sentinel word (ordinary memory of the same allocation: nothing here can fault), and every row a
call has no business with is compared bit for bit.

Bound: |got - float64| <= K * 2^-24 * max(1, |float64|).  E, the float32 oracle's own worst distance from float64 over the case
table in those units (tests/test_temporal_cases.py measures it): 3.19 on the linear lanes (pose 2.77, betas 3.19, cam 2.07), 7.47 on
the root as a rotation matrix (3.33 element by element).  K = 4 E rounded up to a power of two -- the 4 for sinf / cosf / atan2f /
sqrtf / division a few ulp from correctly rounded and for the contraction the compiler may apply in the filter arithmetic:
K = 16 (9.5e-7) on the linear lanes, K = 32 (1.9e-6) on the root, against 2e-5 before.  E is taken over the outputs and the
state's x lanes.  The state's dx_f lanes are under the same bound but printed apart (dx_root, ...): they hold a filtered difference
of two consecutive x times the 30 Hz rate, and on the root, whose x_raw is computed and not given, the float32 oracle itself is
20.4 units from float64 there (4.2 on the linear lanes) -- the margin under K = 32 is 1.6, not 4.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_cases as TC  # noqa: E402
from test_gpu_conv_shapes import SENTINEL, Guarded  # noqa: E402

from oracle import temporal_oracle as TO  # noqa: E402
from oracle import temporal_ref64 as R64  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ('thetas', 'betas', 'cam')
K_OF = {'root': TC.K_ROOT, 'aa': TC.K_ROOT, 'pose': TC.K_LINEAR, 'betas': TC.K_LINEAR, 'cam': TC.K_LINEAR}
K_OF.update({'dx_' + k: v for k, v in list(K_OF.items()) if k != 'aa'})
SENTINEL_F32 = np.array([SENTINEL], np.int32).view(np.float32)[0]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _ref64(n_betas, coeff):
    """name -> per frame (the tuple of R64.smooth, the state row after it).  Read-only."""
    out = {}
    for c in TC.cases():
        f, rows = R64.make_filters(coeff), []
        for th, be, ca in zip(c['thetas'], c['betas'], c['cam']):
            ref = R64.smooth(f, th, be[:n_betas], ca)
            rows.append((ref, R64.state_row(f)))
        out[c['name']] = rows
    return out


def _guarded(dev, array):
    """`array` (float32 numpy) on the device inside sentinel bands."""
    g = Guarded(dev, array.shape, 64, SENTINEL)
    g.reset(torch.from_numpy(np.ascontiguousarray(array)).to(dev))
    return g


def _sentinel(*shape):
    return np.full(shape, SENTINEL_F32, np.float32)


def _bits(g):
    return (g.inner if isinstance(g, Guarded) else g).contiguous().view(torch.int32).cpu().numpy()


def _vals(g):
    return g.inner.cpu().numpy()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


class Worst(dict):
    def take(self, ratios):
        for k, v in ratios.items():
            self[k] = max(self.get(k, 0.0), v) if v == v else float('nan')

    def within_bound(self, what):
        print('%s: worst ratio in units of 2^-24 * max(1, |float64|): ' % what + '  '.join('%s %.2f' % (k, self[k]) for k in sorted(self)))
        for k, v in self.items():
            assert v <= K_OF[k], (what, k, v)


def _bank(dev, state, slots, n_betas, coeff, th, be, ca):
    from romp_amd import lib as L
    s = torch.tensor(list(slots), dtype=torch.int32, device=dev)
    L.check(L.load().romp_oneeuro_smooth(L.ptr(state.inner), L.ptr(s), len(slots), n_betas, coeff, L.ptr(th.inner), L.ptr(be.inner),
                                         L.ptr(ca.inner), L.stream_ptr(dev)))
    torch.cuda.current_stream(dev).synchronize()


class Tables:
    """out_count / out_rows / out_slots and the estimates of a frames call, on the host and on the device."""

    def __init__(self, dev, capacity, count, rows, slots, inputs):
        self.T, self.capacity = len(count), capacity
        self.count, self.rows, self.slots = np.asarray(count, np.int32), np.asarray(rows, np.int32), np.asarray(slots, np.int32)
        assert self.rows.shape == self.slots.shape == (self.T, capacity)
        self.inputs = tuple(np.ascontiguousarray(v, np.float32) for v in inputs)
        self.n_betas = self.inputs[1].shape[1]
        self.d = [torch.from_numpy(v).to(dev) for v in (self.count, self.rows, self.slots) + self.inputs]
        self.dev = dev

    def outputs(self):
        return [_guarded(self.dev, _sentinel(self.T * self.capacity, w)) for w in (72, self.n_betas, 3)]

    def run(self, state, coeff, outs, splits=None):
        """The call, or one call per (first frame, frames) of `splits`, on the current stream."""
        from romp_amd import lib as L
        cap = self.capacity
        for t0, T in splits or [(0, self.T)]:
            cnt, rows, slots, th, be, ca = self.d
            L.check(L.load().romp_oneeuro_smooth_frames(
                L.ptr(state.inner), T, cap, L.ptr(cnt[t0:]), L.ptr(rows[t0:]), L.ptr(slots[t0:]), self.n_betas, coeff, L.ptr(th), L.ptr(be),
                L.ptr(ca), L.ptr(outs[0].inner[t0 * cap:]), L.ptr(outs[1].inner[t0 * cap:]), L.ptr(outs[2].inner[t0 * cap:]),
                L.stream_ptr(self.dev)))
        torch.cuda.current_stream(self.dev).synchronize()

    def reported(self):
        """{(t, k)} a call filters."""
        return {(t, k) for t in range(self.T) for k in range(min(int(self.count[t]), self.capacity))}

    def check_untouched_outputs(self, outs):
        keep = np.ones((self.T, self.capacity), bool)
        for t, k in self.reported():
            keep[t, k] = False
        for g in outs:
            assert g.bands_intact()
            assert (_bits(g).reshape(self.T, self.capacity, -1)[keep] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ the bank entry
ROWS = 40
SLOT_OF = [(7 * i + 3) % ROWS for i in range(len(TC.NAMES))]            # a fixed non-monotone permutation into a larger buffer


@pytest.mark.parametrize('coeff', [3.0, 1.0])
@pytest.mark.parametrize('n_betas', [1, 10, 11, 16])
def test_bank_entry_against_float64(dev, n_betas, coeff):
    """romp_oneeuro_smooth, every case a person of one launch per frame (shorter cases drop out as they end): outputs, root as a
    matrix and element by element, and the state row [1, x_raw, x_f, dx_f] after every frame; rows of other slots, unused rows and
    all bands unchanged.  Reaches all four branches with both signs of q0 and the s2 == 0 arm; state words 0 and 1."""
    from romp_amd import lib as L
    cs, ref = TC.cases(), _ref64(n_betas, coeff)
    stride = L.load().romp_oneeuro_state_floats(n_betas)
    D = 81 + n_betas
    assert stride == 1 + 3 * D and len(set(SLOT_OF)) == len(cs) and SLOT_OF != sorted(SLOT_OF)
    init = _sentinel(ROWS, stride)
    init[SLOT_OF] = 0
    state = _guarded(dev, init)
    prev = _vals(state)
    worst = Worst()
    for f in range(TC.MAX_FRAMES):
        alive = [i for i, c in enumerate(cs) if len(c['thetas']) > f]
        x = [np.stack([cs[i][k][f][:n_betas] if k == 'betas' else cs[i][k][f] for i in alive]) for k in KEYS]
        th, be, ca = (_guarded(dev, v) for v in x)
        _bank(dev, state, [SLOT_OF[i] for i in alive], n_betas, coeff, th, be, ca)
        assert state.bands_intact() and th.bands_intact() and be.bands_intact() and ca.bands_intact()
        got, now = [_vals(g) for g in (th, be, ca)], _vals(state)
        for r, i in enumerate(alive):
            name = cs[i]['name']
            want, want_row = ref[name][f]
            worst.take(TC.output_ratios(got[0][r], got[1][r], got[2][r], want, name))
            row = now[SLOT_OF[i]]
            assert row[0] == 1.0
            assert _same(row[1 + 9:1 + D], np.concatenate([x[0][r][3:], x[1][r], x[2][r]])), (name, f)       # x_raw of the linear lanes
            assert _same(row[1 + D + 9:1 + 2 * D], np.concatenate([got[0][r][3:], got[1][r], got[2][r]])), (name, f)
            worst.take(TC.state_ratios(row, want_row, n_betas))
            if f == 0:
                assert not row[1 + 2 * D:].any() and _same(row[1:1 + D], row[1 + D:1 + 2 * D])               # passed through, edx = 0
        others = [r for r in range(ROWS) if r not in {SLOT_OF[i] for i in alive}]
        assert _same(now[others], prev[others]), f
        prev = now
    assert _same(prev[[r for r in range(ROWS) if r not in SLOT_OF]], _sentinel(ROWS - len(cs), stride))
    rest = prev[SLOT_OF[TC.NAMES.index('rest')]]
    assert not rest[1 + 2 * D:].any()                                                                          # at rest dx is exactly 0
    worst.within_bound('bank entry, n_betas %d, smooth_coeff %g' % (n_betas, coeff))


# ------------------------------------------------------------------------------------------------ the frames entry
def _case_tables(dev, n_betas, frames=TC.MAX_FRAMES, seed=11):
    """Every case a slot of a frames call: input rows shuffled over the whole call, entries shuffled per frame, slots not in row order;
    the entries past a frame's count name a live slot and a valid row, which a kernel that ran past the count would filter."""
    cs = TC.cases()
    cap = len(cs) + 1
    rs = np.random.RandomState(seed)
    slot_of = rs.permutation(cap)[:len(cs)]
    where = [(f, i) for f in range(frames) for i, c in enumerate(cs) if len(c['thetas']) > f]
    row_of = dict(zip(where, rs.permutation(len(where))))
    inputs = [np.zeros((len(where), w), np.float32) for w in (72, n_betas, 3)]
    count, rows, slots, who = [], np.zeros((frames, cap), np.int32), np.zeros((frames, cap), np.int32), {}
    for f in range(frames):
        alive = [i for i in range(len(cs)) if (f, i) in row_of]
        rs.shuffle(alive)
        count.append(len(alive))
        rows[f], slots[f] = row_of[(f, alive[0])], slot_of[alive[0]]
        for k, i in enumerate(alive):
            rows[f, k], slots[f, k], who[(f, k)] = row_of[(f, i)], slot_of[i], i
            for dst, key in zip(inputs, KEYS):
                dst[row_of[(f, i)]] = cs[i][key][f][:dst.shape[1]]
    return Tables(dev, cap, count, rows, slots, inputs), slot_of, who


@pytest.mark.parametrize('coeff', [3.0, 1.0])
@pytest.mark.parametrize('n_betas', [1, 10, 11, 16])
def test_frames_entry_against_float64(dev, n_betas, coeff):
    """romp_oneeuro_smooth_frames over the same cases as ONE call of T frames, as T calls of one frame and split (2, T - 2): equal
    bits in the outputs and in the final state, all within bound of float64; output rows k >= count keep the sentinel.  State words 0
    (first report) and 1 (the later calls of the split runs)."""
    from romp_amd import lib as L
    cs, ref = TC.cases(), _ref64(n_betas, coeff)
    tab, slot_of, who = _case_tables(dev, n_betas)
    T, cap = tab.T, tab.capacity
    stride = L.load().romp_oneeuro_state_floats(n_betas)
    spare = [s for s in range(cap) if s not in slot_of]
    init = np.zeros((cap, stride), np.float32)
    init[spare] = SENTINEL_F32
    runs = []
    for splits in (None, [(t, 1) for t in range(T)], [(0, 2), (2, T - 2)]):
        state, outs = _guarded(dev, init), tab.outputs()
        tab.run(state, coeff, outs, splits)
        assert state.bands_intact()
        tab.check_untouched_outputs(outs)
        runs.append([_vals(g) for g in outs] + [_vals(state)])
    for other in runs[1:]:
        assert all(_same(a, b) for a, b in zip(runs[0], other))
    th, be, ca, st = runs[0]
    worst = Worst()
    for (f, k), i in who.items():
        e = f * cap + k
        worst.take(TC.output_ratios(th[e], be[e], ca[e], ref[cs[i]['name']][f][0], cs[i]['name']))
    for i, c in enumerate(cs):
        row = st[slot_of[i]]
        assert row[0] == 1.0
        worst.take(TC.state_ratios(row, ref[c['name']][len(c['thetas']) - 1][1], n_betas))
    assert _same(st[spare], init[spare])
    worst.within_bound('frames entry, n_betas %d, smooth_coeff %g' % (n_betas, coeff))


# ------------------------------------------------------------------------------------------------ state words
WORD_T, WORD_CAP, WORD_NB = 4, 3, 10


def _word_inputs():
    """Twelve estimates (frames 0..3 of three cases) and three more (their frame 4) that give every slot a history."""
    names = ('random_s3', 'flip', 'y_2.5')
    take = lambda f: [np.stack([TC.case(n)[k][f][:WORD_NB] if k == 'betas' else TC.case(n)[k][f] for n in names]) for k in KEYS]
    frames = [take(f) for f in range(WORD_T)]
    return [np.concatenate([fr[j] for fr in frames]) for j in range(3)], take(4)


def _run_words(dev, word, count, reports, coeff=3.0, splits=None):
    """Slots with a history and `word` in front of it; reports[slot] = the frames at which the slot is reported.  The call against
    simulate_frames: what is filtered, with which history, the final words and rows.  -> (Worst, state before, state after, the
    simulation)."""
    from romp_amd import lib as L
    inputs, warm = _word_inputs()
    rs = np.random.RandomState(int(abs(word) * 10) + sum(map(len, reports)))
    stride = L.load().romp_oneeuro_state_floats(WORD_NB)
    state = _guarded(dev, np.zeros((WORD_CAP, stride), np.float32))
    _bank(dev, state, range(WORD_CAP), WORD_NB, coeff, *(_guarded(dev, v) for v in warm))
    filters = {}
    for s in range(WORD_CAP):
        filters[s] = R64.make_filters(coeff)
        R64.smooth(filters[s], warm[0][s], warm[1][s], warm[2][s])
    state.inner[:, 0] = word
    before = _vals(state)
    rows, slots = np.zeros((WORD_T, WORD_CAP), np.int32), np.full((WORD_T, WORD_CAP), 1, np.int32)
    shuffle = rs.permutation(len(inputs[0]))                                    # slot s follows case s: its frame t lies in row shuffle[3 t + s]
    inputs = [np.empty_like(v) for v in inputs]
    for dst, src in zip(inputs, _word_inputs()[0]):
        dst[shuffle] = src
    for t in range(WORD_T):
        here = [s for s in range(WORD_CAP) if t in reports[s]]
        rs.shuffle(here)
        assert len(here) >= min(count[t], WORD_CAP) or count[t] == 0
        for k, s in enumerate(here):
            rows[t, k], slots[t, k] = shuffle[WORD_CAP * t + s], s
    ran = {t for t0, n in splits or [(0, WORD_T)] for t in range(t0, t0 + n)}
    count = [c if t in ran else 0 for t, c in enumerate(count)]                 # (frames no call covers: as good as empty)
    tab = Tables(dev, WORD_CAP, count, rows, slots, inputs)
    outs = tab.outputs()
    tab.run(state, coeff, outs, splits)
    assert state.bands_intact()
    tab.check_untouched_outputs(outs)
    sim = R64.simulate_frames([word] * WORD_CAP, WORD_T, WORD_CAP, count, rows, slots, inputs, filters, coeff)
    assert {(e[0], e[1]) for e in sim['entries']} == tab.reported()
    th, be, ca = (_vals(g) for g in outs)
    after = _vals(state)
    worst = Worst()
    for t, k, slot, history, want in sim['entries']:
        e = t * WORD_CAP + k
        worst.take(TC.output_ratios(th[e], be[e], ca[e], want, 'words'))
        r = rows[t, k]
        passed = _same(np.concatenate([th[e][3:], be[e], ca[e]]), np.concatenate([inputs[0][r][3:], inputs[1][r], inputs[2][r]]))
        assert passed == (history != 'continued'), (t, k, slot, history)
    touched = {e[2] for e in sim['entries']}
    assert after[:, 0].tolist() == sim['words']
    for s in range(WORD_CAP):
        if s in touched:
            worst.take(TC.state_ratios(np.concatenate([[1.0], after[s][1:]]), R64.state_row(sim['filters'][s]), WORD_NB))
        else:
            assert _same(after[s][1:], before[s][1:]) and after[s][0] == (word if word >= 0 else 0.0)
    return worst, before, after, sim


def _patterns(pivot):
    """Reported before the pivot frame only, after it only, on both sides, never."""
    return {'before': list(range(pivot)), 'after': [min(pivot + 1, WORD_T - 1)], 'both': sorted({max(pivot - 1, 0), pivot, WORD_T - 1}),
            'never': []}


@pytest.mark.parametrize('word', [0.0, 1.0, -1.0, -3.0, -3.5, -1.5])
def test_state_word(dev, word):
    """One state word -- 0, 1, -(t + 1) for t = 0 and 2, -(t + 1.5) for t = 2 and 0 -- on slots reported before the restart frame
    only, after it only, on both sides and never (capacity 3, T = 4, two hand-written tables): what is filtered, with which
    history, and each slot's final word as simulate_frames has them."""
    pivot = int(-word) - 1 if word < 0 else 2
    p = _patterns(pivot)
    worst, histories, finals = Worst(), [], {}
    for kinds in (('before', 'after', 'both'), ('never', 'both', 'after')):
        reports = [p[k] for k in kinds]
        count = [sum(t in r for r in reports) for t in range(WORD_T)]
        w, _, after, sim = _run_words(dev, word, count, reports)
        worst.take(w)
        histories += [e[3] for e in sim['entries']]
        for k, s in zip(kinds, range(WORD_CAP)):
            finals[k] = after[s, 0]
    print('word %g: histories %s, final words %s' % (word, sorted(set(histories)), finals))
    if word < 0:
        assert finals['after'] == finals['both'] == 1.0 and finals['never'] == finals['before'] == 0.0 and 'restarted' in histories
        assert ('fresh' in histories) == (word != int(word) and pivot > 0) and ('continued' in histories)
    else:
        assert finals['never'] == word and finals['before'] == finals['after'] == finals['both'] == 1.0
        assert set(histories) == ({'fresh', 'continued'} if word == 0 else {'continued'})
    worst.within_bound('state word %g' % word)


def test_count_above_capacity(dev):
    """out_count[t] = capacity + 5: exactly `capacity` entries are filtered, nothing is written past them."""
    reports = [list(range(WORD_T))] * WORD_CAP
    worst, _, after, sim = _run_words(dev, 1.0, [WORD_CAP + 5] * WORD_T, reports)
    assert len(sim['entries']) == WORD_CAP * WORD_T and (after[:, 0] == 1.0).all()
    worst.within_bound('counts above the capacity')


def test_empty_frame_and_absent_slot(dev):
    """A frame with out_count[t] = 0 in the middle leaves every state row bit-unchanged across it (seen by running the frames one
    call each), changes nothing of the whole call's result, and a slot absent from every frame keeps its whole state row."""
    reports, count = [[0, 2, 3], [0, 3], []], [2, 0, 1, 2]
    worst, before, whole, _ = _run_words(dev, 1.0, count, reports)
    _, _, upto0, _ = _run_words(dev, 1.0, [2, 0, 0, 0], reports)
    _, _, upto1, _ = _run_words(dev, 1.0, count, reports, splits=[(0, 1), (1, 1)])
    _, _, split, _ = _run_words(dev, 1.0, count, reports, splits=[(t, 1) for t in range(WORD_T)])
    assert _same(upto0, upto1) and not _same(upto0, before)
    assert _same(split, whole)
    assert _same(whole[2], before[2]) and whole[2, 0] == 1.0
    worst.within_bound('an empty frame in the middle')


# ------------------------------------------------------------------------------------------------ non-finite values
NONFINITE = {'nan_root': ('thetas', 1, float('nan')), 'inf_beta': ('betas', 4, float('inf')), 'minus_inf_cam': ('cam', 0, float('-inf'))}


def _three_persons(kind):
    names = ('random_s3', 'flip', 'random_s1')
    x = [np.stack([TC.case(n)[k][:4, :WORD_NB] if k == 'betas' else TC.case(n)[k][:4] for n in names], 1).copy() for k in KEYS]   # (4, 3, w)
    key, lane, value = NONFINITE[kind]
    x[KEYS.index(key)][1, 1, lane] = value                                  # frame 1, the middle person
    return x


def _run_persons(dev, entry, x, persons, coeff=3.0):
    """Frames 0..3 of the given persons through one entry -> (outputs (4, P, w) x 3, final state rows (P, stride))."""
    from romp_amd import lib as L
    P = len(persons)
    stride = L.load().romp_oneeuro_state_floats(WORD_NB)
    state = _guarded(dev, np.zeros((P + 2, stride), np.float32))
    slots = [P + 1 - j for j in range(P)]
    if entry == 'bank':
        outs = [np.zeros((4, P, w), np.float32) for w in (72, WORD_NB, 3)]
        for f in range(4):
            bufs = [_guarded(dev, v[f][persons]) for v in x]
            _bank(dev, state, slots, WORD_NB, coeff, *bufs)
            assert all(b.bands_intact() for b in bufs)
            for o, b in zip(outs, bufs):
                o[f] = _vals(b)
    else:
        cap = P + 2
        rows, sl = np.zeros((4, cap), np.int32), np.zeros((4, cap), np.int32)
        for f in range(4):
            rows[f, :P], sl[f, :P] = [f * P + j for j in range(P)], slots
        tab = Tables(dev, cap, [P] * 4, rows, sl, [v[:, persons].reshape(4 * P, -1) for v in x])
        bufs = tab.outputs()
        tab.run(state, coeff, bufs)
        tab.check_untouched_outputs(bufs)
        outs = [_vals(b).reshape(4, cap, -1)[:, :P] for b in bufs]
    assert state.bands_intact()
    st = _vals(state)
    assert not st[0].any()                                                   # row 0 is nobody's
    return outs, st[slots]


@pytest.mark.parametrize('kind', sorted(NONFINITE))
@pytest.mark.parametrize('entry', ['bank', 'frames'])
def test_nonfinite_stays_with_its_person(dev, entry, kind):
    """A NaN root component, +inf in one beta or -inf in cam[0] of the middle of three persons at frame 1: the other two give the
    bits of a run without that person, outputs and states; the middle one is NaN / infinite exactly where the float32 oracle is,
    its root axis-angle 0 where the oracle's NaN -> 0 applies, its finite lanes within bound of float64, its state word still 1."""
    x = _three_persons(kind)
    outs, st = _run_persons(dev, entry, x, [0, 1, 2])
    outs2, st2 = _run_persons(dev, entry, x, [0, 2])
    for a, b in zip(outs, outs2):
        assert _same(a[:, [0, 2]], b)
    assert _same(st[[0, 2]], st2)
    f32, f64, worst = TO.make_filters(3.0), R64.make_filters(3.0), Worst()
    with np.errstate(all='ignore'):
        for f in range(4):
            mine = [v[f, 1] for v in x]
            want = [v.numpy() for v in TO.smooth(f32, *(torch.from_numpy(v.copy()) for v in mine))]
            ref = R64.smooth(f64, *mine)
            for got, w, r, seg in zip((outs[0][f, 1], outs[1][f, 1], outs[2][f, 1]), want, ref, ('pose', 'betas', 'cam')):
                assert np.array_equal(np.isnan(got), np.isnan(w)) and np.array_equal(np.isinf(got), np.isinf(w)), (f, seg)
                assert np.array_equal(got[np.isinf(w)], w[np.isinf(w)])
                ok = np.isfinite(w)
                if seg == 'pose':
                    ok[:3] = False
                    if kind == 'nan_root' and f >= 1:
                        assert not got[:3].any() and not w[:3].any()
                    else:
                        worst.take({'root': TC.ratio(R64.rodrigues9(got[:3]), R64.rodrigues9(r[:3])), 'aa': TC.ratio(got[:3], r[:3])})
                worst.take({seg: TC.ratio(got[ok], r[ok])})
    assert st[1, 0] == 1.0 and not np.isfinite(st[1]).all() and np.isfinite(st[[0, 2]]).all()
    worst.within_bound('%s entry, %s' % (entry, kind))


# ------------------------------------------------------------------------------------------------ repeatability
@pytest.mark.parametrize('entry', ['bank', 'frames'])
def test_repeatable_on_a_side_stream(dev, entry):
    """The same inputs from the same starting state twice, the second time on a side stream: equal bits."""
    cs = TC.cases()
    results = []
    for stream in (torch.cuda.current_stream(dev), torch.cuda.Stream(dev)):
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            if entry == 'bank':
                stride = 1 + 3 * (81 + 16)
                state = _guarded(dev, np.zeros((len(cs), stride), np.float32))
                got = []
                for f in range(3):
                    bufs = [_guarded(dev, np.stack([c[k][f] for c in cs])) for k in KEYS]
                    _bank(dev, state, range(len(cs)), 16, 3.0, *bufs)
                    got += [_vals(b) for b in bufs]
            else:
                tab, _, _ = _case_tables(dev, 16, frames=3)
                state, bufs = _guarded(dev, np.zeros((tab.capacity, 1 + 3 * (81 + 16)), np.float32)), tab.outputs()
                tab.run(state, 3.0, bufs)
                got = [_vals(b) for b in bufs]
            stream.synchronize()
            results.append(got + [_vals(state)])
        torch.cuda.synchronize(dev)
    assert all(_same(a, b) for a, b in zip(*results))
    assert (results[0][-1][:len(cs), 0] == 1.0).sum() >= len(cs) - 1
