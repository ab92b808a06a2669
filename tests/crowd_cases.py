"""Crowd-mode merge (csrc/crowd.hip): the numpy restatement, its float64 twin and the named edge cases -- TEST INFRASTRUCTURE ONLY.

Restatement: points 6-9 of bev/main.py:process_long_image with bev/split2process.py and bev/post_parser.py, in the reference's
float32 operation order.  It follows the reference's comparisons where they matter for non-finite values: the pair scale is
`where(ps1 > ps2, ps1, ps2)` (not a NaN-propagating maximum), `center_confs[a] < center_confs[b]` decides who goes (false on a tie
and on NaN: the later row goes), the sort of remove_outlier puts NaN last.  Per stage it reports the removed rows and, for the two
suppressions, every pair (a, b) that removed someone.  tests/golden/bev_crowd_edges.npz (scripts/make_golden_bev_crowd_edges.py:
the reference's own stage functions on the crafted cases below) pins it.

Cases: every builder returns a list of case dicts (inputs, 'res': the restatement's result, 'prop': what the case is for) and
asserts that property itself from the restatement.  Random builders take the first of 20 seeds whose margin (the smallest relative
distance of any compared value to its threshold) exceeds 1e-5; crafted ones place their values exactly or assert a margin of 1e-3.

What cannot be built: an exact tie of a pair distance with the suppression threshold (71 rounded square roots and a rounded mean
stand between the inputs and the distance; there is no input for which every implementation's distance is the threshold itself),
and overlapping offset ranges (two workgroups of the crop stage would race on the shared rows; the ABI's clamps only ever make
ranges empty when offsets are non-decreasing, which is all the callers produce).
"""
import functools

import numpy as np

from oracle import bev_post_oracle as PO

F32 = np.float32
INF = float('inf')


# ----------------------------------------------------------------------------------------------- numpy restatement
def split_plan(h, w_pad, overlap):
    """get_image_split_plan on the padded width (left, right, top, bottom; int32 truncation; the last crop keeps the previous
    step's right)."""
    n = int(np.ceil((w_pad / h - 1) / (1 - overlap))) + 1
    step = (1 - overlap) * h
    boxes, right = [], None
    for i in range(n):
        if i == n - 1:
            left = w_pad - h
        else:
            left = step * i
            right = left + h
        boxes.append([left, right, 0, h])
    return np.array(boxes).astype(np.int32)


def frame_pad_info(h, w):
    top = (w - h) // 2
    return np.array([top, w - top, 0, w, h, w], F32)


def crop_pad_info(ch, cw):
    side = max(ch, cw)
    top, left = (side - ch) // 2, (side - cw) // 2
    return np.array([top, top + ch, left, left + cw, ch, cw], F32)


def _margin(margins, x, thr):
    x = np.asarray(x, np.float64).ravel()
    x = x[np.isfinite(x)]                                              # (a non-finite value compares the same whatever the rounding)
    if x.size:
        margins.append(float(np.min(np.abs(x / float(thr) - 1))))


def _pair_dist(p, sc):
    """pj2d_dist_mat_normalized, 64 rows at a time (every entry is computed as in one piece)."""
    n = len(p)
    d = np.empty((n, n), F32)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(0, n, 64):
            d[i:i + 64] = np.sqrt(((p[i:i + 64, None] - p[None]) ** 2).sum(-1)).mean(-1).astype(F32)
        s1, s2 = sc[:, None], sc[None]
        return d / np.where(s1 > s2, s1, s2)


def _suppress(pj_org, cam, conf, alive, thr, margins):
    """conf-based suppressing_redundant_prediction_via_projection over the rows `alive` (row order).
    -> removed rows (mask), pairs [(removed row, row a, row b, list position a, list position b, list length)]."""
    idx = np.nonzero(alive)[0]
    out = np.zeros(len(alive), bool)
    if len(idx) < 2:
        return out, []
    d = _pair_dist(pj_org[idx], cam[idx, 0] * F32(2))
    _margin(margins, d[np.triu_indices(len(idx), 1)], F32(thr))
    with np.errstate(invalid='ignore'):
        a, b = np.nonzero(np.triu(d < F32(thr), 1))
        drop = np.where(conf[idx[a]] < conf[idx[b]], idx[a], idx[b])
    out[drop] = True
    return out, [(int(r), int(idx[i]), int(idx[j]), int(i), int(j), len(idx)) for r, i, j in zip(drop, a, b)]


def _outlier(trans, cam, alive, rel_thresh, scale_thresh, margins):
    idx = np.nonzero(alive)[0]
    out = np.zeros(len(alive), bool)
    m = len(idx)
    if m < 3:
        return out
    t = trans[idx]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        dm = np.sqrt(((t[:, None] - t[None]) ** 2).sum(-1)).astype(F32)
        mean = np.sort(dm, 1)[:, 1:-1].mean(1).astype(F32)
        rel = mean / ((mean.sum() - mean) / F32(m - 1))
        small = cam[idx, 0] < F32(scale_thresh)
        _margin(margins, rel[small], F32(rel_thresh))
        out[idx[(rel > F32(rel_thresh)) & small]] = True
    return out


def crop_bounds(crops, c, H):
    """The float32 cam_x bounds of crop c: rows with cam_x > hi or cam_x < lo go (None: no such bound)."""
    K = len(crops)
    hi = F32(1 - (int(crops[c][1]) - int(crops[c + 1][0])) / H / 2) if c != K - 1 else None
    lo = F32((int(crops[c - 1][1]) - int(crops[c][0])) / H / 2 - 1) if c >= 2 else None
    return hi, lo


def crop_camera(crops, c, H, W, pad_length):
    """convert_crop_cam_params2full_image's float32 scale and shift of crop c."""
    l, r, t, b = [int(v) for v in crops[c]]
    return F32(max(r - l, b - t) / max(H, W)), F32(np.mean([l - pad_length, r - pad_length]) / (W / 2) - 1)


def crowd_merge(crop_id, cam, conf, joints, crops, H, W, pad_length, nms=20., rel=1.6):
    """Points 6-9 of process_long_image on per-row detections (rows crop-major; crop_id -1: a row no crop covers, dropped).
    -> dict(keep, cam_full, cam_trans, pj2d_org, stages: how many rows each step removed, margin: the smallest relative distance
    of a compared value to its threshold, margin_computed: the same without the cam_x bounds (a case may place cam_x on one),
    keep1: the crop-stage survivors, removed: per stage the removed rows -- excluded [(row, 'hi' | 'lo')], crop_suppressed / suppressed [(row, a, b, pos a, pos b, list length)], crop_outliers / outliers [row])."""
    cam, conf, joints = np.asarray(cam, F32), np.asarray(conf, F32), np.asarray(joints, F32)
    crop_id = np.asarray(crop_id)
    K, N = len(crops), len(cam)
    alive = crop_id >= 0
    cam_full = cam.copy()
    st = dict(excluded=0, crop_suppressed=0, crop_outliers=0, suppressed=0, outliers=0)
    removed = dict(excluded=[], crop_suppressed=[], crop_outliers=[], suppressed=[], outliers=[])
    margins, placed = [], []
    for c in range(K):
        rows = crop_id == c
        if not rows.any():
            continue
        l, r, t, b = [int(v) for v in crops[c]]
        hi, lo = crop_bounds(crops, c, H)
        with np.errstate(invalid='ignore'):
            if hi is not None:
                _margin(placed, cam[rows, 2], hi)
                ex = rows & (cam[:, 2] > hi)
                st['excluded'] += int(ex.sum()); alive &= ~ex
                removed['excluded'] += [(int(i), 'hi') for i in np.nonzero(ex)[0]]
            if lo is not None:
                _margin(placed, cam[rows & alive, 2], lo)
                ex = rows & alive & (cam[:, 2] < lo)
                st['excluded'] += int(ex.sum()); alive &= ~ex
                removed['excluded'] += [(int(i), 'lo') for i in np.nonzero(ex)[0]]
        ch, cw = b - t, r - l
        sel = np.nonzero(rows)[0]
        pj, tr = np.zeros((N, joints.shape[1], 2), F32), np.zeros((N, 3), F32)
        with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
            _, pj[sel], tr[sel] = PO.project(joints[sel], cam[sel], [0, ch, 0, cw, ch, cw])
        rm, pairs = _suppress(pj, cam, conf, rows & alive, nms * max(ch, cw) / 640, margins)
        st['crop_suppressed'] += int(rm.sum()); alive &= ~rm
        removed['crop_suppressed'] += pairs
        rm = _outlier(tr, cam, rows & alive, rel, 1, margins)
        st['crop_outliers'] += int(rm.sum()); alive &= ~rm
        removed['crop_outliers'] += [int(i) for i in np.nonzero(rm)[0]]
        scale, shift = crop_camera(crops, c, H, W, pad_length)
        with np.errstate(invalid='ignore', over='ignore'):
            cam_full[rows] = cam[rows] * scale
            cam_full[rows, 2] += shift
    keep1 = alive.copy()
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        _, pj, tr = PO.project(joints, cam_full, frame_pad_info(H, W))
    rm, pairs = _suppress(pj, cam_full, conf, alive, nms * max(H, W) / 640, margins)
    st['suppressed'] = int(rm.sum()); alive &= ~rm
    removed['suppressed'] = pairs
    rm = _outlier(tr, cam_full, alive, rel, 0.5, margins)
    st['outliers'] = int(rm.sum()); alive &= ~rm
    removed['outliers'] = [int(i) for i in np.nonzero(rm)[0]]
    return {'keep': alive, 'cam_full': cam_full, 'cam_trans': tr, 'pj2d_org': pj, 'stages': st,
            'margin': min(margins + placed + [1.]), 'margin_computed': min(margins + [1.]), 'keep1': keep1, 'removed': removed}


def twin64(crop_id, cam, joints, crops, H, W, pad_length):
    """The camera conversion, translation and full-frame projection in float64 on the float32 inputs and the float32 per-crop
    constants (the reference multiplies and adds them as float32 scalars).  -> cam_full, cam_trans, pj2d_org; rows no crop covers
    are NaN."""
    cam64 = np.asarray(cam, F32).astype(np.float64)
    cam_full = np.full(cam64.shape, np.nan)
    for c in range(len(crops)):
        rows = np.asarray(crop_id) == c
        scale, shift = crop_camera(crops, c, H, W, pad_length)
        with np.errstate(invalid='ignore', over='ignore'):
            cam_full[rows] = cam64[rows] * np.float64(scale)
            cam_full[rows, 2] += np.float64(shift)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        _, pj, tr = PO.project(np.asarray(joints, F32).astype(np.float64), cam_full, frame_pad_info(H, W), dtype=np.float64)
    return cam_full, tr, pj


def crop_id_from_offsets(offsets, N, K):
    """The ABI's reading of `offsets`: crop c owns rows [clamp(offsets[c], 0, N), clamp(offsets[c + 1], that, N))."""
    cid = np.full(N, -1, np.int32)
    for c in range(K):
        o0 = min(max(int(offsets[c]), 0), N)
        o1 = min(max(int(offsets[c + 1]), o0), N)
        assert np.all(cid[o0:o1] == -1), 'overlapping offset ranges are not a case (two workgroups would race)'
        cid[o0:o1] = c
    return cid


# ------------------------------------------------------------------------------------------------------ case tools
BASES = (np.random.RandomState(7).randn(24, 71, 3) * [0.25, 0.45, 0.1]).astype(F32)      # 24 unlike bodies


def make_case(name, H, W, pad_length, crops, rows, prop, offsets=None, nms=20., rel=1.6):
    """rows: [(crop, cam triple, joints (71, 3), conf[, tag])], put into crop order (stable).  `offsets`: given explicitly for the
    offsets cases (then `rows` are in memory order and their crop entry is ignored)."""
    crops = np.ascontiguousarray(crops, np.int32)
    K = len(crops)
    if offsets is None:
        rows = sorted(rows, key=lambda r: r[0])
        counts = np.bincount(np.array([r[0] for r in rows], np.int64), minlength=K)
        offsets = np.concatenate([[0], np.cumsum(counts)])
    N = len(rows)
    offsets = np.asarray(offsets, np.int32)
    case = {'name': name, 'H': H, 'W': W, 'pad_length': pad_length, 'crops': crops, 'offsets': offsets, 'N': N, 'K': K,
            'nms': nms, 'rel': rel, 'prop': prop,
            'cam': np.array([r[1] for r in rows], F32).reshape(N, 3), 'conf': np.array([r[3] for r in rows], F32),
            'joints': np.array([r[2] for r in rows], F32).reshape(N, 71, 3),
            'tags': {r[4]: i for i, r in enumerate(rows) if len(r) > 4}}
    case['crop_id'] = crop_id_from_offsets(offsets, N, K)
    with np.errstate(all='ignore'):
        case['res'] = crowd_merge(case['crop_id'], case['cam'], case['conf'], case['joints'], crops, H, W, pad_length, nms, rel)
    return case


def twin_of(case):
    return twin64(case['crop_id'], case['cam'], case['joints'], case['crops'], case['H'], case['W'], case['pad_length'])


def describe(case):
    r = case['res']
    counts = np.bincount(case['crop_id'][case['crop_id'] >= 0], minlength=case['K'])
    return '%s: N %d, K %d, max per crop %d, crop-stage survivors %d, kept %d, stages %s, margin %.1e' % (
        case['name'], case['N'], case['K'], counts.max() if len(counts) else 0, int(r['keep1'].sum()), int(r['keep'].sum()),
        r['stages'], r['margin'])


def _first_seed(build, what):
    """The margin rule of the random cases: the first of 20 seeds whose restatement margin exceeds 1e-5."""
    for seed in range(20):
        case = build(seed)
        if case is not None and case['res']['margin'] > 1e-5:
            case['seed'] = seed
            return case
    raise AssertionError('%s: no seed among 20 with a margin above 1e-5' % what)


def _random_rows(rs, crop_counts, spread=0.03, nbases=8, x=(-1.1, 1.1), scale=(0.2, 1.2), remote=0.1):
    """Detections like those of tests/test_bev_crowd.py: a few body shapes with noise, some remote tiny persons."""
    rows = []
    base = (rs.randn(nbases, 71, 3) * [0.25, 0.45, 0.1]).astype(F32)
    for c, n in crop_counts:
        for _ in range(n):
            s = 0.04 if rs.rand() < remote else rs.uniform(*scale)
            cam = [s, rs.uniform(-0.5, 0.5), rs.uniform(*x)]
            rows.append((c, cam, base[rs.randint(nbases)] + rs.randn(71, 3) * spread, rs.uniform(0.05, 0.95)))
    return rows


def hand_crops(K, H, step=40, width=120):
    """K overlapping crops of unequal width, top and bottom (the ABI takes any crop inside the padded frame)."""
    crops = []
    for c in range(K):
        l = step * c
        crops.append([l, l + width - 7 * (c % 3), c % 4, H - (c % 5)])
    return np.array(crops, np.int32)


def _excl(res, c, crop_id):
    return {k for r, k in res['removed']['excluded'] if crop_id[r] == c}


# --------------------------------------------------------------------------------------------------- the seam cases
def _seam(K):
    H, pl = 120, 60
    crops = hand_crops(K, H)
    W = int(crops[:, 1].max()) - 2 * pl
    peopled = [c for c in (62, 63, 64, 65, 66, 127, 128) if c < K]

    def build(seed):
        rs = np.random.RandomState(1000 * K + seed)
        rows = _random_rows(rs, [(c, rs.randint(40, 90)) for c in peopled], nbases=12)
        return make_case('seam%d' % K, H, W, pl, crops, rows, 'K = %d hand-made crops of unequal width, top and bottom; people in '
                         'crops %s; rows go by the upper and the lower bound on both sides of each seam' % (K, peopled))

    case = _first_seed(build, 'seam%d' % K)
    res, cid = case['res'], case['crop_id']
    assert len({(r - l, t, b) for l, r, t, b in crops.tolist()}) > 6          # unequal width, top and bottom
    for c in peopled:
        want = {'hi', 'lo'} if c != K - 1 else {'lo'}
        assert _excl(res, c, cid) == want, (K, c, _excl(res, c, cid))
    assert res['stages']['crop_suppressed'] > 0 and res['stages']['crop_outliers'] > 0
    for c in peopled:                                                  # crop-stage survivors on both sides of every seam
        assert (res['keep1'] & (cid == c)).any(), c
    return [case]


def seam64():
    return _seam(64)


def seam65():
    return _seam(65)


def seam129():
    return _seam(129)


def plan71():
    H, W, ov = 300, 4000, 0.8
    pl = int(H * ov)
    crops = split_plan(H, W + 2 * pl, ov)
    assert len(crops) == 71

    def build(seed):
        rs = np.random.RandomState(7100 + seed)
        return make_case('plan71', H, W, pl, crops, _random_rows(rs, [(c, rs.randint(0, 7)) for c in range(71)], spread=0.05),
                         'the 71-crop plan of a 300 x 4000 frame, 0-6 people per crop')

    case = _first_seed(build, 'plan71')
    cid = case['crop_id']
    assert (cid >= 64).any() and (cid < 64).any() and case['res']['stages']['excluded'] > 0
    assert any(cid[r] >= 64 for r, _ in case['res']['removed']['excluded'])
    return [case]


def _compaction_property(case, c, what):
    """In crop c, a row suppressed at list position >= 256 (the list: the rows the boundary left, in row order) and a survivor
    behind it."""
    res, cid = case['res'], case['crop_id']
    pos = [max((pa if r == a else pb) for rr, a, b, pa, pb, _ in res['removed']['crop_suppressed'] if rr == r)
           for r in {p[0] for p in res['removed']['crop_suppressed']} if cid[r] == c]
    late = [p for p in pos if p >= 256]
    assert late, '%s: no crop-stage removal at a list position >= 256' % what
    excluded = {r for r, _ in res['removed']['excluded']}
    lst = [r for r in np.nonzero(cid == c)[0] if r not in excluded]
    assert any(res['keep1'][r] for r in lst[min(late) + 1:]), '%s: no survivor behind a removed row of a later chunk' % what
    return len(late)


def big_crop():
    H, W, ov = 512, 1024, 0.46
    pl = int(H * ov)
    crops = split_plan(H, W + 2 * pl, ov)
    assert len(crops) == 5

    def build(seed):
        rs = np.random.RandomState(300 + seed)
        counts = [(0, 4), (1, 3), (2, 300), (3, 5), (4, 2)]
        return make_case('big_crop', H, W, pl, crops, _random_rows(rs, counts, nbases=24, x=(-0.75, 0.75), remote=0.03),
                         'a crop of 300 rows: the second chunk of the 256-thread compaction, in place')

    case = _first_seed(build, 'big_crop')
    _compaction_property(case, 2, 'big_crop')
    return [case]


def one_crop_1000():
    H = W = 512

    def build(seed):
        rs = np.random.RandomState(1000 + seed)
        return make_case('one_crop_1000', H, W, 0, [[0, W, 0, H]], _random_rows(rs, [(0, 1000)], nbases=32, remote=0.02),
                         'K = 1 with 1000 rows: four compaction chunks, a crop-stage pair loop of 10^6 pairs')

    case = _first_seed(build, 'one_crop_1000')
    assert case['res']['stages']['excluded'] == 0 and case['res']['stages']['crop_suppressed'] > 0
    _compaction_property(case, 0, 'one_crop_1000')
    return [case]


# --------------------------------------------------------------------------------------------- the global grid stride
FIRST_PASS = 2048 * 256            # pairs of crowd_pairs_kernel's first grid pass


def _neighbour_cam(cam, crops, c, c2, H, W, pl):
    """The camera that crop c2 would report for the full-frame person that crop c reports as `cam`."""
    s1, h1 = [np.float64(v) for v in crop_camera(crops, c, H, W, pl)]
    s2, h2 = [np.float64(v) for v in crop_camera(crops, c2, H, W, pl)]
    cam = np.asarray(cam, np.float64)
    return [cam[0] * s1 / s2, cam[1] * s1 / s2, (cam[2] * s1 + h1 - h2) / s2]


def _global_stride(name, K, per_crop, planted, far_last, prop):
    H, pl, step = 120, 60, 40
    crops = np.array([[step * c, step * c + 120, 0, H] for c in range(K)], np.int32)
    W = int(crops[-1, 1]) - 2 * pl

    def build(seed):
        rs = np.random.RandomState(52 * K + seed)
        rows = []
        for c in range(K - 1 if far_last else K):
            for i in range(per_crop):
                cam = [rs.uniform(0.3, 0.45), rs.uniform(-0.6, 0.6), rs.uniform(-0.6, 0.6)]
                rows.append((c, cam, BASES[rs.randint(24)] + rs.randn(71, 3) * 0.03, rs.uniform(0.05, 0.95)))
        for n, c in enumerate(planted):                                # the same person seen by crops c and c + 1
            cam = [0.4, 0.75 if n % 2 else -0.75, 0.33]                # (cam_y beyond everyone else's)
            j = BASES[n % 24] * F32(0.8)
            rows.append((c, cam, j, 0.9, 'dup%d_a' % n))
            rows.append((c + 1, _neighbour_cam(cam, crops, c, c + 1, H, W, pl), j, 0.2, 'dup%d_b' % n))
        if far_last:                                                   # two rows: no crop-stage outlier pass for them
            rows.append((K - 1, [0.4, 0.1, 0.2], BASES[3], 0.5))
            rows.append((K - 1, [0.02, 0.1, -0.2], BASES[4], 0.6, 'far'))
        return make_case(name, H, W, pl, crops, rows, prop)

    return _first_seed(build, name)


def global_stride():
    a = _global_stride('global_stride', 40, 20, (2, 20, 35, 38), False,
                       'at least 725 crop-stage survivors: removals whose only pair lies beyond the first pass of the pair grid')
    res, tags = a['res'], a['tags']
    m = int(res['keep1'].sum())
    assert m >= 725 and m * m > FIRST_PASS, m
    for n in range(4):                                                 # both copies inside their bounds, alive after the crop stage
        assert res['keep1'][tags['dup%d_a' % n]] and res['keep1'][tags['dup%d_b' % n]]
    beyond = {}
    for r, ra, rb, pa, pb, mm in res['removed']['suppressed']:
        assert mm == m
        beyond.setdefault(r, []).append(pa * m + pb >= FIRST_PASS)
    a['only_beyond'] = sorted(r for r, v in beyond.items() if all(v))
    assert a['only_beyond'] and any(any(v) for v in beyond.values())
    assert tags['dup2_b'] in a['only_beyond'] and tags['dup3_b'] in a['only_beyond'] and tags['dup0_b'] in beyond

    b = _global_stride('global_stride_1024', 56, 20, (5, 50), True,
                       'more than 1024 crop-stage survivors and a global outlier at a list position >= 1024')
    res = b['res']
    assert int(res['keep1'].sum()) > 1024
    far = b['tags']['far']
    assert res['keep1'][far] and far in res['removed']['outliers'] and int(res['keep1'][:far].sum()) >= 1024
    return [a, b]


# ------------------------------------------------------------------------------------------------ the crafted frames
def frame9():
    """120 x 480 at overlap 0.46: 9 crops (the last 103 wide), bounds about +-0.77."""
    H, W, ov = 120, 480, 0.46
    pl = int(H * ov)
    crops = split_plan(H, W + 2 * pl, ov)
    assert len(crops) == 9
    return H, W, pl, crops


def _assert_crafted(case):
    assert case['res']['margin_computed'] >= 1e-3, (case['name'], case['res']['margin_computed'])
    return case


def _far(tag='far', conf=0.5, s=0.04):
    return [s, 0.1, 0.0], BASES[9], conf, tag


def counts():
    H, W, pl, crops = frame9()
    near = [([0.5, -0.3, 0.55], BASES[0], 0.7, 'p0'), ([0.55, 0.3, -0.5], BASES[1], 0.6, 'p1'), ([0.45, 0.4, -0.1], BASES[2], 0.8, 'p2')]
    cases = []
    for n in range(5):
        # (1) n rows alive entering the crop-stage suppression (and its outlier pass): the far person is the second of them
        alive = ([near[0], _far()] + near[1:])[:n]
        rows = [(3,) + p for p in alive] + [(3, [0.5, 0.0, 0.95], BASES[5], 0.9, 'x_hi'), (3, [0.5, 0.0, -0.95], BASES[6], 0.9, 'x_lo')]
        c = _assert_crafted(make_case('counts_crop_%d' % n, H, W, pl, crops, rows,
                                      '%d rows alive at the crop stage: the far person stays below 3' % n))
        res, t = c['res'], c['tags']
        assert {r for r, _ in res['removed']['excluded']} == {t['x_hi'], t['x_lo']} and not res['removed']['crop_suppressed']
        if n >= 2:
            assert (t['far'] in res['removed']['crop_outliers']) == (n >= 3) and res['keep'][t['far']] == (n < 3)
        cases.append(c)
        # (2) n rows alive entering the crop-stage outlier pass, after one duplicate went in the suppression
        if n >= 1:
            rows = [(3,) + p for p in alive] + [(3, alive[0][0], alive[0][1], 0.1, 'dup')]
            c = _assert_crafted(make_case('counts_crop_outlier_%d' % n, H, W, pl, crops, rows,
                                          '%d rows alive entering the crop-stage outlier pass after a suppression' % n))
            res, t = c['res'], c['tags']
            assert {p[0] for p in res['removed']['crop_suppressed']} == {t['dup']}
            if n >= 2:
                assert (t['far'] in res['removed']['crop_outliers']) == (n >= 3)
            cases.append(c)
        # (3) n rows alive entering the global suppression and outlier pass: one row per crop
        people = ([near[0], _far()] + near[1:])[:n]
        rows = [(1 + 2 * i,) + p for i, p in enumerate(people)]
        if n:
            c = _assert_crafted(make_case('counts_global_%d' % n, H, W, pl, crops, rows,
                                          '%d rows, one per crop: the far person goes in the global outlier pass from 3 on' % n))
            res, t = c['res'], c['tags']
            assert not res['removed']['crop_outliers'] and not res['removed']['suppressed'] and res['keep1'].all()
            if n >= 2:
                assert (t['far'] in res['removed']['outliers']) == (n >= 3)
            cases.append(c)
        # (4) ... after one cross-crop duplicate went in the global suppression
        if n >= 1:
            first = rows[0]
            rows = rows + [(2, _neighbour_cam(first[1], crops, 1, 2, H, W, pl), first[2], 0.1, 'dup')]
            c = _assert_crafted(make_case('counts_global_outlier_%d' % n, H, W, pl, crops, rows,
                                          '%d rows alive entering the global outlier pass after a suppression' % n))
            res, t = c['res'], c['tags']
            assert {p[0] for p in res['removed']['suppressed']} == {t['dup']} and res['keep1'].all()
            if n >= 2:
                assert (t['far'] in res['removed']['outliers']) == (n >= 3)
            cases.append(c)
    # the two scale thresholds: a square frame and one crop, so cam_full == cam
    sq = [[0, 120, 0, 120]]
    cluster = [([3.0, 0.4 * i - 0.4, 0.5 * i - 0.5], BASES[i], 0.5 + 0.1 * i, 'c%d' % i) for i in range(3)]
    for name, s, gone in (('between', 0.7, True), ('below', 0.04, True), ('above', 1.5, False)):
        rows = [(0,) + p for p in cluster] + [(0, [s, 0.0, 0.0], BASES[9], 0.5, 'far')]
        c = _assert_crafted(make_case('counts_scale_' + name, 120, 120, 0, sq, rows,
                                      'cam[0] = %g against the crop-stage scale threshold 1 and the global 0.5' % s))
        res, t = c['res'], c['tags']
        assert (t['far'] in res['removed']['crop_outliers']) == gone and not res['removed']['outliers']
        assert np.array_equal(c['res']['cam_full'], c['cam'])
        cases.append(c)
    # ... and the global 0.5 from both sides: the row is alone in its crop (no crop-stage pass) and a relative outlier among 4
    two = [[0, 120, 0, 120], [0, 120, 0, 120]]                       # two crops over the whole square frame: scale 1, shift 0
    for name, s, gone in (('global_between', 0.7, False), ('global_below', 0.4, True)):
        rows = [(0, [s, 0.0, 0.0], BASES[9], 0.5, 'far')] + [(1,) + p for p in cluster]
        c = _assert_crafted(make_case('counts_scale_' + name, 120, 120, 0, two, rows,
                                      'cam_full[0] = %g, alone in its crop, against the global scale threshold 0.5' % s))
        res, t = c['res'], c['tags']
        assert res['keep1'].all() and not res['removed']['suppressed'] and res['removed']['outliers'] == ([t['far']] if gone else [])
        assert np.array_equal(c['res']['cam_full'], c['cam'])
        cases.append(c)
    return cases


def ties():
    H, W, pl, crops = frame9()
    cases = []
    P = [([0.5, -0.4, -0.5], BASES[0]), ([0.5, 0.0, 0.0], BASES[1]), ([0.5, 0.4, 0.5], BASES[2])]
    rows = []
    for i, (ca, cb) in enumerate(((0.5, 0.5), (0.3, 0.6), (0.6, 0.3))):      # exact duplicates: d = 0
        rows += [(4, P[i][0], P[i][1], ca, 'a%d' % i), (4, P[i][0], P[i][1], cb, 'b%d' % i)]
    c = _assert_crafted(make_case('ties_duplicates', H, W, pl, crops, rows,
                                  'exact duplicates: equal conf removes the later row, else the lower conf goes'))
    t = c['tags']
    assert {p[0] for p in c['res']['removed']['crop_suppressed']} == {t['b0'], t['a1'], t['b2']}
    cases.append(c)

    d = 0.045                                                          # A~B and B~C (d about 2.7 of 3.75), A and C apart (5.4)
    rows = [(4, [0.5, 0.0, -d], BASES[1], 0.3, 'A'), (4, [0.5, 0.0, 0.0], BASES[1], 0.5, 'B'), (4, [0.5, 0.0, d], BASES[1], 0.7, 'C'),
            (4, [0.5, 0.45, 0.5], BASES[2], 0.4, 'bystander')]
    c = _assert_crafted(make_case('ties_chain', H, W, pl, crops, rows, 'a chain A~B~C: C removes B while B still removes A'))
    t = c['tags']
    got = {(p[0], p[1], p[2]) for p in c['res']['removed']['crop_suppressed']}
    assert got == {(t['A'], t['A'], t['B']), (t['B'], t['B'], t['C'])} and c['res']['keep'][t['C']]
    cases.append(c)

    hi, _ = crop_bounds(crops, 4, H)                                   # an excluded row suppresses nobody
    rows = [(4, [0.5, 0.0, float(hi) + 0.01], BASES[1], 0.9, 'out'), (4, [0.5, 0.0, float(hi) - 0.02], BASES[1], 0.2, 'in'),
            (4, [0.5, -0.4, -0.3], BASES[0], 0.5, 'bystander')]
    c = _assert_crafted(make_case('ties_excluded', H, W, pl, crops, rows, 'a boundary-excluded duplicate suppresses nobody'))
    t = c['tags']
    assert c['res']['removed']['excluded'] == [(t['out'], 'hi')] and not c['res']['removed']['crop_suppressed']
    assert c['res']['keep'][t['in']]
    cases.append(c)

    rows = []                                                          # cross-crop duplicates: the global tie rule
    for i, (ca, cb) in enumerate(((0.5, 0.5), (0.3, 0.6), (0.6, 0.3))):
        cam = [0.5, 0.4 * i - 0.4, 0.55]
        rows += [(2 + 2 * i, cam, BASES[i], ca, 'a%d' % i), (3 + 2 * i, _neighbour_cam(cam, crops, 2 + 2 * i, 3 + 2 * i, H, W, pl),
                                                            BASES[i], cb, 'b%d' % i)]
    c = _assert_crafted(make_case('ties_global', H, W, pl, crops, rows,
                                  'cross-crop duplicates: equal conf removes the later row, else the lower conf goes'))
    t = c['tags']
    assert c['res']['keep1'].all() and {p[0] for p in c['res']['removed']['suppressed']} == {t['b0'], t['a1'], t['b2']}
    cases.append(c)
    return cases


def _bound_rows(crops, H, which):
    """Per crop in `which`: cam_x at the float32 bound and at its float32 neighbours, every row another body at another cam_y."""
    rows, expect = [], {}
    for c in which:
        hi, lo = crop_bounds(crops, c, H)
        xs = []
        if hi is not None:
            xs += [('hi', hi, False), ('hi+', np.nextafter(hi, F32(2)), True), ('hi-', np.nextafter(hi, F32(-2)), False)]
        if lo is not None:
            xs += [('lo', lo, False), ('lo-', np.nextafter(lo, F32(-2)), True), ('lo+', np.nextafter(lo, F32(2)), False)]
        if lo is None:
            xs.append(('nolo', F32(-0.95), False))                     # crops 0 and 1: nothing is too far left
        for i, (tag, x, gone) in enumerate(xs):
            y = -0.55 + 0.22 * i + (0.11 if c % 2 else 0.)
            s = 1.2 if tag == 'nolo' else 0.5                          # (1.2: no crop-stage outlier, so the row is seen to stay)
            rows.append((c, [s, y, F32(x)], BASES[(6 * c + i) % 24], 0.3 + 0.1 * i, '%d%s' % (c, tag)))
            expect['%d%s' % (c, tag)] = gone
    return rows, expect


def bounds():
    H, W, pl, crops = frame9()
    K = len(crops)
    rows, expect = _bound_rows(crops, H, (0, 1, 2, K - 2, K - 1))
    c = _assert_crafted(make_case('bounds_k9', H, W, pl, crops, rows, 'cam_x equal to the float32 bounds and their neighbours in '
                                  'crops 0, 1, 2, K - 2, K - 1: both comparisons are strict, crops 0 and 1 have no lower bound'))
    gone = {r for r, _ in c['res']['removed']['excluded']}
    assert gone == {c['tags'][t] for t, g in expect.items() if g}
    assert sorted(t for t in expect if t[0] in '01' and 'lo' in t) == ['0nolo', '1nolo'] and '2lo' in expect and '%dhi' % (K - 1) not in expect
    cases = [c]
    far = lambda x, i, tag: ([0.5, 0.3 * i - 0.3, x], BASES[i], 0.5, tag)
    c = _assert_crafted(make_case('bounds_k1', 120, 240, 0, [[0, 240, 0, 120]], [(0,) + far(3., 0, 'p'), (0,) + far(-3., 1, 'm')],
                                  'K = 1: no bound at all'))
    assert not c['res']['removed']['excluded']
    cases.append(c)
    c = _assert_crafted(make_case('bounds_k2', 120, 200, 0, [[0, 120, 0, 120], [80, 200, 0, 120]],
                                  [(0,) + far(3., 0, 'p0'), (0,) + far(-3., 1, 'm0'), (1,) + far(3., 2, 'p1'), (1,) + far(-3., 3, 'm1')],
                                  'K = 2: crop 0 has the upper bound only, crop 1 (the last, and c < 2) none'))
    assert c['res']['removed']['excluded'] == [(c['tags']['p0'], 'hi')]
    cases.append(c)
    return cases


def geometry():
    cases = []

    def planned(name, H, W, ov, prop, seed0):
        pl = int(H * ov)
        crops = split_plan(H, W + 2 * pl, ov)
        return _first_seed(lambda seed: make_case(name, H, W, pl, crops, _random_rows(
            np.random.RandomState(seed0 + seed), [(c, np.random.RandomState(seed0 + seed + c).randint(0, 7)) for c in range(len(crops))],
            spread=0.05), prop), name)

    c = planned('geometry_tall', 900, 700, 0.8, 'H > W: a negative top (Python floor division), max(H, W) = H', 900)
    assert frame_pad_info(900, 700)[0] == -100 and c['res']['stages']['excluded'] > 0
    cases.append(c)

    def hand(name, H, W, pl, step, width, prop, seed0):
        K = (W + 2 * pl - width) // step + 1
        crops = np.array([[step * i, step * i + width, i % 3, H - (i % 2)] for i in range(K)], np.int32)
        return _first_seed(lambda seed: make_case(name, H, W, pl, crops, _random_rows(
            np.random.RandomState(seed0 + seed), [(i, 4) for i in range(K)], spread=0.05), prop), name)

    c = hand('geometry_nopad', 120, 600, 0, 60, 120, 'pad_length 0; crops with top > 0 and bottom < H', 10)
    assert (c['crops'][:, 2] > 0).any() and (c['crops'][:, 3] < 120).any()
    cases.append(c)
    for H, W in ((120, 601), (120, 600), (301, 120), (300, 120)):      # W - H = 481, 480, -181, -180: tops 240, 240, -91, -90
        width = min(H, 120)
        c = hand('geometry_%dx%d' % (H, W), H, W, 30, 30, width, 'W - H = %d: the floor division of the frame pad' % (W - H), H + W)
        assert frame_pad_info(H, W)[0] == (W - H) // 2
        cases.append(c)
    assert frame_pad_info(301, 120)[0] == -91                         # (truncation would give -90)
    return cases


def offsets():
    H, W, pl, crops = frame9()
    K = len(crops)
    rs = np.random.RandomState(5)
    people = [(0, [0.5, 0.25 * (i % 5) - 0.5, 0.3 * (i % 4) - 0.45], BASES[i % 24], rs.uniform(0.1, 0.9)) for i in range(14)]
    cases = []
    off = [0, 2, 4, 5, 7, 8, 9, 10, 11, 11]                            # offsets[K] = 11 < N = 14
    c = _assert_crafted(make_case('offsets_tail', H, W, pl, crops, people, 'offsets[K] < N: the tail rows get keep 0', offsets=off))
    assert not c['res']['keep'][11:].any() and c['res']['keep'][:11].any() and (c['crop_id'][11:] == -1).all()
    cases.append(c)
    off = [0, 0, 0, 3, 6, 6, 6, 6, 14, 14]                             # empty crops first, last and in a run of three
    c = _assert_crafted(make_case('offsets_empty', H, W, pl, crops, people, 'empty crops at the front, the back and in a run of three',
                                  offsets=off))
    assert sorted(set(c['crop_id'].tolist())) == [2, 3, 7]
    cases.append(c)
    off = [-3, 2, 5, 7, 9, 11, 12, 13, 19, 40]                         # a negative entry, entries above N
    c = _assert_crafted(make_case('offsets_clamped', H, W, pl, crops, people, 'a negative offset and two above N: clamped to [0, N]',
                                  offsets=off))
    assert (c['crop_id'] >= 0).all() and c['crop_id'][0] == 0 and c['crop_id'][-1] == 7 and not (c['crop_id'] == 8).any()
    cases.append(c)
    assert K == 9
    return cases


NONFINITE_VALUES = (('nan', float('nan')), ('pinf', INF), ('ninf', -INF))


def nonfinite():
    """One row X at a time non-finite in one field.  X has an in-crop duplicate of higher and one of lower conf, a cross-crop
    duplicate in the next crop, and finite neighbours of which one pair is a duplicate and one is far (an outlier when the pass
    still works)."""
    H, W, pl, crops = frame9()
    K = len(crops)
    cases = []
    for field in ('cam0', 'cam2', 'joint', 'conf'):
        for vname, v in NONFINITE_VALUES:
            for cx in ((4,) if field != 'cam2' else (4, 0, K - 1)):
                nb = cx + 1 if cx < K - 1 else cx - 1                 # the crop that sees X too
                xc = [0.5, 0.0, 0.55 if nb > cx else 0.3]
                twin = _neighbour_cam(xc, crops, cx, nb, H, W, pl)
                rows = [(cx, list(xc), BASES[1].copy(), 0.5, 'X'), (cx, list(xc), BASES[1], 0.8, 'X_hi'), (cx, list(xc), BASES[1], 0.2, 'X_lo'),
                        (cx, [0.5, -0.45, -0.4], BASES[0], 0.6, 'n0'), (cx, [0.5, -0.45, -0.4], BASES[0], 0.4, 'n0_dup'),
                        (cx, [0.55, 0.45, -0.1], BASES[2], 0.7, 'n1'), (cx, [0.04, 0.1, 0.0], BASES[9], 0.5, 'far'),
                        (nb, twin, BASES[1], 0.65, 'X_next'), (nb, [0.5, 0.45, 0.3], BASES[3], 0.5, 'n2'),
                        (nb, [0.5, -0.45, 0.3], BASES[4], 0.5, 'n3')]
                x = rows[0]
                if field == 'cam0':
                    x[1][0] = v
                elif field == 'cam2':
                    x[1][2] = v
                elif field == 'joint':
                    x[2][17, 1] = v
                else:
                    rows[0] = x[:3] + (v,) + x[4:]
                c = _assert_crafted(make_case('nonfinite_%s_%s_crop%d' % (field, vname, cx), H, W, pl, crops, rows,
                                              '%s of one row is %s (crop %d of %d)' % (field, vname, cx, K)))
                t = c['tags']
                assert t['n0_dup'] in {p[0] for p in c['res']['removed']['crop_suppressed']}       # the finite pair still works
                cases.append(c)
    return cases


BUILDERS = {'seam64': seam64, 'seam65': seam65, 'seam129': seam129, 'plan71': plan71, 'big_crop': big_crop,
            'one_crop_1000': one_crop_1000, 'global_stride': global_stride, 'counts': counts, 'ties': ties, 'bounds': bounds,
            'geometry': geometry, 'offsets': offsets, 'nonfinite': nonfinite}
CRAFTED = ('counts', 'ties', 'bounds', 'offsets', 'nonfinite')
FIXTURE = ('ties', 'counts', 'bounds', 'nonfinite')                    # what tests/golden/bev_crowd_edges.npz holds


@functools.lru_cache(maxsize=None)
def cases(name):
    """The cases of one builder, built once per process and left unchanged."""
    return tuple(BUILDERS[name]())
