"""Golden fixture for the Relative Human scoring (tests/golden/relative_human.npz), written by the reference's own
RH_Evaluation (simple_romp/evaluation/RH_evaluation/{evaluation,matching}.py, imported read-only by path; its unused
`import cv2` gets an empty stand-in module, and torch.Tensor.cuda is the identity for the run because _calc_matched_PCKh_
calls .cuda()).

The script writes synthetic annotations and results in the reference's own pickled formats to a temporary folder, runs
RH_Evaluation on them under an alarm (its matcher spins forever once every pair is consumed) and stores what came out.
Numeric arrays only:

  inputs    names (B,24) uint8 (the image names, zero padded); ann_image, ann_joints (0: no 'kp2d', 14, 19), ann_kp (Na,19,3)
            (x, y, flag; zero padded), ann_depth_id, ann_age: one row per annotated person in file order; ann_as_list: images
            whose kp2d are stored as flat float lists; res_image, res_kp (Np,14,2), res_trans (Np,3): one row per predicted
            person; res_stacked: images whose results are a dict of stacked arrays rather than a list of persons
  outputs   match_<b> (M,2) (prediction, annotation index) and pckh_<b> (M,) per image with results, missed_<b>,
            pr_all / pr_fp / pr_miss (B,), prf1 (3,), eq_dist / cd_dist / fd_dist and eq_age / cd_age / fd_age (n,2) (the pair
            lists get_results received), missed_age, mPCKh (float32), PCRD and PCRD_age (4, NaN: not reported) (float32, as the
            reference returns them), printed (mPCKh, PCRD, ages: the figures of the results file, per cent, two decimals) and
            printed_eq_cd_fd (the "Equal / close / far" line)
  min_gap   the smallest relative distance of any error / scale from 0.143: asserted >= 1e-4, three orders above what a
            float32 sqrt and product can differ by between numpy and the device

Images (see scene()): 1, 2, 5, 12 and 64 matched people; an image missing from the results; one whose depth ids are all -1 and
one with a single valid id; equal ids; depths 0 against float32(0.2) and +-1 ulp; a person with one valid joint, one with a
valid joint at x <= -1, one whose visible joints coincide; ages -1 and 0..3; 14-joint, BK and OCHuman annotations; a far-away
false positive; a person without 'kp2d'.

Build container only (needs the reference checkout):  python scripts/make_golden_relative_human.py
The file regenerates bit for bit (fixed zip timestamps, sorted names).
"""
import contextlib
import io
import os
import re
import signal
import sys
import tempfile
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402

REFERENCE = os.path.dirname(mg.REF)
OUT = os.path.join(ROOT, 'tests', 'golden', 'relative_human.npz')
F = np.float32
J = 14
PCK_THRESH, MIN_GAP, ALARM_S = 0.143, 1e-4, 120
THR = F(0.2)
BK_TO_14 = [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 0, -1]
OCH_TO_14 = [3, 0, 4, 1, 5, 2, 9, 6, 10, 7, 11, 8, 12, -1]


def skeleton(rng, centre):
    return (np.asarray(centre, np.float64) + rng.standard_normal((J, 2)) * np.array([25.0, 50.0])).astype(F)


def near(rng, kp, px):
    return (kp.astype(np.float64) + px * rng.standard_normal(kp.shape)).astype(F)


def annot14(kp, flags=None):
    return np.concatenate([kp, np.ones((J, 1), F) if flags is None else np.asarray(flags, F).reshape(J, 1)], 1).astype(F)


def annot19(rng, kp, mapper):
    """A 19-joint annotation whose mapped joints are `kp` (the 14th target joint has no source: -1) and whose other joints
    are valid clutter that the mapping must leave out."""
    a = np.concatenate([skeleton(rng, kp.mean(0)), np.ones((J, 1), F)], 1)
    a = np.concatenate([a, a[:5]], 0).astype(F)
    for tgt, src in enumerate(mapper):
        if src >= 0:
            a[src, :2] = kp[tgt]
    return a


def scene(rng):
    """-> images: list of (name, persons, preds, stacked, as_list); a person is a dict kp (n,3) or None, depth_id, age; a pred
    (kp2ds (14,2), trans (3,)); preds None: the image is absent from the results."""
    images = []
    person = lambda kp, did, age: {'kp': kp, 'depth_id': did, 'age': age}
    pred = lambda kp, depth, px=12.0: (near(rng, kp, px), np.array([rng.normal(), rng.normal(), depth], F))

    # 0: BK (7-character basename, 19 joints), one person: a single valid depth id, no pair
    kp = skeleton(rng, (200, 250))
    images.append(('0000001.jpg', [person(annot19(rng, kp, BK_TO_14), 2, 0)], [pred(kp, 3.0)], False, False))

    # 1: OCHuman (19 joints), two people of equal id at depths 0 and float32(0.2): |dist| == thr is NOT < thr
    k0, k1 = skeleton(rng, (200, 250)), skeleton(rng, (450, 250))
    images.append(('och_000001.jpg', [person(annot19(rng, k0, OCH_TO_14), 1, 1), person(annot19(rng, k1, OCH_TO_14), 1, 3)],
                   [pred(k1, THR), pred(k0, 0.0)], False, False))

    # 2: five matched people at depths 0, thr, thr + 1 ulp, thr - 1 ulp, 1.5 with ids that make every kind of pair; one of them
    #    with coinciding visible joints (scale 0; the prediction hits one of them exactly: 0 / 0); a person nobody predicted;
    #    a prediction far away from everybody
    ks = [skeleton(rng, (400 + 260 * k, 300 + 90 * (k % 2))) for k in range(5)]
    depths = [F(0.0), THR, np.nextafter(THR, F(1)), np.nextafter(THR, F(0)), F(1.5)]
    ids, ages = [0, 1, 1, 0, -1], [0, 1, 2, -1, 3]
    flags = np.zeros(J); flags[[2, 6, 9]] = 1
    kc = skeleton(rng, (150, 150)); kc[[2, 6, 9]] = F((150.0, 170.0))
    people = [person(annot14(k), i, a) for k, i, a in zip(ks, ids, ages)]
    people[3] = person(annot14(kc, flags), ids[3], ages[3]); ks[3] = kc
    people.append(person(annot14(skeleton(rng, (900, 900))), 2, 2))                      # missed
    preds = [pred(k, d) for k, d in zip(ks, depths)]
    preds[3][0][6] = kc[6]
    preds.append(pred(skeleton(rng, (3000, 3000)), 9.0))                                  # false positive
    images.append(('img_five.jpg', people, [preds[k] for k in (4, 0, 5, 2, 1, 3)], False, True))

    # 3: twelve matched people with ids (66 pairs), every age; one with a single valid joint (PCKh -1),
    #    one with valid joints at x == -1 and x < -1 (valid for matching, not visible for PCKh), one entry without 'kp2d'
    centres = [(150, 150), (80, 700)] + [(420 + 230 * (k % 5), 200 + 330 * (k // 5)) for k in range(10)]
    ks = [skeleton(rng, c) for c in centres]
    one = np.zeros(J); one[3] = 1
    ks[0][3] = F((190.0, 230.0))                                                          # (far corner: the box from (-2, -2) covers the person)
    ks[1][4] = F((-1.0, 650.0)); ks[1][8] = F((-5.0, 720.0))
    ids = [1, 0, 2, 4, 3, 0, 1, 2, 2, 5, 0, 3]
    ages = [0, 1, 2, 3, -1, 0, 1, 2, 3, 0, 0, 1]
    people = [person(annot14(k, one if n == 0 else None), i, a) for n, (k, i, a) in enumerate(zip(ks, ids, ages))]
    people.insert(5, person(None, 1, 0))
    order = rng.permutation(12)
    images.append(('img_twelve.jpg', people, [pred(ks[k], rng.uniform(1.0, 3.0)) for k in order], False, False))

    # 4: the cap, 64 matched people, 2016 pairs; results stored as stacked arrays
    ks = [skeleton(rng, (150 + 210 * (k % 8), 200 + 330 * (k // 8))) for k in range(64)]
    people = [person(annot14(k), int(rng.integers(0, 6)), int(rng.integers(-1, 4))) for k in ks]
    order = rng.permutation(64)
    images.append(('img_64.jpg', people, [pred(ks[k], rng.uniform(1.0, 4.0)) for k in order], True, False))

    # 5: absent from the results: three misses of ages 0, 3, -1
    images.append(('img_absent.jpg', [person(annot14(skeleton(rng, (300 + 300 * k, 400))), k, a) for k, a in enumerate((0, 3, -1))],
                   None, False, False))

    # 6: three matched people without depth ids
    ks = [skeleton(rng, (300 + 300 * k, 400)) for k in range(3)]
    images.append(('img_noids.jpg', [person(annot14(k), -1, a) for k, a in zip(ks, (0, 1, 2))], [pred(k, 2.0 + k0) for k0, k in enumerate(ks)],
                   False, False))
    return images


def write_files(images, folder):
    annots, results = {}, {}
    for name, people, preds, stacked, as_list in images:
        entries = []
        for p in people:
            e = {'bbox': [0, 0, 1, 1], 'depth_id': p['depth_id'], 'age': p['age']}
            if p['kp'] is None:
                e['kp2d'] = None
            else:
                e['kp2d'] = [float(v) for v in p['kp'].reshape(-1)] if as_list else p['kp']
            entries.append(e)
        annots[name] = entries
        if preds is not None:
            if stacked:
                results[name] = {'kp2ds': np.stack([k for k, _ in preds]), 'trans': np.stack([t for _, t in preds])}
            else:
                results[name] = [{'kp2ds': k, 'trans': t} for k, t in preds]
    np.savez(os.path.join(folder, 'test_annots.npz'), annots=annots)
    np.savez(os.path.join(folder, 'results.npz'), results=results)
    return os.path.join(folder, 'results.npz')


def to14(kp, name):
    """The 14 ground-truth joints (x, y) the reference scores, -2 where invalid or unmapped (for the gap check only)."""
    a = kp.astype(np.float64).copy()
    a[a[:, 2] == 0] = -2.0
    if len(a) == 19:
        m = np.asarray(BK_TO_14 if len(name.replace('.jpg', '')) == 7 else OCH_TO_14)
        a = a[m]
        a[m == -1] = -2.0
    return a[:, :2].astype(F)


def ratio_gap(images, ev):
    """The smallest relative distance of err / scale from the threshold over every matched person's visible joints."""
    gap = np.inf
    for name, people, preds, _, _ in images:
        for p, g in ev.match_results.get(name, []):
            real, est = to14(people[g]['kp'], name), preds[p][0]
            vis = (real > -1).all(-1)
            if vis.sum() < 2:
                continue
            r = real[vis]
            scale = np.sqrt(float(r[:, 0].max() - r[:, 0].min()) ** 2 + float(r[:, 1].max() - r[:, 1].min()) ** 2)
            err = np.linalg.norm(real[vis].astype(np.float64) - est[vis].astype(np.float64), axis=-1)
            with np.errstate(all='ignore'):
                q = err / scale
            q = q[np.isfinite(q)]
            if len(q):
                gap = min(gap, float(np.abs(q - PCK_THRESH).min() / PCK_THRESH))
    return gap


def load_reference():
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    sys.path.insert(0, os.path.join(REFERENCE, 'simple_romp', 'evaluation'))
    import RH_evaluation.evaluation as ev
    return ev


def write_npz(path, arrays):
    """np.savez_compressed with sorted names and a fixed timestamp: the same bytes on every run."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name], order='C'), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def run_reference(ref, images):
    """RH_Evaluation on the scene -> the evaluation object, what get_results and compute_prf1 saw and returned, stdout."""
    seen = {}
    get_results, compute_prf1 = ref.get_results, ref.compute_prf1

    def spy_results(depth_relative, missed_age_ids, *a, **k):
        seen['dr'] = {key: [t.clone() for t in v] for key, v in depth_relative.items()}
        seen['missed_age'] = missed_age_ids.clone()
        seen['eval'] = get_results(depth_relative, missed_age_ids, *a, **k)
        return seen['eval']

    def spy_prf1(*a):
        seen['prf1'] = compute_prf1(*a)
        return seen['prf1']

    def on_alarm(*_):
        raise SystemExit('the reference did not terminate within %d s: its matcher spins once every pair is consumed' % ALARM_S)

    ref.get_results, ref.compute_prf1 = spy_results, spy_prf1
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(ALARM_S)
    out = io.StringIO()
    try:
        with tempfile.TemporaryDirectory() as folder, contextlib.redirect_stdout(out):
            ev = ref.RH_Evaluation(write_files(images, folder), folder, set_name='test')
            with open(ev.results_txt_save_path) as f:
                seen['txt'] = f.read().splitlines()
    finally:
        signal.alarm(0)
        torch.Tensor.cuda = cuda
        ref.get_results, ref.compute_prf1 = get_results, compute_prf1
    return ev, seen, out.getvalue()


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    ref = load_reference()
    for seed in range(200):
        images = scene(np.random.default_rng(seed))
        ev, seen, text = run_reference(ref, images)
        gap = ratio_gap(images, ev)
        if gap >= MIN_GAP:
            break
    else:
        raise SystemExit('no seed keeps every err / scale %g away from %g' % (MIN_GAP, PCK_THRESH))
    assert gap >= MIN_GAP
    matched = [len(ev.match_results.get(name, [])) for name, *_ in images]
    assert matched == [1, 2, 5, 12, 64, 0, 3], matched                       # the images hold what they were made for
    assert ev.pr['falsePositive'] == [0, 0, 1, 0, 0, 0, 0] and ev.pr['miss'] == [0, 0, 1, 0, 0, 3, 0], ev.pr

    B = len(images)
    out = {'seed': np.int64(seed), 'min_gap': np.float64(gap)}
    names = np.zeros((B, 24), np.uint8)
    for b, (name, *_) in enumerate(images):
        names[b, :len(name)] = np.frombuffer(name.encode('ascii'), np.uint8)
    out['names'] = names
    rows = [(b, p) for b, (_, people, *_) in enumerate(images) for p in people]
    kp = np.zeros((len(rows), 19, 3), F)
    for r, (_, p) in enumerate(rows):
        if p['kp'] is not None:
            kp[r, :len(p['kp'])] = p['kp']
    out.update(ann_image=np.array([b for b, _ in rows], np.int32), ann_kp=kp,
               ann_joints=np.array([0 if p['kp'] is None else len(p['kp']) for _, p in rows], np.int32),
               ann_depth_id=np.array([p['depth_id'] for _, p in rows], np.int32), ann_age=np.array([p['age'] for _, p in rows], np.int32),
               ann_as_list=np.array([b for b, im in enumerate(images) if im[4]], np.int32),
               res_stacked=np.array([b for b, im in enumerate(images) if im[3]], np.int32))
    preds = [(b, k, t) for b, (_, _, ps, *_) in enumerate(images) if ps is not None for k, t in ps]
    out.update(res_image=np.array([b for b, _, _ in preds], np.int32), res_kp=np.stack([k for _, k, _ in preds]).astype(F),
               res_trans=np.stack([t for _, _, t in preds]).astype(F))

    it = iter(zip(ev.pr['all'], ev.pr['falsePositive'], ev.pr['miss']))        # appended image by image, annotation order
    pr = np.array([next(it) for _ in images], np.int64)
    out.update(pr_all=pr[:, 0], pr_fp=pr[:, 1], pr_miss=pr[:, 2], prf1=np.array(seen['prf1'], np.float64))
    scored = [name for name, m in ev.match_results.items() if len(m)]
    assert len(scored) == len(ev.mPCKh)
    for b, (name, *_) in enumerate(images):
        if name in ev.match_results:
            out[f'match_{b}'] = np.asarray(ev.match_results[name], np.int64).reshape(-1, 2)
            out[f'pckh_{b}'] = ev.mPCKh[scored.index(name)].numpy().astype(F)
        out[f'missed_{b}'] = np.asarray(ev.missed_ids.get(name, []), np.int64).reshape(-1)
    cat = lambda xs, shape, dt: (torch.cat(xs, 0).numpy() if xs else np.zeros(shape)).astype(dt)
    for k in ('eq', 'cd', 'fd'):
        out[k + '_dist'] = cat(seen['dr'][k], (0,), F)
        out[k + '_age'] = cat(seen['dr'][k + '_age'], (0, 2), np.int64)
    assert all(torch.cat(seen['dr'][k], 0).dtype == torch.float32 for k in ('eq', 'cd', 'fd'))
    out['missed_age'] = seen['missed_age'].numpy().astype(np.int64)
    res = {k: float(v) for k, v in seen['eval'].items()}
    assert all(v.dtype == torch.float32 for v in seen['eval'].values())
    out['PCRD'] = F(res['PCRD_0.2'])
    out['PCRD_age'] = np.array([res.get('PCRD_0.2_' + a, np.nan) for a in ref.relative_age_types], F)
    out['mPCKh'] = F(torch.cat(ev.mPCKh).mean().item())
    txt = dict(line.split(': ') for line in seen['txt'])
    out['printed'] = np.array([float(txt['mPCKh_0.6']), float(txt['PCRD_0.2'])] +
                              [float(txt.get('PCRD_0.2_' + a, 'nan')) for a in ref.relative_age_types], np.float64)
    m = re.search(r'Equal ([\d.]+) close ([\d.]+) far ([\d.]+)', text)
    out['printed_eq_cd_fd'] = np.array([float(x) for x in m.groups()], np.float64)
    write_npz(OUT, out)
    print(text)
    print('\n'.join(seen['txt']))
    print('wrote', OUT, os.path.getsize(OUT), 'bytes, seed', seed, 'min gap %.2e' % gap, 'matched', matched)


if __name__ == '__main__':
    main()
