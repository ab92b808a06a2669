"""The crowd-merge edge cases (tests/crowd_cases.py) are what they say, on the CPU: every builder asserts its stated property from
the restatement while it builds; the float64 twin agrees with the float32 restatement on all finite rows at the tolerances of
tests/test_bev_crowd.py; and the restatement reproduces, stage by stage, the row sets that the reference's own stage functions
left on the crafted cases (tests/golden/bev_crowd_edges.npz, scripts/make_golden_bev_crowd_edges.py) -- which ties the tie rule,
the strict bounds, the 2 / 3 thresholds and the non-finite behaviour to the reference rather than to a reading of it.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crowd_cases as CC  # noqa: E402

STAGES = ('excluded', 'crop_suppressed', 'crop_outliers', 'suppressed', 'outliers')


def _removed_rows(res, stage):
    return {(r[0] if isinstance(r, tuple) else r) for r in res['removed'][stage]}


@pytest.mark.parametrize('name', sorted(CC.BUILDERS))
def test_builder_property_and_twin(name):
    for case in CC.cases(name):                                        # (the builder asserted its property while building)
        print(CC.describe(case))
        res, cid = case['res'], case['crop_id']
        assert case['prop'] and len(case['offsets']) == case['K'] + 1 and res['keep'].shape == (case['N'],)
        if name in CC.CRAFTED:
            assert res['margin_computed'] >= 1e-3                      # crafted: nothing is skipped
        else:
            assert res['margin'] > 1e-5 and case['seed'] < 20
        for s in STAGES:                                               # the stage counts are the removed rows
            assert len(_removed_rows(res, s)) == res['stages'][s]
        gone = set().union(*[_removed_rows(res, s) for s in STAGES])
        assert set(np.nonzero(~res['keep'])[0].tolist()) == gone | set(np.nonzero(cid < 0)[0].tolist())
        for r, a, b, pa, pb, m in res['removed']['crop_suppressed'] + res['removed']['suppressed']:
            assert r in (a, b) and a < b and pa < pb < m               # a pair removes one of its own, in row order
        cf, tr, pj = CC.twin_of(case)
        fin = (cid >= 0) & np.isfinite(cf).all(1) & np.isfinite(tr).all(1) & np.isfinite(pj).all((1, 2))
        assert fin.sum() >= case['N'] - (cid < 0).sum() - 1            # (at most the one non-finite row drops out)
        np.testing.assert_allclose(res['cam_full'][fin], cf[fin], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(res['cam_trans'][fin], tr[fin], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(res['pj2d_org'][fin], pj[fin], rtol=0, atol=2e-3)
        bad = (cid >= 0) & ~fin                                        # the non-finite row: non-finite in the same places
        for a, b in ((res['cam_full'], cf), (res['cam_trans'], tr), (res['pj2d_org'], pj)):
            assert np.array_equal(np.isnan(a[bad]), np.isnan(b[bad])) and np.array_equal(np.isinf(a[bad]), np.isinf(b[bad]))


def test_case_names_unique_and_small():
    names = [c['name'] for n in CC.CRAFTED for c in CC.cases(n)]
    assert len(names) == len(set(names)) and all(c['N'] <= 40 for n in CC.CRAFTED for c in CC.cases(n))
    assert set(CC.FIXTURE) <= set(CC.CRAFTED) and set(CC.BUILDERS) >= {
        'seam64', 'seam65', 'seam129', 'plan71', 'big_crop', 'one_crop_1000', 'global_stride', 'counts', 'ties', 'bounds',
        'geometry', 'offsets', 'nonfinite'}


def test_restatement_matches_reference_stage_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, 'bev_crowd_edges.npz'))
    built = {c['name']: c for n in CC.FIXTURE for c in CC.cases(n)}
    assert sorted(g['names'].tolist()) == sorted(built)
    raised = [n for n in built if n + '/raised' in g.files]
    assert raised == []                                                # the reference's stage functions took every case
    for n, case in built.items():
        for k in ('cam', 'conf', 'crop_id', 'crops'):                  # the fixture was made from these very inputs
            assert np.array_equal(g['%s/%s' % (n, k)], case[k], equal_nan=True), (n, k)
        assert g[n + '/joints_sum'] == np.where(np.isfinite(case['joints']), case['joints'], 0).astype(np.float64).sum()
        res = case['res']
        alive = set(np.nonzero(case['crop_id'] >= 0)[0].tolist())
        for s in STAGES:
            alive -= _removed_rows(res, s)
            assert sorted(alive) == g['%s/alive_%s' % (n, s)].tolist(), (n, s)
        kept = np.nonzero(res['keep'])[0]
        assert sorted(alive) == kept.tolist()
        np.testing.assert_allclose(res['cam_full'][kept], g[n + '/cam_full'], rtol=1e-6, atol=1e-7, err_msg=n)
        np.testing.assert_allclose(res['cam_trans'][kept], g[n + '/cam_trans'], rtol=1e-6, atol=1e-6, err_msg=n)
        # (a row with one non-finite coordinate: the reference multiplies by the 3 x 3 intrinsic matrix, whose zeros turn the
        # row's other coordinate into NaN too; the restatement and the device project coordinate by coordinate.  Finite rows only.)
        fin = np.isfinite(g[n + '/pj2d_org']).all((1, 2))
        assert not np.isfinite(res['pj2d_org'][kept][~fin]).all((1, 2)).any(), n
        np.testing.assert_allclose(res['pj2d_org'][kept][fin], g[n + '/pj2d_org'][fin], rtol=0, atol=2e-3, err_msg=n)


def test_fixture_pins_the_rules(golden_dir):
    """The rules DESIGN.md states, read off the reference's own row sets."""
    g = np.load(os.path.join(golden_dir, 'bev_crowd_edges.npz'))
    case = {c['name']: c for n in CC.FIXTURE for c in CC.cases(n)}
    final = lambda n: set(g[n + '/alive_outliers'].tolist())
    t = case['ties_duplicates']['tags']                                # equal conf: the later row goes; else the lower conf
    assert final('ties_duplicates') == {t['a0'], t['b1'], t['a2']}
    t = case['ties_global']['tags']
    assert final('ties_global') == {t['a0'], t['b1'], t['a2']}
    t = case['ties_chain']['tags']                                     # the removal is an OR over pairs
    assert final('ties_chain') == {t['C'], t['bystander']}
    t = case['ties_excluded']['tags']                                  # an excluded row suppresses nobody
    assert final('ties_excluded') == {t['in'], t['bystander']}
    t = case['bounds_k9']['tags']                                      # strict bounds; crops 0 and 1 have no lower bound
    kept = set(g['bounds_k9/alive_excluded'].tolist())
    K = case['bounds_k9']['K']
    for tag, row in t.items():
        assert (row in kept) == (not tag.endswith(('hi+', 'lo-'))), tag
    assert {'0hi', '1hi', '2hi', '2lo', '%dlo' % (K - 1)} <= set(t) and '1lo' not in t and '%dhi' % (K - 1) not in t
    t = case['bounds_k2']['tags']
    assert set(g['bounds_k2/alive_excluded'].tolist()) == {t['m0'], t['p1'], t['m1']}
    assert len(g['bounds_k1/alive_excluded']) == 2
    for n in (2, 3):                                                   # the outlier passes start at 3 rows
        for kind, stage in (('crop', 'crop_outliers'), ('crop_outlier', 'crop_outliers'), ('global', 'outliers'),
                            ('global_outlier', 'outliers')):
            name = 'counts_%s_%d' % (kind, n)
            far = case[name]['tags']['far']
            assert (far in g['%s/alive_%s' % (name, stage)].tolist()) == (n == 2), name
    for name, gone in (('between', True), ('below', True), ('above', False), ('global_between', False), ('global_below', True)):
        far = case['counts_scale_' + name]['tags']['far']
        assert (far in final('counts_scale_' + name)) == (not gone)
    for name in g['names'].tolist():                                   # one NaN translation switches the outlier pass off
        if name.startswith(('nonfinite_cam0_nan', 'nonfinite_cam2_nan')):
            assert g[name + '/alive_crop_outliers'].tolist() == g[name + '/alive_crop_suppressed'].tolist()
            assert case[name]['tags']['far'] in final(name)
