"""The numpy restatement of the IGSM-2D loop (tests/igsm2d_ref.py) against fixture g28, the reference's own run
(tests/golden/make_golden_igsm2d.py): every iterate, the taken flags and the best epoch exactly, the float64 statistics to
1e-12 relative. CPU only."""
import numpy as np
import pytest

import igsm2d_ref as IR


@pytest.fixture(scope='module')
def g(golden):
    return golden('g28_igsm2d')


@pytest.fixture(scope='module')
def runs(g):
    images = IR.g28_images(int(g['seed']), g['tints'])
    out = {}
    for i, tag in enumerate(g['tags']):
        out[str(tag)] = IR.run_loop(images, g['cls_w'], int(g['label'][i]), int(g['shape'][4]), float(g['a']), float(g['epsilon']),
                                    bool(g['targeted'][i]), int(g['shape'][5]))
    return out


@pytest.mark.parametrize('tag', ('untargeted', 'targeted'))
def test_iterates_flags_and_best_epoch_are_the_references(g, runs, tag):
    run, a = runs[tag], float(g['a'])
    sums = g[tag + '_sums']
    assert len(run['iterates']) == sums.shape[0] == 6                     # 3 attack epochs x (3 + 1 views)
    for k, table in enumerate(run['iterates']):
        assert np.array_equal(IR.checksums(table), sums[k]), (tag, k)
    assert np.array_equal(run['best'], g[tag + '_best'].astype(np.float32) * a)
    assert np.array_equal(run['last'], g[tag + '_last'].astype(np.float32) * a)
    assert not np.array_equal(run['best'], run['last'])                  # the fixture's point
    assert np.array_equal(run['taken'], g[tag + '_taken'])
    assert run['best_epoch'] == int(g[tag + '_best_epoch'])


@pytest.mark.parametrize('tag', ('untargeted', 'targeted'))
def test_logits_statistics_and_export_images(g, runs, tag):
    run = runs[tag]
    epochs = int(g['shape'][4])
    assert np.array_equal(run['cla'], g[tag + '_cla'])                    # float64 evaluation, rounded once: the same float32 logits
    for e in range(epochs):
        assert np.array_equal(run['ori_cla'], g[tag + '_ori_cla'][e])
    s32, s64 = g[tag + '_stats_f32'], g[tag + '_stats_f64']
    assert np.abs(run['stats_f64'] - s64).max() <= 1e-12 * np.abs(s64).max()
    assert (np.abs(run['stats_f64'] - s64) <= 1e-12 * np.abs(s64)).all()
    rec = run['records']
    assert np.array_equal(rec[:, 1], s32[:, 1].astype(np.float32)) and np.array_equal(rec[:, 3], s32[:, 3].astype(np.float32))
    assert np.array_equal(rec[:, 11], s32[:, 7]) and np.array_equal(rec[:, 12], s32[:, 8]) and np.array_equal(rec[:, 5], s32[:, 6])
    for col, i64 in ((0, 0), (2, 1), (4, 2)):                             # the records are the float64 means rounded once
        assert np.array_equal(rec[:, col], run['stats_f64'][:, i64].astype(np.float32)) or \
            np.abs(rec[:, col] - s64[:, i64]).max() <= 6e-8 * np.abs(s64[:, i64]).max()
    v = int(g['export_view'])
    assert np.array_equal(run['adv_u8'][v], g[tag + '_export_adv_u8']) and np.array_equal(run['mask_u8'][v], g[tag + '_export_mask_u8'])


def test_strict_rule_is_exercised(g):
    """Some attack epoch ties the best accuracy so far and is NOT taken."""
    hit = False
    for i, tag in enumerate(g['tags']):
        acc, taken = g[str(tag) + '_stats_f32'][:, 3], g[str(tag) + '_taken']
        best = 0. if g['targeted'][i] else 10000.
        for e in range(int(g['shape'][4]) - 1):
            if acc[e] == best:
                assert taken[e] == 0
                hit = True
            if taken[e]:
                best = acc[e]
    assert hit
