"""CPU: tests/attack_loop_ref.py (the numpy restatement of the NeRFail-S epoch bookkeeping) against fixture g24, the
reference's own run of the AS:278-431 loop shape (tests/golden/make_golden_attack_loop.py)."""
import inspect

import numpy as np
import pytest

import attack_loop_ref as R

TAGS = ('untargeted', 'targeted', 'beta')


def _run(g, tag):
    i = list(g['tags']).index(tag)
    return i, bool(g['targeted'][i]), float(g['beta'][i]), int(g['label'][i])


def test_fixture_has_what_the_issue_asks_for(golden):
    g = golden('g24_attack_loop')
    P, H, W, C, epochs = [int(v) for v in g['shape']]
    assert (P, H, W, C, epochs) == (3, 32, 32, 8, 5)
    assert g['train_batches'].tolist() == [4, 2] and g['export_batches'].tolist() == [4, 4]
    assert sorted(g['tags']) == sorted(TAGS) and g['beta'].tolist() == [0., 0., 0.25] and g['targeted'].tolist() == [0, 1, 0]
    worse, gaps = False, []
    for tag in TAGS:
        _, targeted, _, _ = _run(g, tag)
        acc, best = g[tag + '_stats_f32'][:epochs - 1, 3], (0 if targeted else 10000)
        for v in acc:
            worse |= bool(v < best) if targeted else bool(v > best)
            if (v >= best) if targeted else (v <= best):
                best = v
        rows = np.concatenate([g['%s_%s' % (tag, k)].reshape(-1, C) for k in ('train_ori_cla', 'train_cla', 'export_ori_cla', 'export_cla')])
        top = np.sort(rows.astype(np.float64), 1)
        gaps.append((top[:, -1] - top[:, -2]).min() / np.abs(rows).max())
        assert g[tag + '_iterates_rgb_int8'].shape == ((epochs - 1) * 2, P, H, W, 3)
    assert worse                       # (a) some epoch strictly worse than the best so far: best != last
    assert min(gaps) >= 1e-3           # (b) no argmax rests on rounding
    assert not np.array_equal(g['beta_best'], g['beta_last'])


@pytest.mark.parametrize('tag', TAGS)
def test_restated_statistics_and_rule_match_the_reference(golden, tag):
    g = golden('g24_attack_loop')
    epochs = int(g['shape'][4])
    _, targeted, beta, label = _run(g, tag)
    best = R.best_init(targeted)
    s32, s64 = g[tag + '_stats_f32'], g[tag + '_stats_f64']
    best_epoch = -1
    for e in range(epochs):
        export = e == epochs - 1
        cla = g[tag + '_export_cla'] if export else g[tag + '_train_cla'][e]
        ori_cla = g[tag + '_export_ori_cla'] if export else g[tag + '_train_ori_cla'][e]
        sizes = g['export_batches'] if export else g['train_batches']
        row, v0 = np.zeros(R.ROW, np.float32), 0
        for B in sizes:                                         # batch by batch, as the loop accumulates
            row = R.add_to_row(row, stats=R.logit_stats(cla[v0:v0 + B], ori_cla[v0:v0 + B], label))
            if export:
                row = R.add_to_row(row, sqerr=R.img_sqerr(g[tag + '_export_x_rgba'][v0:v0 + B], g['ori'][v0:v0 + B]))
            v0 += B
        if not export:
            row[9] = 1.                                         # (the attack epochs' x_rgba is not stored: image loss not restated there)
        rec, best, take = R.epoch_close(row, best, e, targeted)
        assert int(rec[11]) == int(s32[e, 7]) and int(rec[12]) == int(s32[e, 8]) and int(rec[5]) == int(s32[e, 6])     # counts: exact
        assert rec[1] == np.float32(s32[e, 1]) and rec[3] == np.float32(s32[e, 3])                                 # accuracies: exact
        for col, (i32, i64) in ((0, (0, 0)), (2, (2, 1))) + (((4, (4, 2)),) if export else ()):
            ref32, ref64 = s32[e, i32], s64[e, i64]
            assert abs(float(rec[col]) - ref64) <= 1e-7 * abs(ref64) + 1e-12, (tag, e, col)                        # float64 sums, one rounding
            assert abs(float(rec[col]) - ref32) <= 2 * abs(ref32 - ref64) + 1e-6 * abs(ref32), (tag, e, col)       # the issue's bound
        assert int(take) == int(g[tag + '_taken'][e]), (tag, e)
        if not export:
            best_epoch = int(best[2])
    assert best_epoch == int(g[tag + '_best_epoch'])
    it = g[tag + '_iterates_rgb_int8'].astype(np.float32)
    want = it[2 * best_epoch + 1]                              # the iterate after the best epoch's last batch
    assert np.array_equal(g[tag + '_best'][..., :3], want) and np.array_equal(g[tag + '_last'][..., :3], it[-1])


def test_argmax_ce_and_rounding_rules():
    z = np.array([[1., 3., 3., 0.], [np.nan, 9., 0., 0.], [0., 0., 0., 0.]], np.float32)
    assert R.correct_rows(z, 1).tolist() == [True, False, False] and R.correct_rows(z, 2).tolist() == [False, False, False]
    assert R.correct_rows(z, 0).tolist() == [False, False, True]
    ce = R.ce_rows(z, 1)
    assert np.isnan(ce[1]) and abs(ce[2] - np.log(4.)) < 1e-15 and abs(ce[0] - np.log(2 + np.exp(-2.) + np.exp(-3.))) < 1e-15
    x = np.array([0.5, 1.5, 2.5, 253.5, 254.5, -3., 255.5, 300., np.nan, 17.49, 17.51], np.float32)
    assert R.export_u8(x).tolist() == [0, 2, 2, 254, 254, 0, 255, 255, 0, 17, 18]
    rec, best, take = R.epoch_close(np.zeros(R.ROW, np.float32), R.best_init(False), 0, False)
    assert not take and np.isnan(rec[3]) and best[2] == -1                                     # an epoch without views is never taken


def test_public_interface():
    from nerfail_amd import attack, _lib
    p = inspect.signature(attack.nerfail_s).parameters
    assert list(p) == ['net', 'spatial', 'batches', 'label', 'epochs', 'a', 'epsilon', 'targeted', 'beta', 'export_batches',
                       'on_export', 'log', 'group']
    assert (p['a'].default, p['epsilon'].default, p['targeted'].default, p['beta'].default) == (2., 32., False, 0.)
    assert _lib.ABI_REVISION == 15 and _lib.load().nerfail_abi_revision() == 15 and _lib.ATTACK_ROW_FLOATS == R.ROW
    lib = _lib.load()
    assert lib.nerfail_attack_logit_stats(None, None, 2, 33, 0, None, None) == 1 and b'1..32' in lib.nerfail_last_error()
    assert lib.nerfail_attack_logit_stats(None, None, 2, 8, 8, None, None) == 1 and b'label' in lib.nerfail_last_error()
    assert lib.nerfail_attack_logit_stats(None, None, 2, 8, 0, None, None) == 1 and b'NULL' in lib.nerfail_last_error()
    assert lib.nerfail_img_sqerr(None, None, 1, 4, 0, None, None, None) == 1 and lib.nerfail_img_sqerr(None, None, 0, 4, 0, None, None, None) == 0
    assert lib.nerfail_copy_if(None, None, None, 4, None) == 1 and lib.nerfail_export_u8(None, 4, None, None) == 1
    assert lib.nerfail_attack_epoch_close(None, None, 0, 0, None, None, None) == 1
    assert lib.nerfail_img_sqerr_scratch_bytes() == 2048 * 8
