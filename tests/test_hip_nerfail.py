"""-m gpu: deepfool.deepfool_native and attack.nerfail, the NeRFail product loop, against fixture g27 - the reference's gauss_net
and deepfool.deepfool driven through the AN:269-505 loop shape (tests/golden/make_golden_nerfail.py).

Every discrete decision must equal the fixture's: skip or attack per visit, iter_k, the chosen class of every iteration (the
native path reports them; the mirror deepfool.deepfool does not), the m1 / m2 history, the epochs, the taken passes, the best
record. Tables and export images must lie within 2 x the fixture's float32-vs-float64 distance of the float64 run (the project's
standing convention for g7, g21 and g26), over a floor for entries where the two reference runs happen to agree exactly:

    floor = 8 * 2^-24 * max|table| * (1 + DeepFool iterations accumulated so far)

- a table entry is a sum of one float32 term per DeepFool iteration (rot += scale * (G_k - G_o), each term rounded once, the
sum rounded once: 2 roundings of relative size 2^-24 per iteration on values no larger than the table's maximum; the factor 8
covers the rounding of scale and of the gradient rows themselves, a handful of float32 operations each). The fixture stores the
float64 run rounded to float32, which the same floor covers."""
import numpy as np
import pytest
import torch

import nerfail_problem as NP
from hiputil import N, dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g():
    return NP.load()


@pytest.fixture(scope='module')
def runs(g):
    """Every g27 run once per DeepFool path, with the table after every pass and the export pass's float images."""
    from nerfail_amd import attack
    from nerfail_amd.GaussNet import gauss_net
    out = {}
    orig_done, orig_export = attack._pass_done, gauss_net.export_forward
    for tag in NP.TAGS:
        for native in (None, False):
            tables, exported, lines = [], [], []

            def spy_export(self, *a, exported=exported, **k):
                r = orig_export(self, *a, **k)
                exported.append((N(r[0]), N(r[1])))
                return r
            attack._pass_done = lambda i, t, tables=tables: tables.append(N(t))
            gauss_net.export_forward = spy_export
            try:
                res, env = NP.run(g, tag, dev(), native=native, on_export=lambda *a: None, log=lines.append)
            finally:
                attack._pass_done, gauss_net.export_forward = orig_done, orig_export
            out[tag, native] = (res, tables, exported, lines)
    return out


CASES = [(t, n) for t in NP.TAGS for n in (None, False)]


@pytest.mark.parametrize('tag,native', CASES)
def test_every_discrete_decision_matches_the_reference(g, runs, tag, native):
    res = runs[tag, native][0]
    run = g['runs'][tag]
    P, H, W, C, epochs, n_views, n_export, cap = NP.shape(g)
    assert len(res.stats) == len(run['passes'])
    for p, (d, r) in enumerate(zip(res.stats, run['passes'])):
        got = (d['epoch'], d['next_epoch'], d['m1_pass'], d['m1'], d['m2'], d['views'], d['taken'], d['m2_raises'], d['test_correct'], d['attack_correct'])
        want = tuple(int(r[c]) for c in (NP.EPOCH, NP.NEXT_EPOCH, NP.M1_PASS, NP.M1, NP.M2, NP.VIEWS, NP.TAKEN, NP.RAISES, NP.TEST_CORRECT, NP.ATTACK_CORRECT))
        assert got == want, (tag, native, p, got, want)
        assert d['test_acc'] == r[NP.TEST_ACC] and d['attack_acc'] == r[NP.ATTACK_ACC]
        visits = run['visits'][p]
        if d['epoch'] == epochs - 1:
            assert d['visits'] == [] and d['views'] == n_export
            continue
        order = NP.pass_views(g, tag, p)                                   # the views of the pass, in the loader's order
        assert len(d['visits']) == len(order)
        for (i, skipped, iter_k, classes), v in zip(d['visits'], order):
            assert (int(skipped), iter_k) == (int(visits[v, 0]), int(visits[v, 1])), (tag, native, p, v)
            if native is None and not skipped:
                assert classes == [int(c) for c in visits[v, 2:2 + iter_k]], (tag, p, v, classes)
        assert d['skipped'] == int((visits[order, 0] == 1).sum()) and d['attacked'] == int((visits[order, 0] == 0).sum())
        assert d['completed'] == int(((visits[order, 0] == 0) & (visits[order, 1] < cap)).sum())
        assert d['deepfool_iters'] == int(visits[order, 1].sum())
    assert (res.m1_best, res.m2_best) == (int(run['m1_best']), int(run['m2_best'])) and res.best_acc == float(run['best_acc'])
    assert len(res.need_to_log_dict) >= 1 and all(k.startswith('m1-') for k in res.need_to_log_dict)


@pytest.mark.parametrize('tag,native', CASES)
def test_tables_and_export_within_the_reference_spread(g, runs, tag, native):
    res, tables, exported, _ = runs[tag, native]
    run = g['runs'][tag]
    s0 = g['s0']
    assert len(tables) == len(run['tables_rgb'])
    iters = np.cumsum([d['deepfool_iters'] for d in res.stats])
    worst = 0.

    def held(mine, ref_rgb, dist, n_iter, what):
        floor = 8 * 2.0 ** -24 * max(float(np.abs(ref_rgb).max()), 1.0) * (1 + n_iter)
        err = float(np.abs(mine[..., :3].astype(np.float64) - ref_rgb).max())
        assert np.array_equal(mine[..., 3], s0[..., 3]), what          # alpha untouched
        assert err <= 2 * float(dist) + floor, (tag, native, what, err, float(dist), floor)
        return err / (2 * float(dist) + floor)
    for p, t in enumerate(tables):
        worst = max(worst, held(t, run['tables_rgb'][p], run['tables_dist'][p], iters[p], 'table after pass %d' % p))
    worst = max(worst, held(N(res.best), run['best_rgb'], run['best_dist'], iters[-1], 'best'))
    n_export = NP.shape(g)[6]
    first = exported[:n_export]                                          # the first export pass: what the fixture stores
    x, xr = np.concatenate([e[0] for e in first]), np.concatenate([e[1] for e in first])
    for mine, key in ((x, 'export_x'), (xr, 'export_x_rgba')):
        floor = 8 * 2.0 ** -24 * max(float(np.abs(run[key]).max()), 1.0) * (1 + iters[int(run['export_pass'])])
        err = float(np.abs(mine.astype(np.float64) - run[key]).max())
        assert err <= 2 * float(run[key + '_dist']) + floor, (tag, native, key, err)
        worst = max(worst, err / (2 * float(run[key + '_dist']) + floor))
    print('g27 %s native=%s: worst error / bound %.3f over %d tables, best and export' % (tag, native, worst, len(tables)))


@pytest.mark.parametrize('tag', NP.TAGS)
def test_native_and_mirror_agree(g, runs, tag):
    """Both paths run the same kernels for the gradients and the same arithmetic for the step: the same tables, bit for bit."""
    a, b = runs[tag, None], runs[tag, False]
    assert len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    assert torch.equal(a[0].best, b[0].best) and torch.equal(a[0].last, b[0].last)


@pytest.mark.parametrize('tag', NP.TAGS)
def test_deepfool_native_equals_deepfool_on_the_first_attacked_view(g, tag):
    from nerfail_amd import deepfool as DF
    targeted, label, m1, m2, _ = NP.run_args(g, tag)
    P, H, W, C, epochs, n_views, n_export, cap = NP.shape(g)
    net, s0, items, _ = NP.setup(g, dev(), view_ids=False)
    visits = g['runs'][tag]['visits'][0]
    v = next(v for v in NP.pass_views(g, tag, 0) if visits[v, 0] == 0)
    kw = dict(num_classes=C, max_iter=cap, target_label=label if targeted else None, overshoot=float(g['overshoot']), m1=m1, m2=m2)
    a = DF.deepfool_native((s0, items[v][0], items[v][1]), None, net, **kw)
    b = DF.deepfool((s0, items[v][0], items[v][1]), None, net, **kw)
    assert len(a) == 6 and len(b) == 5
    assert a[1] == b[1] == int(visits[v, 1])                             # loop_i, and the reference's
    assert a[5] == [int(c) for c in visits[v, 2:2 + a[1]]]               # the chosen class of every iteration
    assert int(a[2]) == int(b[2]) and int(a[3]) == int(b[3])             # clean argmax, final (bumped) argmax
    assert torch.equal(a[0], b[0]) and torch.equal(a[4], b[4])
    # with the view named: the same result through the cached index
    c = DF.deepfool_native((s0, items[v][0], items[v][1]), None, net, view_ids=[('g27', v)], **kw)
    assert c[1] == a[1] and c[5] == a[5] and torch.equal(c[4], a[4])
    # what the native path does not cover falls through to the mirror
    net.deterministic = False                                            # (the atomics backward: not the native path's)
    d = DF.deepfool_native((s0, items[v][0], items[v][1]), None, net, **dict(kw, max_iter=1))
    assert len(d) == 6 and d[5] is None and d[1] == min(1, a[1])


def test_native_mycnn_two_views_native_equals_mirror():
    """The native MyCNN victim at the smallest input size tests/test_hip_cnn_multi.py uses, two views, df_max_iter = 3:
    native=None equals native=False in every discrete decision (and, the arithmetic being the same, in the table)."""
    import test_hip_cnn_multi as CM
    from nerfail_amd.attack import nerfail
    from nerfail_amd.GaussNet import gauss_net
    m = CM.native(21, 8)
    Hh, Ww = 766, 766
    rs = np.random.RandomState(3)
    Pn = 2
    s0 = np.zeros((Pn, 64, 64, 4), np.float32)
    s0[..., 3] = 255.0
    n_rows = Pn * 64 * 64
    res = {}
    for native in (None, False):
        net = gauss_net(dev(), 0.02, m, 'my_model', epsilon=None)
        items = []
        r2 = np.random.RandomState(4)
        for v in range(2):
            ori = np.zeros((1, Hh, Ww, 4), np.float32)
            ori[..., :3] = np.floor(r2.uniform(0, 255, size=(1, Hh, Ww, 3)))
            ori[..., 3] = 255.0
            w = r2.uniform(0.0, 0.25, size=(1, Hh, Ww, 8)).astype(np.float32)
            idx = r2.randint(0, n_rows, size=(1, Hh, Ww, 8)).astype(np.float32)
            wi = np.stack([w, idx], 1)
            items.append((torch.from_numpy(wi).to(dev()), torch.from_numpy(ori).to(dev()), ('mycnn', v)))
        with torch.no_grad():
            label = int(torch.argmax(net(torch.from_numpy(s0).to(dev()), items[0][0], items[0][1])[4][0]))
        # accumulate_incomplete: a pass in which no call finishes within df_max_iter still changes the table, so the m1 bisection of
        # AN:442-468 - which, as in the reference, alternates for ever when the m1 that failed keeps failing - never starts
        res[native] = nerfail(net, torch.from_numpy(s0).to(dev()), items, label, 2, m1=1, m2=100, df_max_iter=3, overshoot=1.0,
                              accumulate_incomplete=True, log=None, native=native)
    a, b = res[None], res[False]
    assert len(a.stats) == len(b.stats) == 2 and [d['epoch'] for d in a.stats] == [0, 1]
    keys = ('m1', 'm2', 'm1_pass', 'epoch', 'next_epoch', 'views', 'skipped', 'attacked', 'completed', 'deepfool_iters', 'm2_raises', 'taken',
            'test_correct', 'attack_correct')
    for da, db in zip(a.stats, b.stats):
        assert [da[k] for k in keys] == [db[k] for k in keys]
        assert [v[:3] for v in da['visits']] == [v[:3] for v in db['visits']]
    assert sum(d['attacked'] for d in a.stats) >= 1
    assert all(len(v[3]) == v[2] for d in a.stats for v in d['visits'])
    assert torch.equal(a.best, b.best) and (a.m1_best, a.m2_best, a.best_acc) == (b.m1_best, b.m2_best, b.best_acc)
