"""-m gpu: attack.uap_2d, the UAP-2D product loop. (a) against fixture g29 - the reference's universal_2D_net and deepfool.deepfool
driven through the UA:241-358 loop shape (tests/golden/make_golden_uap2d.py) - with the stand-in classifier at 224 x 224, through
deepfool_2d_native (autograd class gradients, nerfail_uap2d_step) and through the mirror deepfool_2d: every discrete decision equal
to the fixture's, losses within twice the fixture's own float32-to-float64 spread, tables, best and exported images within
uap2d_ref.g29_bound; (b) deepfool_2d_native against deepfool_2d on the first attacked view; (c) the native MyCNN victim at
766 x 766, the smallest size MyCNN accepts: native=None (ops.cnn_fwd + ONE ops.cnn_bwd_data_multi per iteration) against
native=False (the mirror, autograd through MyCNN): every decision and every record field equal except attack_loss, which is a
continuous function of tables that agree to the floor and not bit for bit, and `best` within that floor; (d) the ValueErrors and on_export's arrays.

As for g24 / g28 the stand-in classifier is evaluated in float64 and rounded once on both sides (order-independent logits)."""
import numpy as np
import pytest
import torch

import attack_loop_ref as R
import igsm2d_ref as IR
import uap2d_ref as UR
from hiputil import N, dev

pytestmark = pytest.mark.gpu
TAGS = ('untargeted', 'targeted')
PASS_KEYS = ('epoch', 'next_epoch', 'views', 'test_loss', 'test_acc', 'attack_loss', 'attack_acc', 'taken', 'test_correct', 'attack_correct')


@pytest.fixture(scope='module')
def g(golden):
    return golden('g29_uap2d')


@pytest.fixture(scope='module')
def images(g):
    return torch.from_numpy(UR.g29_images(int(g['seed']), g['tints'], g['extra_tints']))


@pytest.fixture(scope='module')
def cls(g):
    w = torch.from_numpy(g['cls_w']).to(dev())

    class Cls(torch.nn.Module):
        def forward(self, x):
            return (torch.nn.functional.adaptive_avg_pool2d(x.double(), 4).reshape(x.shape[0], -1) @ w.double().t()).float()
    return Cls()


def run_uap(model, model_name, images, native, **kw):
    """attack.uap_2d with the table of every pass, the exported arrays and the log lines recorded."""
    from nerfail_amd import attack
    tables, exported, lines = [], [], []
    orig = attack._uap2d_pass_done
    attack._uap2d_pass_done = lambda index, table: tables.append((index, N(table).copy()))
    try:
        res = attack.uap_2d(model, model_name, images, on_export=lambda *a: exported.append(a), log=lines.append, native=native, **kw)
    finally:
        attack._uap2d_pass_done = orig
    return res, tables, exported, lines


@pytest.fixture(scope='module')
def runs(g, images, cls):
    out = {}
    for i, tag in enumerate(TAGS):
        kw = UR.g29_args(g, i)
        for native in (None, False):
            out[tag, native] = run_uap(cls, 'vit_b_16', images, native, **kw)
    return out


def as_passes(stats):
    return np.array([[d[k] for k in PASS_KEYS] for d in stats], np.float64)


@pytest.mark.parametrize('native', (None, False), ids=('native', 'mirror'))
@pytest.mark.parametrize('tag', TAGS)
def test_decisions_tables_and_best_against_g29(g, runs, tag, native):
    res, tables, exported, lines = runs[tag, native]
    assert [i for i, _ in tables] == list(range(len(res.stats)))
    visits = [d['visits'] for d in res.stats]
    if native is None:
        assert all(c is not None for vs in visits for _, _, _, c in vs)    # the native path reports the chosen classes
    UR.g29_check(g, tag, as_passes(res.stats), visits, [t for _, t in tables], N(res.best), None)
    for d, vs in zip(res.stats, visits):
        att = [v for v in vs if not v[1]]
        assert (d['skipped'], d['attacked']) == (len(vs) - len(att), len(att))
        assert d['completed'] == sum(v[2] < int(g['shape'][5]) for v in att) and d['deepfool_iters'] == sum(v[2] for v in att)
    want_acc = float(g[tag + '_best_acc'])
    assert res.best_acc == want_acc
    assert res.last.data_ptr() == res.best.data_ptr() or np.array_equal(N(res.last), N(res.best))   # after the export pass
    assert lines[0] == 'Attack ...... [0/4]' and any(s.startswith('test Loss:') for s in lines) and 'iter_k < df_max_iter' in lines


@pytest.mark.parametrize('native', (None, False), ids=('native', 'mirror'))
@pytest.mark.parametrize('tag', TAGS)
def test_exported_images_against_g29(g, runs, images, tag, native):
    """Three uint8 arrays per exported view, what cv2.imwrite stores of the fixture's float images: equal wherever the float
    image is further from a rounding boundary than uap2d_ref.g29_bound, never more than one apart; negatives of the
    perturbation at 0."""
    res, _, exported, _ = runs[tag, native]
    views = [int(v) for v in g['export_views']]
    assert [(e[0], e[1]) for e in exported] == [(i, [v]) for i, v in enumerate(views)]
    iters = int(g[tag + '_iters_so_far'][-1])
    best = N(res.best)
    for j, (_, _, adv, mask, ori) in enumerate(exported):
        assert adv.dtype == mask.dtype == ori.dtype == np.uint8
        assert adv.shape == ori.shape == (1, 224, 224, 3) and mask.shape == (224, 224, 3)
        for got, name in ((adv[0], 'adv'), (mask, 'mask')):
            ref = g['%s_export_%s' % (tag, name)][j].astype(np.float64)
            bound = UR.g29_bound(ref, g['%s_export_%s_dist' % (tag, name)], iters)
            c = np.clip(ref, 0., 255.)
            safe = np.abs(c - np.floor(c) - .5) > bound
            want = R.export_u8(ref)
            assert np.array_equal(got[safe], want[safe]) and np.abs(got.astype(int) - want.astype(int)).max() <= 1, (tag, name)
        assert np.array_equal(ori[0], g[tag + '_export_ori'][j])
        assert (best < 0).any() and (mask[best < -.5] == 0).all()           # negative values become 0, as cv2.imwrite saturates
        assert np.array_equal(mask, R.export_u8(best)) and np.array_equal(ori[0], IR.white(N(images)[views[j]]).astype(np.uint8))


def test_deepfool_2d_native_equals_the_mirror_on_the_first_attacked_view(g, images, cls):
    from nerfail_amd import deepfool as DF
    from nerfail_amd.GaussNet import universal_2D_net
    net = universal_2D_net(dev(), 0.02, cls, 'vit_b_16')
    kw = UR.g29_args(g, 0)
    table = torch.zeros((224, 224, 3), device=dev())
    store = images.to(dev())
    view = int(g['untargeted_visits'][0, 0, 0])
    ori = torch.from_numpy(IR.white(N(images)[view])[None]).to(dev())
    args = dict(num_classes=kw['num_classes'], max_iter=kw['df_max_iter'], target_label=None, overshoot=kw['overshoot'], m1=kw['m1'], m2=kw['m2'])
    dr_n, k_n, o_n, arg_n, r_n, classes = DF.deepfool_2d_native((table, None), None, net, images=store, view=view, **args)
    dr_m, k_m, o_m, arg_m, r_m = DF.deepfool_2d((table, ori), None, net, **args)
    assert k_n == k_m == int(g['untargeted_visits'][0, 0, 2])
    assert int(o_n) == int(o_m) and int(arg_n) == int(arg_m)
    assert classes == g['untargeted_visits'][0, 0, 3:3 + k_n].tolist()
    assert torch.equal(dr_n, r_n - table) and torch.equal(dr_m, r_m - table)
    # a one-view store made of ori_img serves when no resident store is given; the sixth value says which path ran
    again = DF.deepfool_2d_native((table, ori), None, net, **args)
    assert again[1] == k_n and again[5] == classes and torch.equal(again[4], r_n)
    assert DF.deepfool_2d_native((table, ori), None, net, num_classes=9, max_iter=0)[5] is None       # 9 classes: the mirror
    one = DF.deepfool_2d_native((table, None), None, net, images=store[view:view + 1], **args)         # a one-view store: view 0
    assert one[1] == k_n and one[5] == classes and torch.equal(one[4], r_n)
    for bad in (dict(images=store), dict(images=store, view=len(store)), dict(images=store, view=-1), dict()):
        with pytest.raises(ValueError, match='deepfool_2d_native'):
            DF.deepfool_2d_native((table, None), None, net, **bad, **args)


# ------------------------------------------------------------------------------------------------------------ (c) native MyCNN
# MyCNN with its initial weights has gradient norms far below the 1e-4 of DF:85's denominator (as g27's stand-in has): with the
# reference's overshoot 0.02 no call completes within three iterations and the table never moves. These constants let calls
# complete, and epsilon is small enough for the +-epsilon clamp to act on what they add.
CNN_KW = dict(label=3, epochs=2, epsilon=4., m1=0, m2=1, targeted=False, df_max_iter=3, overshoot=50., num_classes=8)


@pytest.fixture(scope='module')
def cnn_runs():
    from nerfail_amd import ops
    from nerfail_amd.MyModel import MyCNN
    torch.manual_seed(7)
    model = MyCNN(num_classes=8).to(dev())
    rs = np.random.RandomState(7)
    images = rs.randint(0, 256, size=(2, 766, 766, 4)).astype(np.uint8)
    images[..., 3] = np.where(rs.uniform(size=(2, 766, 766)) < 0.7, 255, 0)
    images = torch.from_numpy(images).to(dev())
    out, calls = {}, []
    orig = ops.cnn_bwd_data_multi

    def spy(packed, ws, masks, d_logits, H, W):
        calls.append(tuple(d_logits.shape))
        return orig(packed, ws, masks, d_logits, H, W)
    for native in (None, False):
        ops.cnn_bwd_data_multi = spy
        try:
            out[native] = run_uap(model, 'my_model', images, native, **CNN_KW) + (list(calls),)
        finally:
            ops.cnn_bwd_data_multi = orig
        del calls[:]
    return out


def test_native_mycnn_equals_the_mirror_in_every_decision(cnn_runs):
    nat, mir = cnn_runs[None], cnn_runs[False]
    assert len(nat[0].stats) == len(mir[0].stats) == 2
    for a, b in zip(nat[0].stats, mir[0].stats):
        for k in a:
            if k == 'visits':
                assert [v[:3] for v in a[k]] == [v[:3] for v in b[k]], (a[k], b[k])
            elif k == 'attack_loss':
                # the one field left out of "equal": a continuous function of the table, and the two paths' tables agree to the
                # floor below, not bit for bit (their norms are summed in another order). Every other field is discrete or - like
                # test_loss, which comes from the clean logits alone - computed by the same launches on the same bits.
                print('attack_loss of epoch %d: native %.17g, mirror %.17g' % (a['epoch'], a[k], b[k]))
            else:
                assert a[k] == b[k], (k, a[k], b[k])
    assert nat[0].best_acc == mir[0].best_acc
    d = nat[0].stats[0]
    print('native MyCNN pass 0: %s' % {k: d[k] for k in d if k != 'visits'}, d['visits'])
    assert d['attacked'] >= 1 and d['completed'] >= 1                      # the table moved: the comparison below is not of zeros
    iters = d['deepfool_iters']
    ref = N(mir[0].best).astype(np.float64)
    err = np.abs(N(nat[0].best) - ref)
    floor = 8. * 2. ** -24 * np.maximum(np.abs(ref), 1.) * (1 + iters)
    print('native vs mirror best: worst error / floor %.3f, %d of %d elements differ' % ((err / floor).max(), (err > 0).sum(), err.size))
    assert np.abs(ref).max() > 0 and (err <= floor).all()
    assert np.abs(ref).max() <= CNN_KW['epsilon']


def test_native_mycnn_takes_its_class_gradients_from_one_backward(cnn_runs):
    nat_calls, mir_calls = cnn_runs[None][4], cnn_runs[False][4]
    iters = sum(d['deepfool_iters'] for d in cnn_runs[None][0].stats)
    assert len(nat_calls) == iters and set(nat_calls) == {(8, 1, 8)}       # [o] + 7 competitors, one view
    assert all(c[0] == 1 for c in mir_calls)                               # (the mirror differentiates row by row)


# ------------------------------------------------------------------------------------------------------------ (d) arguments
def test_value_errors(images, cls):
    from nerfail_amd import attack
    small = images[:1, :8, :8].contiguous()
    with pytest.raises(ValueError, match='epochs'):
        attack.uap_2d(cls, 'vit_b_16', small, 1, 0, log=None)
    with pytest.raises(ValueError, match='export'):
        attack.uap_2d(cls, 'vit_b_16', small, 1, 2, export_views=[], log=None)
    with pytest.raises(ValueError, match='export'):
        attack.uap_2d(cls, 'vit_b_16', small, 1, 1, export_views=lambda n_pass: [], log=None)
    with pytest.raises(ValueError, match='native=True'):
        attack.uap_2d(cls, 'vit_b_16', small, 1, 2, native=True, log=None)
    with pytest.raises(ValueError, match='uint8'):
        attack.uap_2d(cls, 'vit_b_16', small.float(), 1, 2, log=None)


def test_more_than_one_rank_is_refused(images, cls, monkeypatch):
    from nerfail_amd import attack, sharding
    monkeypatch.setattr(sharding, 'world_and_rank', lambda group=None: (2, 0))
    with pytest.raises(ValueError, match='ranks'):
        attack.uap_2d(cls, 'vit_b_16', images[:1], 1, 2, log=None)


def test_epochs_1_exports_the_zero_table_of_an_odd_sized_three_channel_store():
    """5 x 7 views in a U8C3 store: rows and exported images at odd addresses; epochs == 1 is the export pass alone."""
    from nerfail_amd import attack
    rs = np.random.RandomState(3)
    store = rs.randint(0, 256, size=(3, 5, 7, 3)).astype(np.uint8)
    got = []
    res = attack.uap_2d(lambda x: x.mean((2, 3)).repeat(1, 3)[:, :8], 'my_model', torch.from_numpy(store), 1, 1, export_views=[2, 0],
                        on_export=lambda *a: got.append(a), log=None)
    assert len(res.stats) == 1 and res.stats[0]['epoch'] == 0 and res.stats[0]['next_epoch'] == 1 and res.stats[0]['views'] == 2
    assert not N(res.best).any() and not N(res.last).any() and res.stats[0]['taken'] == 1   # (the rule fires after the export pass too)
    assert [(e[0], e[1]) for e in got] == [(0, [2]), (1, [0])]
    for (_, (v,), adv, mask, ori) in got:
        assert np.array_equal(adv[0], store[v]) and np.array_equal(ori[0], store[v]) and not mask.any()
