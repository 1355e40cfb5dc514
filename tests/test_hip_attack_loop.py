"""-m gpu: attack.nerfail_s, the NeRFail-S product loop, against fixture g24 - the reference's gauss_net driven through the
AS:278-431 loop shape (tests/golden/make_golden_attack_loop.py): iterates, best tensor and epoch, epoch statistics, export.

Statistics bound (the project's own-spread yardstick): a CE or image-loss mean may differ from the reference's float32 value
by 2 x |reference f32 - reference f64| + 1e-6 relative. The measured ratios error / bound are printed by the test and
recorded in DESIGN.md section 4.

That spread is taken on the reference's own float32 logits, so it is only meaningful if both sides see the same logits. The
HIP gauss forward gives the reference's x_rgba bit for bit (measured on the fixture's best tensors: 0 differing elements), but
a stand-in classifier evaluated in float32 does not give the same logits on two machines: its 64-pixel means and 48-term
products are added in whatever order the library at hand picks (two CPUs running the generator: logits 2e-5 apart; GPU against
CPU: 1e-5 - all of it 1.5x to 8x outside the bound for the attacked CE). The fixture's generator and these tests therefore
evaluate the stand-in classifier - same weights, same function - in float64, rounded to float32 once (PoolCls64 in
tests/golden/make_golden_attack_loop.py, Cls in tests/mgpu/attack_loop_problem.py): order-independent logits, and the bound
as the issue states it."""
import os

import numpy as np
import pytest
import torch

import attack_loop_ref as R
from conftest import ROOT
from hiputil import N, dev
from mgpu import attack_loop_problem as AP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g():
    return AP.load()


@pytest.fixture(scope='module')
def runs(g):
    """Each of g24's three runs once, with every iterate (the perturbation after each attack batch) and every exported batch."""
    from nerfail_amd import attack
    out = {}
    orig, orig_batch = attack._attack_batch, attack._EpochStats.batch
    for tag in AP.TAGS:
        iterates, exported, lines, logits = [], [], [], []

        def spy(*a, **k):
            s = orig(*a, **k)
            iterates.append(N(s))
            return s
        def spy_batch(self, epoch, cla, ori_cla, x_rgba, views, logits=logits):
            logits.append((epoch, N(cla), N(ori_cla)))
            return orig_batch(self, epoch, cla, ori_cla, x_rgba, views)
        attack._attack_batch, attack._EpochStats.batch = spy, spy_batch
        try:
            res, env = AP.run(g, tag, dev(), on_export=lambda i, vids, adv, mask: exported.append((i, vids, adv, mask)), log=lines.append)
        finally:
            attack._attack_batch, attack._EpochStats.batch = orig, orig_batch
        out[tag] = (res, iterates, exported, lines, logits)
    return out


@pytest.mark.parametrize('tag', AP.TAGS)
def test_iterates_and_best_match_reference(g, runs, tag):
    """The criterion of the g15 loop test (test_hip_gauss.py): a sign step can differ from the reference only where the gradient
    is at rounding level - every element within 2 a, alpha untouched, fewer than 2e-3 of the elements different."""
    res, iterates = runs[tag][:2]
    ref = g[tag + '_iterates_rgb_int8'].astype(np.float32)
    a = float(g['a'])
    assert len(iterates) == ref.shape[0]

    def held(s, want, what):
        frac = float((s[..., :3] != want).mean())
        assert np.abs(s[..., :3] - want).max() <= 2 * a, what
        assert np.array_equal(s[..., 3], g['s0'][..., 3]), what
        assert frac < 2e-3, (what, frac)
        return frac
    worst = max(held(s, ref[i], i) for i, s in enumerate(iterates))
    assert res.best_epoch == int(g[tag + '_best_epoch'])
    worst = max(worst, held(N(res.best), g[tag + '_best'][..., :3], 'best'), held(N(res.last), g[tag + '_last'][..., :3], 'last'))
    print('g24 %s: worst fraction of elements that differ from the reference iterates %.2e' % (tag, worst))
    assert np.array_equal(N(res.best), iterates[2 * res.best_epoch + 1])       # the iterate after the best epoch's last batch, bit for bit
    assert np.array_equal(N(res.last), iterates[-1])
    if tag == 'beta':
        assert not np.array_equal(N(res.best), N(res.last))                    # the fixture's point: best != last


@pytest.mark.parametrize('tag', AP.TAGS)
def test_epoch_counts_accuracies_and_rule_match_reference(g, runs, tag):
    res, lines = runs[tag][0], runs[tag][3]
    s32 = g[tag + '_stats_f32']
    epochs = int(g['shape'][4])
    assert len(res.stats) == epochs and [d['epoch'] for d in res.stats] == list(range(epochs))
    for e, d in enumerate(res.stats):
        assert (d['views'], d['test_correct'], d['attack_correct']) == (int(s32[e, 6]), int(s32[e, 7]), int(s32[e, 8])), (tag, e, d)
        assert np.float32(d['test_acc']) == np.float32(s32[e, 1]) and np.float32(d['attack_acc']) == np.float32(s32[e, 3])   # exact
        assert d['taken'] == int(g[tag + '_taken'][e]), (tag, e)
    assert res.best_acc == pytest.approx(float(s32[res.best_epoch, 3]), abs=1e-7)
    assert len(lines) == 7 * epochs and lines[1].startswith('test Loss:') and lines[2].startswith('attack Loss:')


@pytest.mark.parametrize('tag', AP.TAGS)
def test_epoch_losses_within_reference_spread(g, runs, tag):
    """CE and image-loss means against the reference's float32 values, bound 2 x |reference f32 - reference f64| + 1e-6
    relative (module docstring: why the stand-in classifier is evaluated in float64 on both sides)."""
    res = runs[tag][0]
    s32, s64 = g[tag + '_stats_f32'], g[tag + '_stats_f64']
    ratios = []
    for e, d in enumerate(res.stats):
        for key, i32, i64 in (('test_loss', 0, 0), ('attack_loss', 2, 1), ('img_loss', 4, 2)):
            ref32, ref64 = float(s32[e, i32]), float(s64[e, i64])
            bound = 2 * abs(ref32 - ref64) + 1e-6 * abs(ref32)
            err = abs(d[key] - ref32)
            ratios.append((err / bound if bound > 0 else (0. if err == 0 else np.inf), key, e, err, bound, d[key], ref32))
    for k in ('test_loss', 'attack_loss', 'img_loss'):
        r = max(r for r in ratios if r[1] == k)
        print('g24 %s %s: worst error / bound %.3f (epoch %d: error %.3e, bound %.3e, got %.9g, reference f32 %.9g)' % ((tag, k) + r[:1] + r[2:]))
    for r in ratios:
        assert r[0] <= 1.0, (tag,) + r


@pytest.mark.parametrize('tag', AP.TAGS)
def test_statistics_are_exact_for_the_logits_of_the_run(g, runs, tag):
    """The epoch records against the float64 restatement applied to the logits this run produced: equal to float32 rounding.
    Also prints how far those logits are from the reference's (the fixture stores them)."""
    res, logits = runs[tag][0], runs[tag][4]
    _, _, label = AP.run_args(g, tag)
    epochs = int(g['shape'][4])
    far = 0.
    for e in range(epochs):
        mine = [l for l in logits if l[0] == e]
        row = np.zeros(R.ROW, np.float32)
        for _, cla, ori_cla in mine:
            row = R.add_to_row(row, stats=R.logit_stats(cla, ori_cla, label))
        row[9] = 1.
        rec = R.epoch_close(row, R.best_init(False), e, False)[0]
        d = res.stats[e]
        assert abs(d['test_loss'] - float(rec[0])) <= 1.2e-7 * abs(float(rec[0])) and abs(d['attack_loss'] - float(rec[2])) <= 1.2e-7 * abs(float(rec[2]))
        ref_cla = g[tag + '_export_cla'] if e == epochs - 1 else g[tag + '_train_cla'][e]
        far = max(far, float(np.abs(np.concatenate([m[1] for m in mine]) - ref_cla).max()))
    print('g24 %s: largest |logit - reference logit| %.2e (logits up to %.1f)' % (tag, far, float(np.abs(g[tag + '_train_cla']).max())))
    # a logit is a float32 sum of 48 weighted means of 64 pixels each: two correct float32 evaluations in different orders may
    # differ by ~(48 + 64) x 2^-24 of the sum of the terms' magnitudes (a few hundred) - 1e-4 of the largest logit covers it
    assert far <= 1e-4 * float(np.abs(g[tag + '_train_cla']).max())


def test_export_pass(g, runs):
    """The export epoch renders the BEST tensor over all eight views. Its images are, exactly, the cv2.imwrite conversion of
    what the gauss forward makes of that tensor; and they are the reference's x_rgba / x through the same conversion (at most
    one level apart where a value sits at a rounding boundary) on every pixel none of whose eight table rows differs from the
    reference's best tensor - the iterate criterion allows < 2e-3 of the elements to differ, so nearly all pixels."""
    from nerfail_amd.GaussNet import gauss_gather
    from hiputil import T
    for tag in AP.TAGS:
        res, exported = runs[tag][0], runs[tag][2]
        assert [e[0] for e in exported] == [0, 1] and [e[2].shape for e in exported] == [(4, 32, 32, 4)] * 2
        adv, mask = np.concatenate([e[2] for e in exported]), np.concatenate([e[3] for e in exported])
        assert adv.dtype == np.uint8 and mask.dtype == np.uint8
        assert res.stats[-1]['views'] == 8
        x, xr = gauss_gather(res.best, T(g['wi']), T(g['ori']), None)
        assert np.array_equal(adv, R.export_u8(N(xr))) and np.array_equal(mask, R.export_u8(N(x)))
        changed = (N(res.best) != g[tag + '_best']).any(-1).reshape(-1)                    # table rows that differ from the reference's
        clean = ~changed[g['wi'][:, 1].astype(np.int64)].any(-1)                           # [8,H,W]: pixels fed by unchanged rows only
        print('g24 %s export: %d of %d table rows differ from the reference best, %.4f of the pixels compared' % (tag, changed.sum(), changed.size, clean.mean()))
        assert clean.mean() > 0.9
        for got, want in ((adv, R.export_u8(g[tag + '_export_x_rgba'])), (mask, R.export_u8(g[tag + '_export_x']))):
            d = np.abs(got.astype(np.int32) - want.astype(np.int32))[clean]
            assert d.max() <= 1 and (d != 0).mean() < 1e-3, (tag, d.max(), (d != 0).mean())
        assert np.array_equal(adv[..., 3], g['ori'][..., 3].astype(np.uint8))


def test_beta_zero_last_is_bitwise_nerfail_s_loop(g):
    from nerfail_amd.attack import nerfail_s_loop
    for tag in ('untargeted', 'targeted'):
        targeted, beta, label = AP.run_args(g, tag)
        res, (net, s0, train, export) = AP.run(g, tag, dev())
        net2, s0b, train2, _ = AP.setup(g, dev())
        want = nerfail_s_loop(net2, s0b, s0b, train2, torch.tensor(label, device=dev()), int(g['shape'][4]) - 1, float(g['a']),
                              float(g['epsilon']), targeted)
        assert torch.equal(res.last, want.view(res.last.shape)), tag


@pytest.mark.parametrize('fused', (True, False))
def test_every_iterate_of_an_epoch_is_bitwise_nerfail_s_step(g, fused):
    """One attack epoch of nerfail_s with beta == 0 against nerfail_s_step fed the same batches one by one, with the sign step
    fused into the gather backward and as a kernel of its own: the loop and the step are one body, iterate by iterate."""
    from nerfail_amd import attack
    targeted, beta, label = AP.run_args(g, 'untargeted')
    assert beta == 0.
    net, s0, train, export = AP.setup(g, dev())
    net.fused_sign_step = fused
    calls, orig = [], attack._attack_batch

    def spy(net_, s, s_init, batch, *a, **k):
        out = orig(net_, s, s_init, batch, *a, **k)
        calls.append((s, batch, out))
        return out
    attack._attack_batch = spy
    try:
        res = attack.nerfail_s(net, s0, train, label, 2, float(g['a']), float(g['epsilon']), targeted, beta, export_batches=export, log=None)
    finally:
        attack._attack_batch = orig
    assert len(calls) == len(train) == 2
    net2, s0b, _, _ = AP.setup(g, dev())
    net2.fused_sign_step = fused
    s = s0b
    for s_in, batch, s_out in calls:
        assert torch.equal(s_in, s)
        s, _ = attack.nerfail_s_step(net2, s, s0b, batch[0], batch[1], torch.tensor(label, device=dev()), float(g['a']), float(g['epsilon']), targeted)
        assert torch.equal(s, s_out) and not torch.equal(s, s_in)
    assert torch.equal(res.last, s)


def test_one_epoch_exports_the_initial_tensor(g):
    from nerfail_amd.GaussNet import gauss_gather
    exported = []
    res, (net, s0, train, export) = AP.run(g, 'untargeted', dev(), epochs=1, on_export=lambda i, v, adv, mask: exported.append((adv, mask)))
    assert torch.equal(res.best, s0) and torch.equal(res.last, s0) and res.best_epoch == -1 and res.best_acc is None
    assert len(res.stats) == 1 and res.stats[0]['views'] == 8 and len(exported) == 2
    x, xr = gauss_gather(s0, export[0][0], export[0][1], None)
    assert np.array_equal(exported[0][0], R.export_u8(N(xr))) and np.array_equal(exported[0][1], R.export_u8(N(x)))
    opaque = g['ori'][:4, ..., 3] > 0
    assert np.array_equal(exported[0][0][opaque], g['ori'][:4].astype(np.uint8)[opaque])      # a zero perturbation: the clean pixels


def test_uint8_resident_images_give_the_same_run(g):
    targeted, beta, label = AP.run_args(g, 'beta')
    from nerfail_amd.attack import nerfail_s
    out = []
    for u8 in (False, True):
        net, s0, train, export = AP.setup(g, dev(), ori_u8=u8)
        out.append(nerfail_s(net, s0, train, label, 3, float(g['a']), float(g['epsilon']), targeted, beta, export_batches=export, log=None))
    assert torch.equal(out[0].best, out[1].best) and torch.equal(out[0].last, out[1].last)
    assert [d['img_loss'] for d in out[0].stats] == [d['img_loss'] for d in out[1].stats]


def _sync_mode_works():
    x = torch.ones(1, device=dev())
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            x.item()
        except RuntimeError:
            return True
        return False
    finally:
        torch.cuda.set_sync_debug_mode(prev)


def test_no_host_wait_inside_an_epoch(g, monkeypatch):
    """Everything but the one read per epoch end (attack._read_stats) and the export epoch's image copies runs with host
    waits forbidden: torch's sync debug mode where this build honours it, else Tensor.item / cpu / tolist refused."""
    from nerfail_amd import attack
    targeted, beta, label = AP.run_args(g, 'beta')
    net, s0, train, export = AP.setup(g, dev(), view_ids=True)
    args = (float(g['a']), float(g['epsilon']), targeted, beta)
    attack.nerfail_s(net, s0, train, label, 2, *args, export_batches=export, log=None)       # first pass: indices, caches, allocations
    torch.cuda.synchronize()
    native = _sync_mode_works()
    print('set_sync_debug_mode("error") catches a host wait on this build:', native)
    prev = torch.cuda.get_sync_debug_mode()
    orig = {name: getattr(torch.Tensor, name) for name in ('item', 'cpu', 'tolist')}
    guarded = [False]

    def forbid(on):
        guarded[0] = on
        if native:
            torch.cuda.set_sync_debug_mode('error' if on else prev)

    def refuse(name):
        def f(self, *a, **k):
            if guarded[0] and self.is_cuda:
                raise AssertionError('Tensor.%s on a device tensor inside an epoch' % name)
            return orig[name](self, *a, **k)
        return f
    if not native:
        for name in orig:
            monkeypatch.setattr(torch.Tensor, name, refuse(name))
    reads = []
    read = attack._read_stats

    def read_unguarded(*a):
        forbid(False)
        try:
            reads.append(1)
            return read(*a)
        finally:
            forbid(True)
    monkeypatch.setattr(attack, '_read_stats', read_unguarded)
    try:
        forbid(True)
        res = attack.nerfail_s(net, s0, train, label, 4, *args, export_batches=export, log=None)    # three attack epochs + export, no on_export
    finally:
        forbid(False)
        torch.cuda.set_sync_debug_mode(prev)
        monkeypatch.undo()
    assert len(reads) == 4 and len(res.stats) == 4 and res.stats[-1]['views'] == 8


def test_two_ranks_agree_with_one(g, rank_launcher, tmp_path):
    """Two gloo ranks on the one GPU: every rank ends with the same best tensor and records; against one rank the counts are
    exact and the sums inside the statistics bound (each rank's share is summed first, then the two shares)."""
    from nerfail_amd.attack import STAT_FIELDS
    script = os.path.join(ROOT, 'tests', 'mgpu', 'attack_loop_rank.py')
    for world in (1, 2):
        rep = rank_launcher(script, world, [str(tmp_path)], timeout=300)
        assert rep['rc'] == [0] * world, '\n'.join(rep['logs'])
    one = dict(np.load(tmp_path / 'loop_w1_r0.npz'))
    two = [dict(np.load(tmp_path / ('loop_w2_r%d.npz' % r))) for r in range(2)]
    col = {k: i for i, k in enumerate(STAT_FIELDS)}
    for tag in ('beta', 'untargeted'):
        assert np.array_equal(two[0][tag + '_best'], two[1][tag + '_best']) and np.array_equal(two[0][tag + '_last'], two[1][tag + '_last'])
        assert np.array_equal(two[0][tag + '_stats'], two[1][tag + '_stats'])
        assert int(two[0][tag + '_best_epoch']) == int(one[tag + '_best_epoch']) == int(g[tag + '_best_epoch'])
        frac = float((two[0][tag + '_best'] != one[tag + '_best']).mean())
        assert frac < 2e-3 and np.abs(two[0][tag + '_best'] - one[tag + '_best']).max() <= 2 * float(g['a']), frac
        a, b = two[0][tag + '_stats'], one[tag + '_stats']
        for k in ('views', 'taken', 'best_epoch', 'epoch', 'test_correct', 'attack_correct', 'test_acc', 'attack_acc', 'best_acc'):
            assert np.array_equal(a[:, col[k]], b[:, col[k]]), (tag, k)
        s32, s64 = g[tag + '_stats_f32'], g[tag + '_stats_f64']
        for k, i32, i64 in (('test_loss', 0, 0), ('attack_loss', 2, 1), ('img_loss', 4, 2)):
            bound = 2 * np.abs(s32[:, i32] - s64[:, i64]) + 1e-6 * np.abs(s32[:, i32])
            err = np.abs(a[:, col[k]] - b[:, col[k]])
            print('two ranks vs one, %s %s: worst error / bound %.3f' % (tag, k, float((err / bound).max())))
            assert (err <= bound).all(), (tag, k, err, bound)
        assert two[0][tag + '_exported'][:, 1].tolist() == [2, 2] and two[1][tag + '_exported'][:, 1].tolist() == [2, 2]
        assert one[tag + '_exported'][:, 1].tolist() == [4, 4]
