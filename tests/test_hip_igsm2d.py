"""-m gpu: attack.igsm_2d, the IGSM-2D product loop. (a) against fixture g28 - the reference's universal_2D_net driven through
the IG:263-416 loop shape (tests/golden/make_golden_igsm2d.py) - with the stand-in classifier at 224 x 224: every iterate, every
taken flag, the best epoch, the accuracies and the exported uint8 images equal to the fixture, the losses within twice the
fixture's own float32-to-float64 distance plus 1e-6; (b) the native MyCNN path against the general one at 766 x 766, the
smallest size MyCNN accepts: bitwise equal; (c) GaussNet.universal_2D_net against nerfail_u2d_fwd, forward and backward.

As for g24 the stand-in classifier is evaluated in float64 and rounded once on both sides (order-independent logits)."""
import numpy as np
import pytest
import torch

import igsm2d_ref as IR
from hiputil import N, dev

pytestmark = pytest.mark.gpu
TAGS = ('untargeted', 'targeted')


@pytest.fixture(scope='module')
def g(golden):
    return golden('g28_igsm2d')


@pytest.fixture(scope='module')
def runs(g):
    """Each of g28's runs once, with the checksums of every iterate, every exported batch and the log lines."""
    from nerfail_amd import attack
    w = torch.from_numpy(g['cls_w']).to(dev())

    class Cls(torch.nn.Module):
        def forward(self, x):
            return (torch.nn.functional.adaptive_avg_pool2d(x.double(), 4).reshape(x.shape[0], -1) @ w.double().t()).float()
    images = torch.from_numpy(IR.g28_images(int(g['seed']), g['tints']))
    out = {}
    orig = attack._igsm2d_batch_done
    for i, tag in enumerate(TAGS):
        assert str(g['tags'][i]) == tag
        sums, exported, lines = [], [], []
        attack._igsm2d_batch_done = lambda e, b, table, sums=sums: sums.append(IR.checksums(N(table)))
        try:
            res = attack.igsm_2d(Cls(), 'vit_b_16', images, int(g['label'][i]), int(g['shape'][4]), float(g['a']), float(g['epsilon']),
                                 bool(g['targeted'][i]), batch_size=int(g['shape'][5]),
                                 on_export=lambda bi, vids, adv, mask, exported=exported: exported.append((bi, vids, adv, mask)), log=lines.append)
        finally:
            attack._igsm2d_batch_done = orig
        out[tag] = (res, sums, exported, lines)
    return out


@pytest.mark.parametrize('tag', TAGS)
def test_iterates_best_and_flags_equal_the_fixture(g, runs, tag):
    res, sums = runs[tag][:2]
    a = float(g['a'])
    want = g[tag + '_sums']
    assert len(sums) == want.shape[0]
    for k, s in enumerate(sums):
        assert np.array_equal(s, want[k]), (tag, k)
    assert np.array_equal(N(res.best), g[tag + '_best'].astype(np.float32) * a)
    assert np.array_equal(N(res.last), g[tag + '_last'].astype(np.float32) * a)
    assert tuple(res.best.shape) == tuple(res.last.shape) == (4, 224, 224, 3)
    assert not np.array_equal(N(res.best), N(res.last))                    # the fixture's point: a tie is not taken
    assert [d['taken'] for d in res.stats] == g[tag + '_taken'].tolist()
    assert res.best_epoch == int(g[tag + '_best_epoch'])


@pytest.mark.parametrize('tag', TAGS)
def test_accuracies_counts_and_log_lines(g, runs, tag):
    res, lines = runs[tag][0], runs[tag][3]
    s32 = g[tag + '_stats_f32']
    epochs = int(g['shape'][4])
    assert len(res.stats) == epochs and [d['epoch'] for d in res.stats] == list(range(epochs))
    for e, d in enumerate(res.stats):
        assert (d['views'], d['test_correct'], d['attack_correct']) == (int(s32[e, 6]), int(s32[e, 7]), int(s32[e, 8])), (tag, e, d)
        assert np.float32(d['test_acc']) == np.float32(s32[e, 1]) and np.float32(d['attack_acc']) == np.float32(s32[e, 3])   # exact
    assert res.best_acc == pytest.approx(float(s32[res.best_epoch, 3]), abs=1e-7)
    assert len(lines) == 5 * epochs and lines[0] == 'Attack ...... [0/4]' and lines[1].startswith('test Loss:')
    assert lines[3].startswith('attack Beta Loss:') and lines[4].startswith('attack Img Loss:')


@pytest.mark.parametrize('tag', TAGS)
def test_losses_within_the_fixtures_own_spread(g, runs, tag):
    """CE and image-loss means against the reference's float32 values: 2 x |reference f32 - reference f64| + 1e-6 relative."""
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
        print('g28 %s %s: worst error / bound %.3f (epoch %d: error %.3e, bound %.3e, got %.9g, reference f32 %.9g)' % ((tag, k) + r[:1] + r[2:]))
    for r in ratios:
        assert r[0] <= 1.0, (tag,) + r


@pytest.mark.parametrize('tag', TAGS)
def test_exported_images_equal_the_fixture(g, runs, tag):
    res, exported = runs[tag][0], runs[tag][2]
    assert [(bi, vids) for bi, vids, _, _ in exported] == [(0, [0, 1, 2]), (1, [3])]
    v = int(g['export_view'])
    _, vids, adv, mask = exported[0]
    assert adv.dtype == mask.dtype == np.uint8 and adv.shape == mask.shape == (3, 224, 224, 3)
    assert np.array_equal(adv[vids.index(v)], g[tag + '_export_adv_u8']) and np.array_equal(mask[vids.index(v)], g[tag + '_export_mask_u8'])
    best = N(res.best)
    assert np.array_equal(np.concatenate([e[3] for e in exported]), np.clip(best, 0, 255).astype(np.uint8))   # negative values become 0


def test_epochs_1_exports_the_zero_table(g):
    from nerfail_amd import attack
    images = IR.g28_images(int(g['seed']), g['tints'])
    got = []
    res = attack.igsm_2d(lambda x: x.mean((2, 3)), 'vit_b_16', torch.from_numpy(images[:2]), 1, 1, on_export=lambda *a: got.append(a), log=None)
    assert res.best_epoch == -1 and not N(res.best).any() and len(res.stats) == 1
    assert np.array_equal(got[0][2], IR.white(images[:2]).astype(np.uint8)) and not got[0][3].any()


def test_odd_sizes_and_a_three_channel_store():
    """5 x 7 views in a U8C3 store, a short last batch: rows of the table and exported images that start at odd addresses."""
    from nerfail_amd import attack
    rs = np.random.RandomState(3)
    images = rs.randint(0, 256, size=(5, 5, 7, 3)).astype(np.uint8)
    got = []
    res = attack.igsm_2d(lambda x: x.mean((2, 3)), 'my_model', torch.from_numpy(images), 1, 3, a=8., epsilon=16., batch_size=3,
                         on_export=lambda *a: got.append(a), log=None)
    assert [(g_[0], g_[1], g_[2].shape) for g_ in got] == [(0, [0, 1, 2], (3, 5, 7, 3)), (1, [3, 4], (2, 5, 7, 3))]
    best = N(res.best)
    assert np.abs(N(res.last)).max() == 16. and set(np.unique(best)) <= {-16., -8., 0., 8., 16.}
    assert np.array_equal(np.concatenate([g_[2] for g_ in got]), np.clip(images.astype(np.float32) + best, 0, 255).astype(np.uint8))
    assert np.array_equal(np.concatenate([g_[3] for g_ in got]), np.clip(best, 0, 255).astype(np.uint8))


# ------------------------------------------------------------------------------------------------------------ (b) native MyCNN
@pytest.fixture(scope='module')
def cnn_runs():
    from nerfail_amd import attack, ops
    from nerfail_amd.MyModel import MyCNN
    torch.manual_seed(7)
    model = MyCNN(num_classes=8).to(dev())
    rs = np.random.RandomState(7)
    images = rs.randint(0, 256, size=(3, 766, 766, 4)).astype(np.uint8)
    images[..., 3] = np.where(rs.uniform(size=(3, 766, 766)) < 0.7, 255, 0)
    images = torch.from_numpy(images).to(dev())
    out, seen = {}, []
    orig_fwd, orig_grad = ops.cnn_fwd, torch.autograd.grad

    def spy_fwd(packed, x, num_classes, keep_masks):
        res = orig_fwd(packed, x, num_classes, keep_masks)
        seen.append((bool(x.requires_grad), res[0].grad_fn is not None, torch.is_grad_enabled()))
        return res

    def no_grad_call(*a, **k):
        raise AssertionError('the native path called torch.autograd.grad')
    for native in (True, False):
        ops.cnn_fwd = spy_fwd
        if native:
            torch.autograd.grad = no_grad_call
        try:
            res = attack.igsm_2d(model, 'my_model', images, 3, 3, a=2., epsilon=4., targeted=False, batch_size=2, log=None, native=native)
        finally:
            ops.cnn_fwd, torch.autograd.grad = orig_fwd, orig_grad
        out[native] = (res, list(seen))
        del seen[:]
    return out


def test_native_and_general_path_are_bitwise_equal(cnn_runs):
    (nat, _), (gen, _) = cnn_runs[True], cnn_runs[False]
    nb, nl, gb, gl = N(nat.best), N(nat.last), N(gen.best), N(gen.last)
    print('native vs general: %d of %d elements of `last` differ, %d of `best`' % ((nl != gl).sum(), nl.size, (nb != gb).sum()))
    assert np.array_equal(nb.view(np.int32), gb.view(np.int32)) and np.array_equal(nl.view(np.int32), gl.view(np.int32))
    assert [d['taken'] for d in nat.stats] == [d['taken'] for d in gen.stats]
    assert nat.stats == gen.stats and nat.best_epoch == gen.best_epoch
    assert nl.any() and np.abs(nl).max() <= 4.


def test_native_path_builds_no_autograd_graph(cnn_runs):
    seen = cnn_runs[True][1]
    assert len(seen) >= 2 * 2                                             # 2 attack epochs x 2 batches (+ the clean logits, the export pass)
    assert not any(req or graph for req, graph, _ in seen)                 # the classifier input never requires grad; no graph
    assert any(req and graph for req, graph, _ in cnn_runs[False][1])      # (the general path does differentiate)


def test_native_true_needs_mycnn():
    from nerfail_amd import attack
    with pytest.raises(ValueError, match='native=True'):
        attack.igsm_2d(lambda x: x.mean((2, 3)), 'my_model', torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 0, 2, native=True)


# ------------------------------------------------------------------------------------------------------------ (c) universal_2D_net
@pytest.mark.parametrize('shared', (False, True))
def test_universal_2d_net_equals_u2d_fwd(shared):
    import nerfail_amd.ops as O
    from nerfail_amd.GaussNet import universal_2D_net
    H, W, B = 29, 37, 3
    rs = np.random.RandomState(11 + shared)
    images = rs.randint(0, 256, size=(5, H, W, 4)).astype(np.uint8)
    images[..., 3] = rs.randint(0, 2, size=(5, H, W)) * 255
    idx = [4, 0, 2]
    r_np = rs.uniform(-300, 300, size=(H, W, 3) if shared else (5, H, W, 3)).astype(np.float32)
    G = torch.from_numpy(rs.standard_normal((B, 3, H, W)).astype(np.float32)).to(dev())
    seen = []

    class Model(torch.nn.Module):
        def forward(self, x):
            seen.append(x)
            return (x * G).sum((2, 3))
    net = universal_2D_net(dev(), 0.02, Model(), 'my_model')
    st = torch.from_numpy(images).to(dev())
    table = torch.from_numpy(r_np).to(dev())
    x_rgb, cls_in, mask = O.u2d_fwd(st, torch.tensor(idx, device=dev()), table, True, True, True)
    r = (table if shared else table[idx]).clone().requires_grad_(True)
    ori = torch.from_numpy(IR.white(images[idx]).astype(np.uint8)).to(dev())     # the dataset's item (MD:247-255), stacked
    r_out, x2, cla, ori_f, ori_cla = net(r, ori)
    assert r_out is r and ori_f.dtype == torch.float32 and torch.equal(ori_f, ori.float())
    assert torch.equal(x2.view(torch.int32), x_rgb.view(torch.int32))
    assert torch.equal(seen[0].view(torch.int32), cls_in.view(torch.int32)) and seen[0].is_contiguous()
    assert torch.equal(seen[1], ori.float().permute(0, 3, 1, 2))
    grad, = torch.autograd.grad(cla.sum(), r)
    bits = ((mask[..., None] >> torch.arange(3, device=dev(), dtype=torch.uint8)) & 1).bool()
    want = torch.where(bits, G.permute(0, 2, 3, 1), torch.zeros((), device=dev()))
    if shared:
        want = (want[0] + want[1]) + want[2]
        assert torch.allclose(grad, want, rtol=0, atol=1e-6)              # three addends: the order of the sum is torch's
    else:
        assert torch.equal(grad.view(torch.int32), want.contiguous().view(torch.int32))
