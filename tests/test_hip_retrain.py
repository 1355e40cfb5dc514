"""-m gpu: the retrain stage as a product, at toy size, against the file path it replaces.

A 16 x 16 Blender-format scene on disk (test_load_blender.write_toy_scene), a tiny stock-torch victim (global mean, then a Linear).
Each of the four attack loops runs with BOTH on_export - whose uint8 images are written as PNGs (PIL; channel order flipped as
cv2.imwrite would) and read back through load_blender_data(train_dir=...) and training_images - and export_sink, a
PoisonedTrainSet: the sink's stores must equal the file path's arrays bit for bit, and `best` must not notice the sink. Then
RayBatcher.from_resident against the uploading constructor, train() from either, and poisoned_retrain against the hand-written
chain (file path, train.train, evaluate_render), its restart rule, its refusals and its folders.

The NeRFs are test_hip_pipeline's depth (4) at width 256, not its width 64: parameters are compared bit for bit between runs, and
only the W = 256 weight-gradient kernel adds in a fixed order (csrc/mlp_dw.hip: the kernel for other widths uses float atomics,
so two runs of the SAME code at W = 64 already differ in their last bits - measured here: from_resident against itself).
16 + 16 samples and 64 rays keep a step cheap."""
import os
import types

import numpy as np
import pytest
import torch

from hiputil import T, N, dev
from test_load_blender import write_toy_scene

pytestmark = pytest.mark.gpu

H = W = 16
N_TRAIN, LABEL, CLASSES = 3, 2, 8
NAME = 'tiny_linear'                                                       # not "my_model": evaluate_views resizes (to resize_to = 16)
IDS = [('retrain16', v) for v in range(N_TRAIN)]                           # the names the 3-D attacks know the train views by


class TinyCls(torch.nn.Module):
    """Global mean, then a Linear; evaluated in float64 and rounded once (order-independent logits, as the other loop tests)."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.lin = torch.nn.Linear(3, CLASSES)
        with torch.no_grad():
            self.lin.weight.copy_(torch.randn(CLASSES, 3, generator=g) * 0.05)
            self.lin.bias.copy_(torch.randn(CLASSES, generator=g) * 0.1)

    def forward(self, x):
        return (x.double().mean((2, 3)) @ self.lin.weight.double().t() + self.lin.bias.double()).float()


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    from nerfail_amd import GaussNet as G
    from nerfail_amd.load_blender import load_blender_data, training_images
    G._VIEW_CACHE.clear(); G._BATCH_KEYS.clear()
    root = str(tmp_path_factory.mktemp('retrain') / 'scene')
    raw = write_toy_scene(root, H=H, W=W, n=(N_TRAIN, 2, 2), seed=3)       # RGBA, the files' order
    images, poses, _, hwf, i_split = load_blender_data(root)
    focal = hwf[2]
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    bgra = {k: np.ascontiguousarray(v[..., [2, 1, 0, 3]]) for k, v in raw.items()}      # as cv2 reads them
    rs = np.random.RandomState(11)
    Pn = 2                                                                  # point-set views behind the perturbation table
    w = rs.uniform(0.1, 1., size=(N_TRAIN, H, W, 8)).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    idx = rs.randint(0, Pn * H * W, size=(N_TRAIN, H, W, 8)).astype(np.float32)
    s0 = np.zeros((Pn, H, W, 4), np.float32)
    s0[..., 3] = 255.
    return types.SimpleNamespace(root=root, raw=raw, bgra=bgra, poses=poses, hwf=hwf, i_split=i_split, K=K,
                                 clean=training_images(images, white_bkgd=True), wi=T(np.stack([w, idx], 1)), ori=T(bgra['train'].astype(np.float32)),
                                 s0=T(s0), store=T(bgra['train']), cls=TinyCls().to(dev()).eval().requires_grad_(False))


def _file_path(scene, directory, per_view_u8):
    """The reference's road: the exported uint8 images (cv2's channel order) as PNGs named like the train files, then
    load_blender_data(train_dir=...) and training_images. Returns the [n,H,W,3] targets of the train views."""
    from PIL import Image
    from nerfail_amd.load_blender import load_blender_data, training_images
    os.makedirs(directory)
    for v, img in per_view_u8.items():
        mode, order = ('RGBA', [2, 1, 0, 3]) if img.shape[-1] == 4 else ('RGB', [2, 1, 0])
        Image.fromarray(np.ascontiguousarray(img[..., order]), mode).save(os.path.join(directory, 'r_%d.png' % v))
    images, poses, _, hwf, i_split = load_blender_data(scene.root, train_dir=directory)
    imgs = training_images(images, white_bkgd=True, train_dir=directory)
    assert np.array_equal(imgs[N_TRAIN:], scene.clean[N_TRAIN:])
    return imgs


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run_attack(scene, which, sink, on_export):
    from nerfail_amd import attack
    from nerfail_amd.GaussNet import gauss_net
    kw = dict(on_export=on_export, log=None)
    if which in ('nerfail_s', 'nerfail'):
        net = gauss_net(dev(), 0.02, scene.cls, 'my_model', epsilon=None)
        if which == 'nerfail_s':
            batches = [(scene.wi[0:2].contiguous(), scene.ori[0:2].contiguous(), IDS[0:2]), (scene.wi[2:3].contiguous(), scene.ori[2:3].contiguous(), IDS[2:3])]
            if sink is None:
                return attack.nerfail_s(net, scene.s0, batches, LABEL, 3, a=4., epsilon=32., **kw).best
            return attack.nerfail_s_into(sink, net, scene.s0, batches, LABEL, 3, a=4., epsilon=32., **kw).best
        if sink is not None:
            kw['export_sink'] = sink
        views = [(scene.wi[v:v + 1].contiguous(), scene.ori[v:v + 1].contiguous(), IDS[v]) for v in range(N_TRAIN)]
        return attack.nerfail(net, scene.s0, views, LABEL, 2, m1=1, m2=1, df_max_iter=3, num_classes=CLASSES, accumulate_incomplete=True, **kw).best
    if sink is not None:
        kw['export_sink'] = sink
    if which == 'igsm_2d':
        return attack.igsm_2d(scene.cls, 'my_model', scene.store, LABEL, 3, a=4., epsilon=32., batch_size=2, **kw).best
    # overshoot multiplies the accumulated direction (DF:102): at 50 one DeepFool step crosses the boundary, so calls complete
    return attack.uap_2d(scene.cls, 'my_model', scene.store, LABEL, 2, epsilon=32., m1=1, m2=1, df_max_iter=6, overshoot=50., num_classes=CLASSES,
                         **kw).best


@pytest.mark.parametrize('which, channels', [('nerfail_s', 4), ('nerfail', 4), ('igsm_2d', 3), ('uap_2d', 3)])
def test_sink_equals_the_file_path_for_every_attack_loop(scene, tmp_path, which, channels):
    from nerfail_amd.retrain import PoisonedTrainSet
    ids = IDS if channels == 4 else list(range(N_TRAIN))
    exported = {}

    def on_export(index, view_ids, adv_u8, *rest):
        assert adv_u8.dtype == np.uint8 and adv_u8.shape == (len(view_ids), H, W, channels)
        for v, img in zip(view_ids, adv_u8):
            exported[ids.index(v)] = img.copy()
    sink = PoisonedTrainSet(ids, H, W, channels)
    best = _run_attack(scene, which, sink, on_export)
    assert sorted(exported) == list(range(N_TRAIN)) and sink.missing() == []
    sink.require_complete()
    want = _file_path(scene, str(tmp_path / 'adv'), exported)
    got = N(sink.images)
    assert got.shape == (N_TRAIN, H, W, 3) and np.array_equal(_bits(got), _bits(want[:N_TRAIN]))
    assert not np.array_equal(got, scene.clean[:N_TRAIN])                   # the attack moved the views
    assert np.array_equal(N(sink.adv_u8), np.stack([exported[v] for v in range(N_TRAIN)]))
    # the sink alone: no host copy is asked for, and the attack's result does not notice either hook
    sink2 = PoisonedTrainSet(ids, H, W, channels)
    best2 = _run_attack(scene, which, sink2, None)
    best3 = _run_attack(scene, which, None, None)
    assert torch.equal(best, best2) and torch.equal(best, best3)
    assert torch.equal(sink2.images, sink.images) and torch.equal(sink2.adv_u8, sink.adv_u8)


def test_sink_refusals(scene):
    from nerfail_amd.retrain import PoisonedTrainSet
    sink = PoisonedTrainSet([0, 1, 2], H, W, 4)
    x = scene.ori[:2].contiguous()
    with pytest.raises(ValueError, match='no view ids'):
        sink.put(None, x)
    with pytest.raises(ValueError, match='not among'):
        sink.put([0, 7], x)
    with pytest.raises(ValueError, match=r'\[2,16,16,4\]'):
        sink.put([0, 1], scene.ori[:2, :, :, :3].contiguous())
    sink.put([2, 0], x)
    assert sink.missing() == [1]
    with pytest.raises(ValueError, match=r'1 of 3 train views were never exported: \[1\]'):
        sink.require_complete()
    assert np.array_equal(N(sink.adv_u8[2]), scene.bgra['train'][0]) and np.array_equal(N(sink.adv_u8[0]), scene.bgra['train'][1])
    assert np.array_equal(_bits(N(sink.images[2])), _bits(scene.clean[0]))  # a clean view through the hand-off is the clean target


# ---------------------------------------------------------------------------------------------- the batcher and the loop
def _args(basedir, **over):
    a = types.SimpleNamespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=16, N_samples=16,
                              netdepth=4, netwidth=256, netdepth_fine=4, netwidth_fine=256, netchunk=65536, lrate=5e-4, lrate_decay=250,
                              basedir=basedir, expname='retrain_toy', ft_path=None, no_reload=False, perturb=1., white_bkgd=True,
                              raw_noise_std=0., dataset_type='blender', no_ndc=False, lindisp=False, N_rand=64, no_batching=True,
                              precrop_iters=0, precrop_frac=.5, i_print=2, i_weights=1000, chunk=1024)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _make_nerf(args, calls=None):
    from nerfail_amd import run_nerf as RN

    def make(attempt):
        if calls is not None:
            calls.append(attempt)
        torch.manual_seed(100 + attempt)
        out = RN.create_nerf(args)
        with torch.no_grad():            # a freshly initialised NeRF has sigma <= 0 nearly everywhere: the fixtures' nudge
            for net in (out[0]['network_fn'], out[0]['network_fine']):
                net.alpha_linear.bias += 0.5
        return out
    return make


@pytest.fixture(scope='module')
def poisoned(scene, tmp_path_factory):
    """The train views attacked by a fixed perturbation, once through the sink and once through the files."""
    from nerfail_amd.retrain import PoisonedTrainSet
    rs = np.random.RandomState(21)
    x = scene.bgra['train'].astype(np.float32)
    x[..., :3] += rs.uniform(-32., 32., size=x[..., :3].shape).astype(np.float32)
    sink = PoisonedTrainSet(list(range(N_TRAIN)), H, W, 4)
    sink.put([0, 1], T(x[:2]))
    sink.put([2], T(x[2:]))
    adv = N(sink.adv_u8)
    files = _file_path(scene, str(tmp_path_factory.mktemp('poisoned') / 'adv'), {v: adv[v] for v in range(N_TRAIN)})
    assert np.array_equal(_bits(N(sink.images)), _bits(files[:N_TRAIN]))
    return types.SimpleNamespace(sink=sink, files=files, adv=adv)


def test_from_resident_yields_the_rays_and_targets_of_the_file_path_batcher(scene, poisoned):
    from nerfail_amd.train import RayBatcher
    i_train = scene.i_split[0]
    a = RayBatcher(poisoned.files, scene.poses, i_train, scene.hwf, scene.K, 2., 6., seed=4)
    b = RayBatcher.from_resident(poisoned.sink.images, scene.poses, i_train, scene.hwf, scene.K, 2., 6., seed=4)
    assert b.images.data_ptr() == poisoned.sink.images.data_ptr()          # adopted, not copied
    assert torch.equal(a.images, b.images) and torch.equal(a.poses, b.poses)
    for step in range(1, 4):
        for kw in (dict(), dict(precrop=.5), dict(use_batching=True)):
            (ra, ta), (rb, tb) = a.batch(step, 50, **kw), b.batch(step, 50, **kw)
            assert torch.equal(ra, rb) and torch.equal(ta, tb) and ta.shape[1] == 3 and ra.shape[0] > 0
    ra, ta, sa = a.batch(9, 300, view=2, return_sel=True)
    rb, tb, sb = b.batch(9, 300, view=2, return_sel=True)
    assert torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(sa, sb)
    assert np.array_equal(_bits(N(tb)), _bits(poisoned.files[2].reshape(-1, 3)[N(sb)]))         # the targets ARE the file path's pixels
    with pytest.raises(ValueError, match='one slot per view'):
        RayBatcher.from_resident(poisoned.sink.images[:2], scene.poses, i_train, scene.hwf, scene.K, 2., 6.)
    with pytest.raises(ValueError, match='on the device'):
        RayBatcher.from_resident(poisoned.sink.images.cpu(), scene.poses, i_train, scene.hwf, scene.K, 2., 6.)


def _params(render_kwargs_train):
    return [N(p).copy() for net in (render_kwargs_train['network_fn'], render_kwargs_train['network_fine']) for p in net.parameters()]


def _same_params(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_four_steps_of_train_from_either_batcher(scene, poisoned, tmp_path):
    from nerfail_amd.train import RayBatcher, train
    args = _args(str(tmp_path))
    out = []
    for resident in (False, True):
        rkt, _, start, grad_vars, opt = _make_nerf(args)(0)
        before = _params(rkt)
        if resident:
            batcher = RayBatcher.from_resident(poisoned.sink.images, scene.poses, scene.i_split[0], scene.hwf, scene.K, 2., 6., seed=0)
            last, logged = train(None, scene.poses, scene.i_split, scene.hwf, scene.K, args, rkt, opt, start, seed=0, N_iters=5, batcher=batcher, log=lambda s: None)
        else:
            last, logged = train(poisoned.files, scene.poses, scene.i_split, scene.hwf, scene.K, args, rkt, opt, start, seed=0, N_iters=5, log=lambda s: None)
        assert last == 4 and [l[0] for l in logged] == [2, 4] and all(np.isfinite(l[1:]).all() for l in logged)
        assert not _same_params(before, _params(rkt))
        out.append((_params(rkt), logged))
    assert _same_params(out[0][0], out[1][0]) and out[0][1] == out[1][1]


@pytest.fixture(scope='module')
def originals(scene):
    return {tag: T(scene.bgra[tag]) for tag in ('train', 'val', 'test')}


EVAL = dict(num_classes=CLASSES, resize_to=16, batch=2)


def test_poisoned_retrain_equals_the_hand_written_chain(scene, poisoned, originals, tmp_path):
    from nerfail_amd import model_test as MT
    from nerfail_amd.retrain import poisoned_retrain
    from nerfail_amd.train import train
    lines = []
    args = _args(str(tmp_path / 'product'))
    res = poisoned_retrain(poisoned.sink, scene.poses, scene.i_split, scene.hwf, scene.K, args, make_nerf=_make_nerf(args), originals=originals,
                           model=scene.cls, model_name=NAME, label=LABEL, N_iters=5, seed=0, log=lines.append, **EVAL)
    assert res.attempts == 1 and res.last_iteration == 4 and [l[0] for l in res.logged] == [2, 4]
    assert sorted(res.renders) == ['test', 'val'] and sorted(res.reports) == ['test', 'val']
    assert any(s.startswith('[TRAIN] Iter: 4') for s in lines)
    # the chain by hand: the PNGs' arrays, the uploading batcher inside train(), evaluate_render per split
    args2 = _args(str(tmp_path / 'chain'))
    rkt, rkte, start, grad_vars, opt = _make_nerf(args2)(0)
    assert start == 0
    last, logged = train(poisoned.files, scene.poses, scene.i_split, scene.hwf, scene.K, args2, rkt, opt, start, seed=0, N_iters=5, log=lambda s: None)
    assert _same_params(_params(res.render_kwargs_train), _params(rkt)) and logged == res.logged and last == res.last_iteration
    rkte.update(near=2., far=6.)
    for tag, split in (('val', 1), ('test', 2)):
        p = torch.from_numpy(scene.poses[scene.i_split[split]])
        want = MT.evaluate_render(rkte, p, scene.hwf, scene.K, args2.chunk, originals[tag], scene.cls, NAME, LABEL, **EVAL)
        assert res.reports[tag] == want, (tag, res.reports[tag], want)
        assert res.renders[tag].shape == (2, H, W, 3) and res.renders[tag].dtype == torch.uint8 and res.renders[tag].is_cuda
        assert want['e max'] > 0


def test_restart_rule(scene, poisoned, tmp_path):
    from nerfail_amd.retrain import poisoned_retrain
    common = dict(eval_tags=(), N_iters=5, seed=0)
    ref_args = _args(str(tmp_path / 'plain'))
    plain = poisoned_retrain(poisoned.sink, scene.poses, scene.i_split, scene.hwf, scene.K, ref_args, make_nerf=_make_nerf(ref_args), log=None, **common)
    assert plain.attempts == 1 and plain.renders == {} and plain.reports == {}
    # a floor nothing reaches: every attempt is discarded until none is left - max_restarts + 1 NeRFs, the last one kept
    calls, lines = [], []
    args = _args(str(tmp_path / 'never'))
    r = poisoned_retrain(poisoned.sink, scene.poses, scene.i_split, scene.hwf, scene.K, args, make_nerf=_make_nerf(args, calls),
                         restart_below=(2, 1e9), max_restarts=2, log=lines.append, **common)
    assert r.attempts == 3 and calls == [0, 1, 2] and r.last_iteration == 4 and [l[0] for l in r.logged] == [2, 4]
    assert sum('restarting' in s for s in lines) == 2 and sum('no restart left' in s for s in lines) == 1
    assert not _same_params(_params(r.render_kwargs_train), _params(plain.render_kwargs_train))      # attempt 2's NeRF, another seed
    assert not os.path.isdir(os.path.join(args.basedir, args.expname)) or not os.listdir(os.path.join(args.basedir, args.expname))
    # a floor everything reaches: one attempt, and judging it at iteration 2 changes nothing of the run
    calls = []
    args = _args(str(tmp_path / 'always'))
    r = poisoned_retrain(poisoned.sink, scene.poses, scene.i_split, scene.hwf, scene.K, args, make_nerf=_make_nerf(args, calls),
                         restart_below=(2, -1e9), max_restarts=2, log=None, **common)
    assert r.attempts == 1 and calls == [0] and r.logged == plain.logged
    assert _same_params(_params(r.render_kwargs_train), _params(plain.render_kwargs_train))
    for bad in ((3, 15.), (0, 15.), (1000, 15.), (6, 15.)):                 # not logged; not an iteration; at the first checkpoint; beyond N_iters
        with pytest.raises(ValueError, match='restart_below'):
            poisoned_retrain(poisoned.sink, scene.poses, scene.i_split, scene.hwf, scene.K, args, make_nerf=_make_nerf(args), restart_below=bad,
                             log=None, **common)


def test_refusals_checkpoint_and_folders(scene, poisoned, originals, tmp_path):
    from nerfail_amd import model_test as MT
    from nerfail_amd import run_nerf as RN
    from nerfail_amd.retrain import PoisonedTrainSet, attack_output_dir, poisoned_retrain, render_splits
    args = _args(str(tmp_path / 'logs'))
    half = PoisonedTrainSet(list(range(N_TRAIN)), H, W, 4)
    half.put([1], poisoned.sink.images.new_zeros((1, H, W, 4)))
    with pytest.raises(ValueError, match=r'never exported: \[0, 2\]'):
        poisoned_retrain(half, scene.poses, scene.i_split, scene.hwf, scene.K, args, make_nerf=_make_nerf(args), N_iters=5, log=None)
    # the folders: where attack_output_dir says, under names _indexed_files accepts, holding the renders
    save_dir = os.path.join(str(tmp_path), attack_output_dir(scene_name='lego', model_name=NAME, method_name='IGSM', step=1))
    assert save_dir.endswith(os.path.join('output', NAME, 'nerf', 'lego', 'NeRFail_S_3P_100_to_n_e_32_a_2'))
    res = poisoned_retrain(poisoned.sink, scene.poses, scene.i_split, scene.hwf, scene.K, args, make_nerf=_make_nerf(args), originals=originals,
                           model=scene.cls, model_name=NAME, label=LABEL, eval_tags=('test',), N_iters=3, save_dir=save_dir, log=None, **EVAL)
    assert sorted(res.renders) == ['test', 'train', 'val'] and sorted(res.reports) == ['test']
    for tag, n in (('train', N_TRAIN), ('val', 2), ('test', 2)):
        files = MT._indexed_files(os.path.join(save_dir, tag))
        assert sorted(files) == list(range(n))
        back = np.stack([MT._imread_unchanged(files[i]) for i in range(n)])
        assert np.array_equal(back, N(res.renders[tag]))
    # render_splits alone: the reference's folder names, the same bits
    again = render_splits(res.render_kwargs_test, scene.poses, scene.i_split, scene.hwf, scene.K, args.chunk, savedir=str(tmp_path / 'ro'), start=7)
    assert list(again) == ['test', 'train', 'val'] and all(torch.equal(again[t], res.renders[t]) for t in again)
    assert sorted(os.listdir(str(tmp_path / 'ro'))) == ['renderonly_test_000007', 'renderonly_train_000007', 'renderonly_val_000007']
    assert sorted(os.listdir(str(tmp_path / 'ro' / 'renderonly_train_000007'))) == ['000.png', '001.png', '002.png']
    # a found checkpoint: the README's "delete the .tar files"
    d = os.path.join(args.basedir, args.expname)
    os.makedirs(d, exist_ok=True)
    rkt = res.render_kwargs_train
    torch.save({'global_step': 2, 'network_fn_state_dict': rkt['network_fn'].state_dict(),
                'network_fine_state_dict': rkt['network_fine'].state_dict(), 'optimizer_state_dict': res.optimizer.state_dict()},
               os.path.join(d, '000002.tar'))
    with pytest.raises(ValueError, match='000002.tar'):
        poisoned_retrain(poisoned.sink, scene.poses, scene.i_split, scene.hwf, scene.K, args, N_iters=5, log=None)      # (the default make_nerf)
    cont = poisoned_retrain(poisoned.sink, scene.poses, scene.i_split, scene.hwf, scene.K, args, N_iters=5, eval_tags=(), log=None, resume=True)
    assert cont.attempts == 1 and cont.last_iteration == 4 and [l[0] for l in cont.logged] == [4]
    assert RN.create_nerf(args)[2] == 2                                    # (nothing was written at i_weights = 1000)
