"""-m gpu: the device-side training batch (ABI 13) and the loop built on it (nerfail_amd/train.py).

  * nerfail_index_shuffle against the numpy restatement (tests/batch_ref.py), bit for bit;
  * nerfail_train_batch: rays equal to nerfail_ray_gen's rows and targets equal to the image pixels, explicit and drawn batches;
  * train(): three steps equal to three steps of load_blender.train_step fed the same views and pixels - every loss and every
    parameter, bit for bit -, epochs over all training pixels, the checkpoint round trip through create_nerf, no host wait
    between log points, and opcheck on both ops."""
import os
import types

import numpy as np
import pytest
import torch

import batch_ref as B
import synth
from hiputil import T, N, dev, hip_nerf

pytestmark = pytest.mark.gpu

MS = (1, 2, 3, 5, 16, 17, 100, 1023, 1025, 4097)
KEYS = (0, 0x9E3779B9, (7 << 32) | 123456)
NEAR, FAR = 2., 6.


def _ops():
    import nerfail_amd.ops as O
    return O, torch.ops.nerfail_mi


# ---------------------------------------------------------------------------------------------- the shuffle
def test_index_shuffle_matches_the_restatement():
    O, ops = _ops()
    anchor = torch.empty(1, device=dev())
    for m in MS:
        n = max(1, m // 2)
        for key in KEYS:
            for first in sorted({0, 1, m - n}):
                if first + n > m:
                    continue
                got = ops.index_shuffle(anchor, O.as_op_key(key), m, first, n)
                assert got.dtype == torch.int64 and np.array_equal(N(got), B.shuffle(key, m, first, n)), (m, key, first)
            assert np.array_equal(N(ops.index_shuffle(anchor, O.as_op_key(key), m, 0, m)), B.shuffle(key, m))
    # the widest network (2 x 16 bits), indices up to 2^31 - 1, a key with the top bit set
    m, n, key = 1 << 31, 1000, (0xFEDCBA98 << 32) | 0x76543210
    got = N(ops.index_shuffle(anchor, O.as_op_key(key), m, m - n, n))
    assert np.array_equal(got, B.shuffle(key, m, m - n, n)) and got.min() >= 0 and got.max() < m and len(np.unique(got)) == n
    assert ops.index_shuffle(anchor, 3, 10, 10, 0).shape == (0,)


# ---------------------------------------------------------------------------------------------- rays and targets
class Toy:
    """H = 5, W = 7 (not square: a row / column swap shows), three views with distinct poses, slots -> views [2, 0]."""
    H, W = 5, 7
    VIEW_IDS = [2, 0]

    def __init__(self):
        from nerfail_amd.run_nerf import ray_gen
        rs = np.random.RandomState(11)
        self.K = np.array([[9.5, 0, 0.5 * self.W], [0, 9.5, 0.5 * self.H], [0, 0, 1]])
        self.K4 = [float(self.K[0, 0]), float(self.K[1, 1]), float(self.K[0, 2]), float(self.K[1, 2])]
        self.poses_np = np.stack([synth.pose_spherical(37. * i - 50., -30. + 7. * i, 4. + .25 * i) for i in range(3)])
        self.poses = T(self.poses_np[:, :3, :4].reshape(3, 12).astype(np.float32))
        self.images = T(rs.uniform(size=(3, self.H, self.W, 3)).astype(np.float32))
        self.view_ids = torch.tensor(self.VIEW_IDS, dtype=torch.int32, device=dev())
        self.ref_rays = [ray_gen(self.H, self.W, self.K, torch.from_numpy(p[:3, :4]), NEAR, FAR) for p in self.poses_np]

    def expect(self, q, window):
        view, row, col = B.population(q, window[2], window[3], window[0], window[1], view_ids=self.VIEW_IDS)
        v, r, c = (torch.from_numpy(a).to(dev()) for a in (view, row, col))
        rays = torch.stack(self.ref_rays)[v, r * self.W + c]
        return rays, self.images[v, r, c]

    def run(self, window, sel=None, key=0, first=0, n=None, images=True, want_sel=False):
        _, ops = _ops()
        n = int(sel.shape[0]) if sel is not None else n
        return ops.train_batch(self.poses, self.images if images else None, self.view_ids, sel, self.H, self.W, self.K4, NEAR, FAR,
                               list(window), 0, 2, key, first, n, want_sel)


@pytest.fixture(scope='module')
def toy():
    return Toy()


@pytest.mark.parametrize('window,n', [((0, 0, 5, 7), 1), ((0, 0, 5, 7), 63), ((0, 0, 5, 7), 70), ((1, 2, 2, 4), 1), ((1, 2, 2, 4), 16)])
def test_train_batch_explicit_indices(toy, window, n):
    m = 2 * window[2] * window[3]
    q = np.random.RandomState(n).permutation(m)[:n]
    want_rays, want_target = toy.expect(q, window)
    rays, target, sel_out = toy.run(window, sel=T(q.astype(np.int64)), want_sel=True)
    assert tuple(rays.shape) == (n, 11) and torch.equal(rays, want_rays)
    assert tuple(target.shape) == (n, 3) and torch.equal(target, want_target)
    assert np.array_equal(N(sel_out), q)
    rays2, target2, sel2 = toy.run(window, sel=T(q.astype(np.int64)), images=False)        # images = NULL: rays only
    assert torch.equal(rays2, want_rays) and target2.numel() == 0 and sel2.numel() == 0


def test_train_batch_drawn_equals_explicit(toy):
    O, ops = _ops()
    for window, first, n in (((0, 0, 5, 7), 3, 40), ((0, 0, 5, 7), 0, 70), ((1, 2, 2, 4), 5, 11)):
        m = 2 * window[2] * window[3]
        key = O.as_op_key((5 << 32) | 77)
        sel = ops.index_shuffle(toy.poses, key, m, first, n)
        assert np.array_equal(N(sel), B.shuffle((5 << 32) | 77, m, first, n))
        rays_e, target_e, _ = toy.run(window, sel=sel)
        rays_d, target_d, sel_d = toy.run(window, key=key, first=first, n=n, want_sel=True)
        assert torch.equal(sel_d, sel) and torch.equal(rays_d, rays_e) and torch.equal(target_d, target_e)
        want_rays, want_target = toy.expect(N(sel), window)
        assert torch.equal(rays_d, want_rays) and torch.equal(target_d, want_target)


def test_raybatcher_at_800x800_with_precrop():
    from nerfail_amd.run_nerf import ray_gen
    from nerfail_amd.train import RayBatcher, precrop_window
    Hh = Ww = 800
    focal, K = synth.lego_intrinsics(Hh, Ww)
    pose = synth.pose_spherical(30., -30., 4.)
    img = torch.rand((1, Hh, Ww, 3), device=dev())
    rb = RayBatcher(img, pose[None], [0], [Hh, Ww, focal], K, NEAR, FAR, seed=3)
    window = precrop_window(Hh, Ww, .5)
    assert window == (200, 200, 400, 400)
    rays, target, sel = rb.batch(17, 1024, precrop=.5, return_sel=True)
    q = N(sel)
    assert q.shape == (1024,) and len(np.unique(q)) == 1024 and q.min() >= 0 and q.max() < 400 * 400
    assert np.array_equal(q, B.shuffle((3 << 32) | 17, 400 * 400, 0, 1024))
    _, row, col = B.population(q, 400, 400, 200, 200)
    assert row.min() >= 200 and row.max() < 600 and col.min() >= 200 and col.max() < 600
    pix = torch.from_numpy(row * Ww + col).to(dev())
    assert torch.equal(rays, ray_gen(Hh, Ww, K, torch.from_numpy(pose[:3, :4]), NEAR, FAR)[pix])
    assert torch.equal(target, img[0].reshape(-1, 3)[pix])
    rays_full, _, sel_full = rb.batch(17, 1024, return_sel=True)                             # the full image, same key
    assert np.array_equal(N(sel_full), B.shuffle((3 << 32) | 17, Hh * Ww, 0, 1024)) and len(np.unique(N(sel_full))) == 1024


# ---------------------------------------------------------------------------------------------- the loop
def _kwargs(coarse, fine, n_samples=16, n_importance=16):
    return {'network_query_fn': None, 'perturb': 1., 'N_importance': n_importance, 'network_fine': fine, 'N_samples': n_samples,
            'network_fn': coarse, 'use_viewdirs': True, 'white_bkgd': True, 'raw_noise_std': 0., 'ndc': False, 'lindisp': False}


def _loop_args(basedir, **kw):
    a = dict(N_rand=64, no_batching=True, lrate=5e-4, lrate_decay=250, i_print=1, i_weights=10 ** 9, precrop_iters=0, precrop_frac=.5,
             chunk=1024 * 32, basedir=basedir, expname='toy')
    a.update(kw)
    return types.SimpleNamespace(**a)


class Recording:
    """np.random.RandomState that keeps what choice() returned: view, pixels, view, pixels, ..."""

    def __init__(self, seed):
        self.rs, self.calls = np.random.RandomState(seed), []

    def choice(self, *a, **k):
        r = self.rs.choice(*a, **k)
        self.calls.append(r)
        return r


def test_loop_equals_train_step_bit_for_bit(tmp_path):
    """Three steps of load_blender.train_step (host permutation, image upload, get_rays of the full image, gathers) and three
    steps of train() fed the same views and pixels, from the same weights and the same torch seed: D8 W256 coarse + fine
    (deterministic weight-gradient kernel), 16 + 16 samples, 64 rays. Every loss and every parameter is equal."""
    from test_load_blender import write_toy_scene
    from nerfail_amd.load_blender import load_blender_data, training_images, train_step
    from nerfail_amd.optim import Adam
    from nerfail_amd.train import RayBatcher, train
    root = str(tmp_path / 'scene')
    write_toy_scene(root, H=16, W=16, n=(3, 2, 2), seed=3)
    images, poses, _, hwf, i_split = load_blender_data(root)
    Hh, Ww, focal = hwf
    K = np.array([[focal, 0, 0.5 * Ww], [0, focal, 0.5 * Hh], [0, 0, 1]])
    imgs = training_images(images, white_bkgd=True)

    def setup():
        nets = [hip_nerf(seed=s, requires_grad=True)[1] for s in (41, 42)]
        opt = Adam([p for n_ in nets for p in n_.parameters()], lr=5e-4, betas=(0.9, 0.999))
        return nets, opt, _kwargs(*nets)

    nets_a, opt_a, kw_a = setup()
    rec = Recording(0)
    torch.manual_seed(5)
    losses_a = [train_step(imgs, poses, i_split[0], hwf, K, kw_a, opt_a, step, N_rand=64, lrate=5e-4, lrate_decay=250,
                           near=NEAR, far=FAR, rng=rec)[0] for step in range(3)]
    assert len(rec.calls) == 6

    nets_b, opt_b, kw_b = setup()

    class Replay(RayBatcher):
        def batch(self, global_step, N_rand, precrop=None, use_batching=False):
            view, pixels = rec.calls[2 * global_step], rec.calls[2 * global_step + 1]
            return RayBatcher.batch(self, global_step, N_rand, precrop=precrop, view=int(view), sel=pixels)

    torch.manual_seed(5)
    last, logged = train(imgs, poses, i_split, hwf, K, _loop_args(str(tmp_path)), kw_b, opt_b, 0, near=NEAR, far=FAR, N_iters=4,
                         batcher=Replay(imgs, poses, i_split[0], hwf, K, NEAR, FAR), log=lambda s: None)
    assert last == 3 and [it for it, _, _ in logged] == [1, 2, 3]
    losses_b = [l for _, l, _ in logged]
    print('train_step losses', losses_a, 'train() losses', losses_b)
    assert all(np.isfinite(losses_a)) and losses_b == losses_a
    for na, nb in zip(nets_a, nets_b):
        for (name, pa), pb in zip(na.named_parameters(), nb.parameters()):
            assert torch.equal(pa, pb), name
    assert not torch.equal(nets_a[0].pts_linears[0].weight, hip_nerf(seed=41)[1].pts_linears[0].weight)     # (they did move)
    assert opt_a.param_groups[0]['lr'] == opt_b.param_groups[0]['lr']


def _small_scene(H, W, n_views, seed=0):
    rs = np.random.RandomState(seed)
    images = rs.uniform(size=(n_views, H, W, 3)).astype(np.float32)
    poses = np.stack([synth.pose_spherical(40. * i, -30., 4.) for i in range(n_views)])
    focal = .5 * W / np.tan(.5 * synth.LEGO_CAMERA_ANGLE_X)
    return images, poses, [H, W, focal], np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])


def test_epoch_mode_covers_every_pixel_once():
    from nerfail_amd.run_nerf import ray_gen
    from nerfail_amd.train import RayBatcher
    images, poses, hwf, K = _small_scene(4, 6, 3)
    rb = RayBatcher(images, poses, [2, 0], hwf, K, NEAR, FAR, seed=9)          # 2 training views x 4 x 6 = 48 pixels
    epochs = []
    for e in range(2):
        sizes, sels = [], []
        for _ in range(3):
            assert rb.epoch == e
            rays, target, sel = rb.batch(0, 20, use_batching=True, return_sel=True)
            sizes.append(rays.shape[0])
            sels.append(N(sel))
            view, row, col = B.population(sels[-1], 4, 6, view_ids=[2, 0])
            assert np.array_equal(N(target), images[view, row, col])
            for v in (2, 0):
                want = ray_gen(4, 6, K, torch.from_numpy(poses[v, :3, :4]), NEAR, FAR)
                pick = view == v
                assert torch.equal(rays[torch.from_numpy(pick).to(dev())], want[torch.from_numpy((row * 6 + col)[pick]).to(dev())])
        assert sizes == [20, 20, 8]
        epochs.append(np.concatenate(sels))
        assert np.array_equal(np.sort(epochs[-1]), np.arange(48))
        assert np.array_equal(epochs[-1], B.shuffle((9 << 32) | e, 48))
    assert rb.epoch == 2 and rb.i_batch == 0 and not np.array_equal(epochs[0], epochs[1])


def _create_args(basedir):
    return types.SimpleNamespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=16, N_samples=16,
                                 netdepth=4, netwidth=64, netdepth_fine=4, netwidth_fine=64, netchunk=65536, lrate=5e-4,
                                 basedir=basedir, expname='toy', ft_path=None, no_reload=False, perturb=1., white_bkgd=True,
                                 raw_noise_std=0., dataset_type='blender', no_ndc=False, lindisp=False, N_rand=64, no_batching=True,
                                 lrate_decay=250, i_print=1000, i_weights=2, precrop_iters=2, precrop_frac=.5, chunk=1024 * 32)


def test_checkpoint_round_trip(tmp_path):
    from nerfail_amd import run_nerf as RN
    from nerfail_amd.train import train
    images, poses, hwf, K = _small_scene(16, 16, 3, seed=1)
    args = _create_args(str(tmp_path))
    torch.manual_seed(1)
    kw, _, start, grad_vars, opt = RN.create_nerf(args)
    assert start == 0
    with torch.no_grad():
        for net in (kw['network_fn'], kw['network_fine']):
            net.alpha_linear.bias += 0.5                 # (a fresh NeRF has no density: the nudge the other toy tests use)
    w0 = grad_vars[0].detach().clone()
    lines = []
    last, logged = train(images, poses, [[0, 1, 2], [], []], hwf, K, args, kw, opt, start, near=NEAR, far=FAR, N_iters=3, log=lines.append)
    assert last == 2 and logged == [] and any('Saved checkpoints' in s for s in lines)
    assert any('Center cropping of size 8 x 8' in s for s in lines)          # iteration 1 < precrop_iters: its 64 rays are the whole crop
    path = os.path.join(str(tmp_path), 'toy', '000002.tar')
    ckpt = torch.load(path, map_location='cpu')
    assert set(ckpt) == {'global_step', 'network_fn_state_dict', 'network_fine_state_dict', 'optimizer_state_dict'}
    assert ckpt['global_step'] == 2 and not torch.equal(grad_vars[0].detach(), w0)
    kw2, _, start2, grad_vars2, opt2 = RN.create_nerf(args)
    assert start2 == 2
    for a, b in zip(grad_vars, grad_vars2):
        assert torch.equal(a.detach(), b.detach())
    for a, b in zip(grad_vars, grad_vars2):
        assert torch.equal(opt.state[a]['exp_avg'], opt2.state[b]['exp_avg']) and float(opt2.state[b]['step']) == 2.


def _sync_mode_works():
    """Does this torch build raise on a host wait under set_sync_debug_mode('error')?"""
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


def test_no_host_wait_between_log_points(tmp_path, monkeypatch):
    from nerfail_amd.optim import Adam
    from nerfail_amd.train import RayBatcher, train
    images, poses, hwf, K = _small_scene(16, 16, 3, seed=2)
    nets = [hip_nerf(seed=s, requires_grad=True)[1] for s in (43, 44)]
    opt = Adam([p for n_ in nets for p in n_.parameters()], lr=5e-4, betas=(0.9, 0.999))
    kw = _kwargs(*nets)
    args = _loop_args(str(tmp_path), i_print=1000)
    rb = RayBatcher(images, poses, [0, 1, 2], hwf, K, NEAR, FAR, seed=4)
    quiet = lambda s: None                                                               # noqa: E731
    train(images, poses, [[0, 1, 2]], hwf, K, args, kw, opt, 0, N_iters=2, batcher=rb, log=quiet)    # first step: allocations, packs
    torch.cuda.synchronize()
    native = _sync_mode_works()
    print('set_sync_debug_mode("error") catches a host wait on this build:', native)
    prev = torch.cuda.get_sync_debug_mode()
    try:
        if native:
            torch.cuda.set_sync_debug_mode('error')
        else:
            orig = {name: getattr(torch.Tensor, name) for name in ('item', 'cpu', 'tolist')}

            def refuse(name):
                def f(self, *a, **k):
                    if self.is_cuda:
                        raise AssertionError('Tensor.%s on a device tensor between log points' % name)
                    return orig[name](self, *a, **k)
                return f
            for name in orig:
                monkeypatch.setattr(torch.Tensor, name, refuse(name))
        last, logged = train(images, poses, [[0, 1, 2]], hwf, K, args, kw, opt, 1, N_iters=7, batcher=rb, log=quiet)   # five steps
        epoch_args = _loop_args(str(tmp_path), i_print=1000, no_batching=False)                                     # and two of an epoch
        last2, _ = train(images, poses, [[0, 1, 2]], hwf, K, epoch_args, kw, opt, 6, N_iters=9, batcher=rb, log=quiet)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
        monkeypatch.undo()
    assert (last, logged, last2) == (6, [], 8)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for n_ in nets for p in n_.parameters())


def test_batch_ops_pass_opcheck(toy):
    O, ops = _ops()
    assert set(O.BATCH_OPS) == {'index_shuffle', 'train_batch'}
    tests = ('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_dynamic')
    sel = T(np.array([3, 69, 0, 35], np.int64))
    samples = {'index_shuffle': [(toy.poses, O.as_op_key((1 << 63) | 5), 1025, 7, 300)],
               'train_batch': [(toy.poses, toy.images, toy.view_ids, sel, toy.H, toy.W, toy.K4, NEAR, FAR, [0, 0, 5, 7], 0, 2, 0, 0, 4, True),
                               (toy.poses, None, None, None, toy.H, toy.W, toy.K4, NEAR, FAR, [1, 2, 2, 4], 1, 2, 12345, 2, 9, False)]}
    for name in O.BATCH_OPS:
        for args in samples[name]:
            res = torch.library.opcheck(getattr(ops, name).default, args, test_utils=tests)
            assert all(v == 'SUCCESS' for v in res.values()), (name, res)
