"""The NeRF training loop of the reference (run_nerf.py = RN, lines 690-816) on the HIP path, with the front of the step on the
device: `RayBatcher` keeps the training images and poses resident and turns (step, N_rand) into packed rays and target
colours with ONE launch (nerfail_train_batch) - no host permutation, no per-step image upload, no full-image get_rays - and
`train()` runs RN:726-816 without a host wait between log points: loss and PSNR stay in a device ring until `i_print` or a
checkpoint reads them.

The batch of a step is drawn by the keyed index shuffle of include/nerfail_hip.h (ABI 13): the first N_rand values of a
permutation of one view's window (no_batching, RN:744-773), or successive ranges of a permutation of every training pixel
(use_batching, RN:690-742). That is the distribution of the reference's np.random.choice / np.random.shuffle draws, not their
bits: no seed parity with the reference is claimed. `load_blender.train_step` stays the literal RN:746-801 step.

Under torch.distributed with more than one rank `train()` is data-parallel: the N_rand rays of a step are split over the
ranks (a rank's shard is another `first` and `n` of the same permutation), every rank runs the same forward and backward on
its rays with the loss divided by the GLOBAL count, ONE all-reduce per step sums a flat arena of every parameter gradient
plus the loss and mse (_train.GradArena), and every rank applies the identical Adam step."""
import os

import numpy as np
import torch

from . import _lib, ops  # noqa: F401  (ops registers torch.ops.nerfail_mi.*)
from . import run_nerf as RN
from . import sharding
from ._train import GradArena
from .optim import decayed_lrate
from .run_nerf_helpers import img2mse, _cuda

RING = 256          # steps of (loss, mse) kept on the device between two reads


def precrop_window(H, W, frac):
    """(row0, col0, wh, ww) of the centre crop RN:754-761; frac None: the full image."""
    if frac is None:
        return 0, 0, int(H), int(W)
    dH, dW = int(H // 2 * frac), int(W // 2 * frac)
    return H // 2 - dH, W // 2 - dW, 2 * dH, 2 * dW


def _host(a):
    return a.detach().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))


class RayBatcher:
    """Training rays from resident data. `images` is the [N,H,W,3] array load_blender.training_images() returns and `poses`
    [N,3+,4]; the views `i_train` are uploaded once (float32, as RN:748 / RN:752 convert them per step)."""

    def __init__(self, images, poses, i_train, hwf, K, near, far, seed=0, rng=None, device=None):
        self._setup(_cuda() if device is None else torch.device(device), poses, i_train, hwf, K, near, far, seed, rng)
        n = len(self.i_train)
        self.images = torch.empty((n, self.H, self.W, 3), dtype=torch.float32, device=self.dev)
        for s, v in enumerate(self.i_train):             # one view at a time: no second host copy of the whole set
            img = _host(images[v])
            if tuple(img.shape) != (self.H, self.W, 3):
                raise ValueError('RayBatcher: image %d is %s, expected (%d, %d, 3) - RGBA goes through training_images() first'
                                 % (v, tuple(img.shape), self.H, self.W))
            self.images[s].copy_(img.to(torch.float32))

    def _setup(self, dev, poses, i_train, hwf, K, near, far, seed, rng):
        """Everything but the image store."""
        self.dev = dev
        self.H, self.W = int(hwf[0]), int(hwf[1])
        self.K4 = [float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])]
        self.near, self.far = float(near), float(far)
        self.i_train = [int(i) for i in i_train]
        if not self.i_train:
            raise ValueError('RayBatcher: i_train is empty')
        self.slot_of = {v: s for s, v in enumerate(self.i_train)}
        n = len(self.i_train)
        p = _host(poses).to(torch.float32)[self.i_train, :3, :4].reshape(n, 12)
        self.poses = p.contiguous().to(self.dev)
        self.seed = int(seed) & 0xFFFFFFFF
        self.rng = np.random.RandomState(self.seed) if rng is None else rng       # draws the view of a no_batching step (RN:746)
        self.epoch, self.i_batch = 0, 0                  # use_batching: RN:707, advanced as RN:737-742
        self.n_global = 0                                # rays of the last batch over ALL ranks (the loss's denominator)

    @classmethod
    def from_resident(cls, store, poses, i_train, hwf, K, near, far, seed=0, rng=None):
        """A batcher over a store that already lives on the device: `store` float32 [n,H,W,3], slot s holding view i_train[s]
        (retrain.PoisonedTrainSet.images). The tensor is adopted as it is: no copy, no upload."""
        self = cls.__new__(cls)
        if not isinstance(store, torch.Tensor) or not store.is_cuda or store.dtype != torch.float32 or not store.is_contiguous():
            raise ValueError('RayBatcher.from_resident: store must be a contiguous float32 tensor on the device')
        self._setup(store.device, poses, i_train, hwf, K, near, far, seed, rng)
        if tuple(store.shape) != (len(self.i_train), self.H, self.W, 3):
            raise ValueError('RayBatcher.from_resident: store is %s, expected (%d, %d, %d, 3): one slot per view of i_train'
                             % (tuple(store.shape), len(self.i_train), self.H, self.W))
        self.images = store
        return self

    def key(self, counter):
        return ops.as_op_key((self.seed << 32) | (int(counter) & 0xFFFFFFFF))

    def _launch(self, window, view0, n_views, sel, key, first, n, return_sel):
        if n == 0:                                       # an empty shard: no launch
            rays, target = (torch.empty((0, k), dtype=torch.float32, device=self.dev) for k in (_lib.RAY_FLOATS, 3))
            return (rays, target, torch.empty((0,), dtype=torch.int64, device=self.dev)) if return_sel else (rays, target)
        rays, target, sel_out = torch.ops.nerfail_mi.train_batch(self.poses, self.images, None, sel, self.H, self.W, self.K4, self.near,
                                                                 self.far, list(window), view0, n_views, key, first, n, return_sel)
        return (rays, target, sel_out) if return_sel else (rays, target)

    def batch(self, global_step, N_rand, precrop=None, use_batching=False, view=None, sel=None, return_sel=False, rank=0, world=1):
        """(rays [n,11], target [n,3]) of one step - plus the population indices [n] with return_sel.
        use_batching False: one view (drawn with rng.choice(i_train) unless `view` names it), n = min(N_rand, window) distinct
        pixels of its window (`precrop`: the fraction of RN:754-761, None = full image), permutation key (seed << 32) | global_step.
        use_batching True: positions [i_batch, i_batch + N_rand) of the permutation (seed << 32) | epoch of all training
        pixels (full images, as RN:690-742 has no precrop); the last batch of an epoch is short, then the epoch advances.
        sel (with view): explicit int64 indices into the view's window instead of drawn ones.
        rank / world: this rank's rows [lo, hi) = sharding.shard_range(n, rank, world) of that batch - the same permutation
        from `first + lo` on, so the ranks' shards concatenate to the 1-rank batch. The bookkeeping (view draw, i_batch, epoch)
        advances by the global n on every rank; `n_global` holds it."""
        if sel is not None or view is not None or not use_batching:
            window = precrop_window(self.H, self.W, precrop)
            v = int(self.rng.choice(self.i_train)) if view is None else int(view)
            if v not in self.slot_of:
                raise ValueError('RayBatcher: view %d is not one of i_train' % v)
            if sel is not None:
                sel = torch.as_tensor(sel, dtype=torch.int64).to(self.dev)
                self.n_global = int(sel.shape[0])
                lo, hi = sharding.shard_range(self.n_global, rank, world)
                return self._launch(window, self.slot_of[v], 1, sel[lo:hi].contiguous(), 0, 0, hi - lo, return_sel)
            n = self.n_global = min(int(N_rand), window[2] * window[3])
            lo, hi = sharding.shard_range(n, rank, world)
            return self._launch(window, self.slot_of[v], 1, None, self.key(global_step), lo, hi - lo, return_sel)
        window = precrop_window(self.H, self.W, None)
        m = len(self.i_train) * self.H * self.W
        n = self.n_global = min(int(N_rand), m - self.i_batch)
        lo, hi = sharding.shard_range(n, rank, world)
        out = self._launch(window, 0, len(self.i_train), None, self.key(self.epoch), self.i_batch + lo, hi - lo, return_sel)
        self.i_batch += n
        if self.i_batch >= m:                            # RN:738-742: a new order for the next epoch
            self.epoch, self.i_batch = self.epoch + 1, 0
        return out


def _render_kwargs(render_kwargs_train):
    kw = dict(render_kwargs_train)
    if kw.pop('ndc', False):
        raise NotImplementedError('ndc=True is LLFF-only (RN:112-114); the blender configs pass ndc=False')
    if not kw.pop('use_viewdirs', False):
        raise NotImplementedError('HIP path implements use_viewdirs=True (all configs/*.txt)')
    kw.pop('near', None), kw.pop('far', None)            # (already in the packed rays)
    return kw


class LossRing:
    """(loss, mse) of the last RING steps on the device: one small launch per step, read by the host only when asked."""

    def __init__(self, device, size=RING):
        self.buf = torch.zeros((size, 2), dtype=torch.float32, device=device)
        self.size = size

    def put(self, i, loss, mse):
        torch.stack((loss.detach(), mse.detach()), out=self.buf[i % self.size])

    def read(self, i):
        """(loss, psnr) of step i as floats: THE host wait of the loop. psnr = mse2psnr (RH:10) of the fine image loss."""
        loss, mse = self.buf[i % self.size].cpu()
        psnr = -10. * torch.log(mse) / torch.log(torch.Tensor([10.]))
        return float(loss), float(psnr)


def param_checksum(params):
    """int64 [1] on the parameters' device: the wrapping sum of every parameter's bits, each element weighted by its position
    in its tensor + 1 (so that swapped values do not cancel). Equal parameters give equal checksums on every rank."""
    total = None
    for p in params:
        bits = p.detach().reshape(-1).view(torch.int32).to(torch.int64)
        c = (bits * torch.arange(1, bits.numel() + 1, dtype=torch.int64, device=bits.device)).sum()
        total = c if total is None else total + c
    return total.reshape(1)


def check_ranks_agree(params, group=None):
    """Raise unless every rank holds the same parameter bits: a MIN and a MAX all-reduce of param_checksum. A log-point
    check (it waits for the device)."""
    c = param_checksum(params)
    lo, hi = c.clone(), c.clone()
    sharding.all_reduce_(lo, torch.distributed.ReduceOp.MIN, group)
    sharding.all_reduce_(hi, torch.distributed.ReduceOp.MAX, group)
    lo, hi, c = int(lo), int(hi), int(c)
    if lo != hi:
        raise RuntimeError('train: the ranks\' parameters have diverged (checksum %d here, min %d, max %d over the ranks)' % (c, lo, hi))
    return c


def _sync_ranks(params, optimizer, rank, group):
    """Before the first data-parallel step: rank 0's parameters - and, on resume, its Adam state - on every rank; then the
    device RNG of rank r > 0 moves to a stream of its own, so that stratified and noise draws differ between the ranks."""
    for p in params:
        sharding.broadcast_(p.data, 0, group)
        torch.autograd.graph.increment_version(p)        # (the weight images are keyed on it)
    has = torch.tensor([sum(1 for p in params if len(optimizer.state.get(p, {})) > 0)], dtype=torch.int64,
                       device=params[0].device)
    sharding.broadcast_(has, 0, group)
    if int(has) > 0:                                      # a resumed run: rank 0's moments and step counts
        for p in params:
            st = optimizer.state[p]
            if len(st) == 0:
                st['step'] = torch.tensor(0.0, dtype=torch.float32)
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            sharding.broadcast_(st['exp_avg'], 0, group)
            sharding.broadcast_(st['exp_avg_sq'], 0, group)
            step = st['step'].detach().to(device=p.device, dtype=torch.float32).reshape(1).contiguous()
            sharding.broadcast_(step, 0, group)
            st['step'] = step.reshape(()).cpu() if not st['step'].is_cuda else step.reshape(())
    if rank > 0 and params[0].is_cuda:
        gen = torch.cuda.default_generators[params[0].device.index]
        gen.manual_seed((gen.initial_seed() + 0x9E3779B97F4A7C15 * rank) % (1 << 63))


def train(images, poses, i_split, hwf, K, args, render_kwargs_train, optimizer, start, near=2., far=6., seed=0, N_iters=None,
          batcher=None, log=print, group=None, timing=None):
    """RN:726-816: the optimisation loop from iteration start + 1 to N_iters - 1 (RN:717: 200 000 + 1 unless args.N_iters /
    N_iters say otherwise). Per step: batch (RayBatcher, args.no_batching / N_rand / precrop_iters / precrop_frac) ->
    render_rays on the packed rays -> mse(rgb) + mse(rgb0) -> backward -> optimizer.step() -> decayed_lrate. Every
    args.i_weights iterations a checkpoint basedir/expname/{:06d}.tar with the four keys of RN:810-815 (create_nerf reloads
    it; 'global_step' is the number of finished iterations, so a reload resumes behind the saved one); every args.i_print
    iterations one log line. Nothing between those points waits for the GPU. i_video / i_testset rendering is the caller's
    (render_path). `batcher`: a RayBatcher (or anything with its batch()) to bring your own sampler.
    With a torch.distributed process group of more than one rank (`group`: which; None = the default group) the run is
    data-parallel: N_rand stays the GLOBAL batch, each rank trains on its shard of it, one all-reduce per step carries all
    parameter gradients + (loss, mse), every rank steps identically. Parameters (and Adam's state on resume) are rank 0's;
    checkpoints and log lines come from rank 0 (`logged` is returned on every rank); at each log point the ranks compare a
    checksum of their parameters and raise if they differ. One rank: today's loop, no collective (NERFAIL_FORCE_COLLECTIVE=1
    issues it all the same: the 1-rank dry run). `timing`: a dict that gets HIP events around each step's all-reduce.
    Returns (last iteration, [(iteration, loss, psnr) at every log point])."""
    i_train = i_split[0] if isinstance(i_split, (list, tuple)) else i_split
    H, W = int(hwf[0]), int(hwf[1])
    if batcher is None:
        batcher = RayBatcher(images, poses, i_train, hwf, K, near, far, seed=seed)
    kw = _render_kwargs(render_kwargs_train)
    use_batching = not getattr(args, 'no_batching', False)     # RN:692 (the blender configs set no_batching)
    N_rand, chunk = int(args.N_rand), int(getattr(args, 'chunk', 1024 * 32))
    precrop_iters, precrop_frac = int(getattr(args, 'precrop_iters', 0)), float(getattr(args, 'precrop_frac', .5))
    i_print, i_weights = int(getattr(args, 'i_print', 100)), int(getattr(args, 'i_weights', 10000))
    if N_iters is None:
        N_iters = int(getattr(args, 'N_iters', 200000)) + 1
    ring = LossRing(batcher.images.device)
    logged = []
    world, rank = sharding.world_and_rank(group)
    arena = None
    if world > 1 or (sharding.force_collectives() and torch.distributed.is_available() and torch.distributed.is_initialized()):
        params = [p for g in optimizer.param_groups for p in g['params']]
        arena = GradArena([render_kwargs_train['network_fn'], render_kwargs_train.get('network_fine')])
        if sorted(id(p) for n in arena.nets for p in n.ordered_params()) != sorted(id(p) for p in params):
            raise ValueError('train: the optimizer must hold exactly the parameters of network_fn and network_fine')
        _sync_ranks(params, optimizer, rank, group)
        kw['grad_arena'] = arena
        if rank != 0:
            log = lambda s: None                                 # noqa: E731  (rank 0 speaks)
    global_step = start                                  # RN:657
    i = start
    for i in range(start + 1, N_iters):
        precrop = precrop_frac if (not use_batching and i < precrop_iters) else None
        if precrop is not None and i == start + 1:
            w = precrop_window(H, W, precrop)
            log('[Config] Center cropping of size %d x %d is enabled until iter %d' % (w[2], w[3], precrop_iters))
        if arena is None:
            rays, target_s = batcher.batch(global_step, N_rand, precrop=precrop, use_batching=use_batching)
            n_total = None
        else:
            rays, target_s = batcher.batch(global_step, N_rand, precrop=precrop, use_batching=use_batching, rank=rank, world=world)
            n_total = 3 * int(getattr(batcher, 'n_global', N_rand))
        optimizer.zero_grad()
        if rays.shape[0] > 0:
            if rays.shape[0] <= chunk:
                ret = RN.render_rays(rays, retraw=True, **kw)
            else:                                                # several backward passes: they cannot share the arena
                ret = RN.batchify_rays(rays, chunk, retraw=True, **dict(kw, grad_arena=None))
            img_loss = img2mse(ret['rgb_map'], target_s, n_total)
            loss = img_loss
            if 'rgb0' in ret:
                loss = loss + img2mse(ret['rgb0'], target_s, n_total)
            loss.backward()
            if arena is not None:
                arena.put_tail(loss, img_loss)
        elif arena is None:
            raise ValueError('train: the batch of iteration %d is empty' % i)
        else:                                                    # an idle rank: zeros into the sum, and the same step as everyone
            arena.zero_()
        if arena is not None:
            arena.adopt()
            arena.reduce_(group, timing)
            loss, img_loss = arena.loss, arena.mse
        optimizer.step()
        new_lrate = decayed_lrate(args.lrate, global_step, args.lrate_decay)         # RN:796-800
        for param_group in optimizer.param_groups:
            param_group['lr'] = new_lrate
        ring.put(i, loss, img_loss)
        global_step += 1
        if i % i_weights == 0 and rank == 0:
            d = os.path.join(args.basedir, args.expname)
            os.makedirs(d, exist_ok=True)
            path = os.path.join(d, '{:06d}.tar'.format(i))
            fine = render_kwargs_train.get('network_fine')
            torch.save({'global_step': global_step,
                        'network_fn_state_dict': render_kwargs_train['network_fn'].state_dict(),
                        'network_fine_state_dict': fine.state_dict() if fine is not None else None,
                        'optimizer_state_dict': optimizer.state_dict()}, path)
            log('Saved checkpoints at %s' % path)
        if i % i_print == 0:
            if arena is not None:
                check_ranks_agree(params, group)
            l, p = ring.read(i)
            logged.append((i, l, p))
            log('[TRAIN] Iter: %d Loss: %s  PSNR: %s' % (i, l, p))
    return i, logged
