#!/usr/bin/env python3
"""One rank of the data-parallel TRAINING test (tests/test_hip_train_multirank.py). Started as a fresh process by
tests/mgpu/launcher.py with RANK / WORLD_SIZE / MASTER_* in the environment; every rank uses HIP device 0 (the test box has
one GPU), so the process group is gloo and sharding stages the gradient arena through pinned host memory. What runs is
nerfail_amd itself: fixture g7's training step on this rank's shard + the arena all-reduce, then train.train() - three steps,
an idle rank (N_rand = 1), a checkpoint and a resume from it.

    python tests/mgpu/train_rank.py OUTDIR          -> OUTDIR/train_w{world}_r{rank}.npz
"""
import datetime
import glob
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from mgpu import train_problem as TP  # noqa: E402


def main(out_dir):
    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    torch.cuda.set_device(0)
    if world > 1:                          # a short timeout: a dead peer ends the rest instead of holding them
        dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    from nerfail_amd import run_nerf as RN, sharding
    from nerfail_amd._train import GradArena, ordered_params
    from nerfail_amd.train import RayBatcher, train
    calls, real = [], dist.all_reduce

    def counted(t, *a, **k):               # every collective the product issues, by size
        calls.append(t.numel() * t.element_size())
        return real(t, *a, **k)
    dist.all_reduce = counted
    out = {}

    # ---- fixture g7's step, this rank's rows, ONE all-reduce of the arena
    g = TP.g7()
    for tag, D, W in TP.G7_TAGS:
        coarse, fine = TP.g7_nets(D, W)
        arena = GradArena([coarse, fine])
        R = g[tag + '_rays'].shape[0]
        lo, hi = sharding.shard_range(R, rank, world)
        del calls[:]
        TP.g7_shard_step(g, tag, coarse, fine, lo, hi, arena)
        out[tag + '_local'] = arena.buf.cpu().numpy()                    # this shard's arena, before the collective
        arena.reduce_()
        out[tag + '_arena'], out[tag + '_calls'], out[tag + '_P'] = arena.buf.cpu().numpy(), np.array(calls, np.int64), arena.P
        out[tag + '_aliased'] = all(arena.holds(p.grad) for n in (coarse, fine) for p in ordered_params(n))
        if world == 2:                     # the same two shards computed again in THIS process, arenas added on the device
            parts = []
            for lo2, hi2 in sharding.shard_ranges(R, 2):
                a2 = GradArena([coarse, fine])
                TP.g7_shard_step(g, tag, coarse, fine, lo2, hi2, a2)
                parts.append(a2.buf)
            out[tag + '_inproc_sum'] = (parts[0] + parts[1]).cpu().numpy()

    # ---- train(): STEPS iterations, a checkpoint after the last, every step a log point
    images, poses, hwf, K = TP.scene()
    i_split = [[0, 1, 2, 3], [], []]

    def run(tag, n_rand, seed, steps, start_from_ckpt=False, i_weights=10 ** 9):
        args = TP.create_args(os.path.join(out_dir, 'ckpt_w%d_%s' % (world, tag)), N_rand=n_rand, i_weights=i_weights)
        torch.manual_seed(seed + (0 if start_from_ckpt else rank))        # ranks START apart: train() makes them rank 0's
        kw, _, start, grad_vars, opt = RN.create_nerf(args)
        if not start_from_ckpt:
            assert start == 0
            TP.nudge_density(kw)
        params = [p for n in (kw['network_fn'], kw['network_fine']) for p in ordered_params(n)]
        rb = RayBatcher(images, poses, i_split[0], hwf, K, TP.NEAR, TP.FAR, seed=11)
        for _ in range(start):                                           # (a resumed sampler: the view draws already made)
            rb.rng.choice(rb.i_train)
        snaps, lines = [], []
        out[tag + '_params0'] = TP.flat(params)                          # what this rank starts from, before train() aligns the ranks

        def log(s):
            lines.append(s)
            if s.startswith('[TRAIN]'):
                snaps.append((TP.flat(params), TP.flat([p.grad for p in params])))
        del calls[:]
        quiet = world > 1 and rank > 0
        if quiet:                          # rank > 0 logs nothing: take the snapshots through the sampler instead, one step late
            class Tap:
                n_global, images = 0, rb.images

                def batch(self, *a, **k):
                    if params[0].grad is not None:
                        snaps.append((TP.flat(params), TP.flat([p.grad for p in params])))
                    o = rb.batch(*a, **k)
                    self.n_global = rb.n_global
                    return o
            sampler = Tap()
        else:
            sampler = rb
        last, logged = train(images, poses, i_split, hwf, K, args, kw, opt, start, near=TP.NEAR, far=TP.FAR, N_iters=start + steps + 1,
                             batcher=sampler, log=log)
        if quiet:
            snaps.append((TP.flat(params), TP.flat([p.grad for p in params])))
        assert last == start + steps and len(snaps) == steps, (last, len(snaps))
        out[tag + '_params'] = np.stack([s[0] for s in snaps])
        out[tag + '_grad1'] = snaps[0][1]
        out[tag + '_losses'] = np.array([l for _, l, _ in logged], np.float64)
        out[tag + '_psnr'] = np.array([p for _, _, p in logged], np.float64)
        out[tag + '_lines'] = len(lines)
        out[tag + '_calls'] = np.array(calls, np.int64)
        out[tag + '_P'] = sum(p.numel() for p in params)
        out[tag + '_adam'] = TP.flat([opt.state[p][k] for p in params for k in ('exp_avg', 'exp_avg_sq')])
        out[tag + '_adam_step'] = np.array([float(opt.state[p]['step']) for p in params])
        return args

    args = run('loop', 32, 1, TP.STEPS, i_weights=TP.STEPS)
    if world > 1:
        dist.barrier()
    out['ckpt_files'] = np.array(sorted(os.path.basename(f) for f in glob.glob(os.path.join(args.basedir, args.expname, '*.tar'))))
    if world <= 2:
        run('idle', 1, 3, 2)               # N_rand = 1: at world 2 rank 1 owns no ray, joins the sum and steps all the same
    # resume: every rank reloads rank 0's checkpoint through create_nerf and trains one more step
    os.makedirs(os.path.join(out_dir, 'ckpt_w%d_resume' % world, 'toy'), exist_ok=True)
    if rank == 0:
        import shutil
        shutil.copy(os.path.join(args.basedir, args.expname, '%06d.tar' % TP.STEPS), os.path.join(out_dir, 'ckpt_w%d_resume' % world, 'toy'))
    if world > 1:
        dist.barrier()
    run('resume', 32, 5, 1, start_from_ckpt=True)

    np.savez(os.path.join(out_dir, 'train_w%d_r%d.npz' % (world, rank)), **out)
    assert [l for l in open('/proc/self/maps') if 'libnerfail_hip' in l], 'libnerfail_hip.so is not mapped: the product path did not run'
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print('rank %d/%d ok' % (rank, world), flush=True)


if __name__ == '__main__':
    main(sys.argv[1])
