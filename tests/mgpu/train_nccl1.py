#!/usr/bin/env python3
"""RCCL dry run of data-parallel training on ONE GPU (tests/test_hip_train_multirank.py::test_rccl_path_one_rank_training):
a 1-rank process group with backend 'nccl' (= RCCL on ROCm) and NERFAIL_FORCE_COLLECTIVE=1, so that train.train() takes the
data-parallel path - gradient arena, loss share over the global count, the arena all-reduced on torch's current stream - with a
sum over one rank, the identity: the parameters must be those of the run without a process group, bit for bit (D8 W256
networks: their weight-gradient kernel adds in a fixed order, so two runs of one step agree to the bit at all). After the
first step (allocations, communicator creation) torch's sync debug mode is on for the rest of the loop: the RCCL path adds
no host wait between log points.

    python tests/mgpu/train_nccl1.py OUTDIR          -> OUTDIR/train_nccl1.npz
"""
import datetime
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from mgpu import train_problem as TP  # noqa: E402


def _sync_mode_works(dev):
    x = torch.ones(1, device=dev)
    torch.cuda.set_sync_debug_mode('error')
    try:
        x.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode('default')
    return False


_ORIG = {name: getattr(torch.Tensor, name) for name in ('item', 'cpu', 'tolist')}


def _refuse_host_reads(on):
    def refuse(name):
        def f(self, *a, **k):
            if self.is_cuda:
                raise AssertionError('Tensor.%s on a device tensor between log points' % name)
            return _ORIG[name](self, *a, **k)
        return f
    for name in _ORIG:
        setattr(torch.Tensor, name, refuse(name) if on else _ORIG[name])


def main(out_dir):
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29534')
    os.environ.pop('NERFAIL_FORCE_COLLECTIVE', None)
    from nerfail_amd.optim import Adam
    from nerfail_amd.train import RayBatcher, train
    from hiputil import hip_nerf
    images, poses, hwf, K = TP.scene()
    i_split = [[0, 1, 2, 3], [], []]
    native = _sync_mode_works(dev)

    class Guarded:
        """The sampler, switching the sync debug mode on at its first batch: from there to the end of train() is the loop."""

        def __init__(self, rb, on):
            self.rb, self.on, self.images, self.n_global = rb, on, rb.images, 0

        def batch(self, *a, **k):
            if self.on:
                torch.cuda.set_sync_debug_mode('error')
            else:                          # a build whose debug mode does not raise: refuse the host reads themselves
                _refuse_host_reads(True)
            o = self.rb.batch(*a, **k)
            self.n_global = self.rb.n_global
            return o

    def run(timing=None):
        nets = [hip_nerf(8, 256, s, requires_grad=True)[1] for s in (43, 44)]
        params = [p for n in nets for p in n.ordered_params()]
        opt = Adam(params, lr=5e-4, betas=(0.9, 0.999))
        kw = {'network_query_fn': None, 'perturb': 0., 'N_importance': 16, 'network_fine': nets[1], 'N_samples': 16, 'network_fn': nets[0],
              'use_viewdirs': True, 'white_bkgd': True, 'raw_noise_std': 0., 'ndc': False, 'lindisp': False}
        args = TP.create_args(out_dir, i_print=1000)
        rb = RayBatcher(images, poses, i_split[0], hwf, K, TP.NEAR, TP.FAR, seed=4)
        quiet = lambda s: None                                                                        # noqa: E731
        train(images, poses, i_split, hwf, K, args, kw, opt, 0, N_iters=2, batcher=rb, log=quiet, timing=timing)   # step 1
        torch.cuda.synchronize()
        try:
            last, logged = train(images, poses, i_split, hwf, K, args, kw, opt, 1, N_iters=4, batcher=Guarded(rb, native), log=quiet,
                                 timing=timing)                                                       # steps 2 and 3, no log point
        finally:
            torch.cuda.set_sync_debug_mode('default')
            _refuse_host_reads(False)
        assert (last, logged) == (3, [])
        torch.cuda.synchronize()
        return TP.flat(params), TP.flat([opt.state[p]['exp_avg_sq'] for p in params]), sum(p.numel() for p in params)

    ref, ref_v, P = run()                                                                             # no process group: today's loop
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev, timeout=datetime.timedelta(seconds=120))
    os.environ['NERFAIL_FORCE_COLLECTIVE'] = '1'
    timing = {}
    got, got_v, _ = run(timing)
    ev = timing['allreduce_events']
    np.savez(os.path.join(out_dir, 'train_nccl1.npz'), ref=ref, got=got, ref_v=ref_v, got_v=got_v, P=P, sync_mode_native=native,
             allreduce_ms=np.array([e0.elapsed_time(e1) for e0, e1, _ in ev]), allreduce_bytes=np.array([b for _, _, b in ev]),
             backend=np.array(str(dist.get_backend())))
    dist.destroy_process_group()
    print('train_nccl1 ok', flush=True)


if __name__ == '__main__':
    main(sys.argv[1])
