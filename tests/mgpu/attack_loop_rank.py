#!/usr/bin/env python3
"""One rank of the two-rank nerfail_s test (tests/test_hip_attack_loop.py). Started as a fresh process by tests/mgpu/launcher.py;
every rank uses HIP device 0, so the process group is gloo (see tests/mgpu/rank.py). Runs attack.nerfail_s on fixture g24's
beta run and stores what the ranks must agree on.

    python tests/mgpu/attack_loop_rank.py OUTDIR          -> OUTDIR/loop_w{world}_r{rank}.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from mgpu import attack_loop_problem as AP  # noqa: E402


def main(out_dir):
    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    if world > 1:
        dist.init_process_group('gloo', rank=rank, world_size=world)
    from nerfail_amd.attack import STAT_FIELDS
    g = AP.load()
    out = {}
    for tag in ('beta', 'untargeted'):
        exported = []
        res, _ = AP.run(g, tag, dev, on_export=lambda i, vids, adv, mask: exported.append((i, adv.shape[0])))
        out[tag + '_best'], out[tag + '_last'] = res.best.cpu().numpy(), res.last.cpu().numpy()
        out[tag + '_stats'] = np.array([[d[k] for k in STAT_FIELDS] for d in res.stats], np.float64)
        out[tag + '_best_epoch'] = res.best_epoch
        out[tag + '_exported'] = np.array(exported)
    np.savez(os.path.join(out_dir, 'loop_w%d_r%d.npz' % (world, rank)), **out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print('rank %d/%d ok' % (rank, world), flush=True)


if __name__ == '__main__':
    main(sys.argv[1])
