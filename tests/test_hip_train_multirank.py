"""-m gpu: data-parallel NeRF TRAINING across ranks, executed. Fresh processes share the box's one GPU (gloo process group;
nerfail_amd.sharding stages the gradient arena through pinned host memory - RCCL refuses two ranks on one device), one launch
of tests/mgpu/train_rank.py per world size 1, 2 and 3: fixture g7's training step on each rank's shard + the arena all-reduce,
then train.train() itself - three steps, an idle rank, a checkpoint, a resume. tests/mgpu/train_nccl1.py runs the RCCL branch
once in a 1-rank 'nccl' group."""
import os

import numpy as np
import pytest

from conftest import ROOT
from mgpu import train_problem as TP

pytestmark = pytest.mark.gpu
SCRIPT = os.path.join(ROOT, 'tests', 'mgpu', 'train_rank.py')
WORLDS = (1, 2, 3)

# Step-1 gradient of train(), 2 ranks against 1, per-parameter L2 distance ||a - b|| / ||b||. Both runs evaluate the same rays with
# the same weights (perturb = 0), so the per-ray forward and backward-data are the same numbers; what differs is the order in which
# the weight-gradient kernel and then the all-reduce add the per-sample products: 32 rays x 32 samples, relative rounding ~
# sqrt(1024) x 2^-24 = 1.9e-6, which is the bound. Measured ("Data-parallel training"): worst parameter 7.5e-7 at
# 2 ranks, 6.9e-7 at 3 (the W = 64 weight-gradient kernel adds with atomics: the figure moves in its last digit between runs).
GRAD1_L2_BOUND = 2e-6


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def runs(rank_launcher, tmp_path_factory):
    out = tmp_path_factory.mktemp('train_mgpu')
    for world in WORLDS:
        rep = rank_launcher(SCRIPT, world, [str(out)], timeout=300)
        assert rep['rc'] == [0] * world, '\n'.join(rep['logs'])
    return {w: [dict(np.load(out / ('train_w%d_r%d.npz' % (w, r)))) for r in range(w)] for w in WORLDS}, out


@pytest.mark.parametrize('tag,D,W', TP.G7_TAGS)
def test_g7_step_reduced_gradients(runs, golden, tag, D, W):
    from nerfail_amd._train import GradArena
    from nerfail_amd.run_nerf_helpers import NeRF
    res, _ = runs
    g = golden('g7_train_grads')
    nets = [NeRF(D=D, W=W, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True) for _ in range(2)]
    layout = GradArena(nets, device='cpu')                            # (names and offsets only)
    P = layout.P
    ratios = {}
    for world in WORLDS:
        rs = res[world]
        for r in rs:
            assert int(r[tag + '_P']) == P and bool(r[tag + '_aliased'])
            assert np.array_equal(_bits(r[tag + '_arena']), _bits(rs[0][tag + '_arena']))            # bitwise identical on all ranks
            # ONE collective of 4 (P + 2) bytes per step; a 1-rank run issues none
            assert r[tag + '_calls'].tolist() == ([4 * (P + 2)] if world > 1 else [])
        buf = rs[0][tag + '_arena']
        assert abs(buf[P] - float(g[tag + '_loss'])) < 1e-5 * abs(float(g[tag + '_loss']))           # the loss, in the tail
        ratios[world], lines = TP.g7_worst_ratio(g, tag, TP.arena_named(layout, buf))
        assert ratios[world] <= 1.0, '\n'.join(lines)                                              # test_training_step_gradients' bound
    print('g7 %s: worst error / bound by world size %s' % (tag, {w: round(v, 3) for w, v in ratios.items()}))
    # two ranks: a two-term sum has one order - the reduced arena is bitwise the two ranks' shard arenas added in this process
    two = res[2]
    assert np.array_equal(_bits(two[0][tag + '_arena']), _bits(two[0][tag + '_local'] + two[1][tag + '_local']))
    # ... and bitwise the same two shards computed AGAIN in one process and added on the device, where computing a shard twice
    # gives the same bits: the W = 256 weight-gradient kernel (fixed-order slabs). The W = 64 kernel adds its sample chunks
    # with atomicAdd, so two runs of one shard differ in the last bits (with or without an arena); their distance is printed.
    again = two[0][tag + '_inproc_sum']
    d = np.linalg.norm(again[:P].astype(np.float64) - two[0][tag + '_arena'][:P]) / np.linalg.norm(again[:P].astype(np.float64))
    print('g7 %s: 2-rank result vs the two shards recomputed in one process: L2 distance %.1e' % (tag, d))
    if W == 256:
        assert np.array_equal(_bits(two[0][tag + '_arena']), _bits(again))
    else:
        assert d <= 3072 ** .5 * 2. ** -24      # <= 3072 atomic adds per element (16 rays x 192 samples) in another order: sqrt(n) 2^-24 = 3.3e-6


def test_train_three_steps_ranks_identical(runs):
    res, _ = runs
    one = res[1][0]
    P = int(one['loop_P'])
    for world in WORLDS:
        rs = res[world]
        for r in rs:
            assert r['loop_params'].shape == (TP.STEPS, P)
            assert np.array_equal(_bits(r['loop_params']), _bits(rs[0]['loop_params']))             # after EVERY step
            assert np.array_equal(_bits(r['loop_adam']), _bits(rs[0]['loop_adam']))
            assert np.array_equal(r['loop_losses'], rs[0]['loop_losses']) and len(r['loop_losses']) == TP.STEPS
            assert np.array_equal(r['loop_psnr'], rs[0]['loop_psnr']) and np.isfinite(r['loop_psnr']).all()
            assert np.array_equal(_bits(r['loop_grad1']), _bits(rs[0]['loop_grad1']))
            big = r['loop_calls'][r['loop_calls'] != 8]
            if world == 1:
                assert r['loop_calls'].size == 0                                                    # one rank: no collective at all
            else:                                   # per step ONE all-reduce of the arena; per log point MIN + MAX of the checksum
                assert big.tolist() == [4 * (P + 2)] * TP.STEPS and (r['loop_calls'] == 8).sum() == 2 * TP.STEPS
        assert int(rs[0]['loop_lines']) == TP.STEPS + 1                                             # rank 0 speaks: 3 log lines + the checkpoint
        assert all(int(r['loop_lines']) == 0 for r in rs[1:])
        # the ranks STARTED apart (seeded by rank) and were made rank 0's: which are the 1-rank run's initial parameters
        assert all(not np.array_equal(r['loop_params0'], rs[0]['loop_params0']) for r in rs[1:])
        assert np.array_equal(_bits(rs[0]['loop_params0']), _bits(one['loop_params0']))
        assert not np.array_equal(rs[0]['loop_params'][0], rs[0]['loop_params0'])                   # (they did move)
        # against the 1-rank run: step 1 only (Adam's first steps turn rounding-level gradient differences into +-lr)
        assert abs(rs[0]['loop_losses'][0] - one['loop_losses'][0]) <= 1e-5 * abs(one['loop_losses'][0])
    offs = np.concatenate([[0], np.cumsum([np.prod(s) for net in _loop_shapes() for s in net])]).astype(int)
    for world in (2, 3):
        a, b = res[world][0]['loop_grad1'].astype(np.float64), one['loop_grad1'].astype(np.float64)
        d = [np.linalg.norm(a[lo:hi] - b[lo:hi]) / max(np.linalg.norm(b[lo:hi]), 1e-30) for lo, hi in zip(offs[:-1], offs[1:])]
        print('train() step-1 gradient, %d ranks vs 1: worst per-parameter L2 distance %.2e (whole gradient %.2e)'
              % (world, max(d), np.linalg.norm(a - b) / np.linalg.norm(b)))
        if world == 2:
            assert max(d) <= GRAD1_L2_BOUND
    assert np.linalg.norm(one['loop_grad1']) > 1e-4                                                 # a real gradient


def _loop_shapes():
    from nerfail_amd._train import ordered_params
    from nerfail_amd.run_nerf_helpers import NeRF
    net = NeRF(D=4, W=64, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    shapes = [tuple(p.shape) for p in ordered_params(net)]
    return [shapes, shapes]


def test_idle_rank_joins_and_steps(runs):
    """N_rand = 1 on two ranks: rank 1 owns no ray, adds a zeroed arena to the sum and applies the same step; rank 0, which owns
    the ray, follows the 1-rank run."""
    res, _ = runs
    one, two = res[1][0], res[2]
    assert np.array_equal(_bits(two[0]['idle_params']), _bits(two[1]['idle_params'])) and two[0]['idle_params'].shape[0] == 2
    assert np.array_equal(two[0]['idle_losses'], two[1]['idle_losses'])
    assert np.abs(two[0]['idle_losses'] - one['idle_losses']).max() <= 1e-5 * np.abs(one['idle_losses']).max()
    assert not np.array_equal(two[1]['idle_params'][1], two[1]['idle_params0'])                     # the idle rank stepped
    P = int(one['idle_P'])
    assert two[1]['idle_calls'][two[1]['idle_calls'] != 8].tolist() == [4 * (P + 2)] * 2


def test_checkpoint_from_rank_zero_and_resume(runs):
    res, out = runs
    for world in WORLDS:
        rs = res[world]
        for r in rs:
            assert r['ckpt_files'].tolist() == ['%06d.tar' % TP.STEPS]                              # written once: rank 0's
            # reloaded through create_nerf on every rank: the parameters and Adam state the run ended with ...
            assert np.array_equal(_bits(r['resume_params0']), _bits(rs[0]['loop_params'][-1]))
            # ... and one more step from there, identical on all ranks
            assert np.array_equal(_bits(r['resume_params']), _bits(rs[0]['resume_params']))
            assert np.array_equal(_bits(r['resume_adam']), _bits(rs[0]['resume_adam']))
            assert (r['resume_adam_step'] == TP.STEPS + 1).all()
        assert not np.array_equal(rs[0]['resume_params'][0], rs[0]['resume_params0'])
        assert sorted(os.listdir(out / ('ckpt_w%d_loop' % world) / 'toy')) == ['%06d.tar' % TP.STEPS]


def test_rccl_path_one_rank_training(rank_launcher, tmp_path):
    rep = rank_launcher(os.path.join(ROOT, 'tests', 'mgpu', 'train_nccl1.py'), 1, [str(tmp_path)], timeout=300)
    assert rep['rc'] == [0], '\n'.join(rep['logs'])
    r = np.load(tmp_path / 'train_nccl1.npz')
    assert str(r['backend']) == 'nccl'
    assert np.array_equal(_bits(r['got']), _bits(r['ref'])) and np.array_equal(_bits(r['got_v']), _bits(r['ref_v']))
    assert len(r['allreduce_ms']) == 3 and (r['allreduce_ms'] > 0).all()                            # one collective per step
    assert (r['allreduce_bytes'] == 4 * (int(r['P']) + 2)).all()
    print('RCCL 1-rank all-reduce of the %d-byte arena: %s ms; sync debug mode native: %s'
          % (int(r['allreduce_bytes'][0]), np.round(r['allreduce_ms'], 3), bool(r['sync_mode_native'])))
