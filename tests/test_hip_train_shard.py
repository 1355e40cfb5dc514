"""-m gpu, one process: the pieces of data-parallel NeRF training (nerfail_amd.train: sharded batches, one gradient
all-reduce). A rank's batch shard is rows [lo, hi) of the 1-rank batch, bit for bit; the loss share over a global count
(nerfail_mse_part, ABI 14) adds up to the mean; a training step run shard by shard into gradient arenas adds up to the
reference's gradient within the bound the unsharded step is held to; and after backward every p.grad lies in the arena."""
import numpy as np
import pytest
import torch

from hiputil import T, N, dev
from mgpu import train_problem as TP

pytestmark = pytest.mark.gpu


def _batchers(world, seed=5):
    from nerfail_amd.train import RayBatcher
    images, poses, hwf, K = TP.scene()
    mk = lambda: RayBatcher(images, poses, [0, 1, 2, 3], hwf, K, TP.NEAR, TP.FAR, seed=seed)     # noqa: E731
    return mk(), [mk() for _ in range(world)]


def _assert_shards_concatenate(one, ranks, steps, **kw):
    world = len(ranks)
    sizes = []
    for step in range(steps):
        full = one.batch(step, return_sel=True, **kw)
        parts = [rb.batch(step, return_sel=True, rank=r, world=world, **kw) for r, rb in enumerate(ranks)]
        for a, ps in zip(full, zip(*parts)):
            cat = torch.cat(ps, 0)
            assert cat.shape == a.shape and cat.dtype == a.dtype
            assert torch.equal(cat.view(torch.int32) if a.dtype == torch.float32 else cat, a.view(torch.int32) if a.dtype == torch.float32 else a)
        n = full[0].shape[0]
        from nerfail_amd.sharding import shard_ranges
        assert [p[0].shape[0] for p in parts] == [hi - lo for lo, hi in shard_ranges(n, world)]
        for rb in ranks:                                   # bookkeeping advances by the GLOBAL n on every rank
            assert (rb.epoch, rb.i_batch, rb.n_global) == (one.epoch, one.i_batch, n)
        sizes.append(n)
    return sizes


@pytest.mark.parametrize('world', [2, 3])
def test_batch_shards_concatenate_bitwise(world):
    one, ranks = _batchers(world)
    assert _assert_shards_concatenate(one, ranks, 3, N_rand=20) == [20] * 3                        # one view, full window (64 pixels)
    assert _assert_shards_concatenate(one, ranks, 2, N_rand=10, precrop=.5) == [10] * 2            # precrop: window 4 x 4
    assert _assert_shards_concatenate(one, ranks, 2, N_rand=100) == [64] * 2                       # N_rand above the window
    assert _assert_shards_concatenate(one, ranks, 1, N_rand=20, precrop=.5) == [16]                # ... and above the cropped one
    # epochs over all 4 x 64 = 256 pixels: 100 + 100 + 56, then a new order - five batches cross the boundary
    assert _assert_shards_concatenate(one, ranks, 5, N_rand=100, use_batching=True) == [100, 100, 56, 100, 100]
    assert one.epoch == 1 and one.i_batch == 200
    sel = np.array([3, 63, 0, 17, 40, 41, 9], np.int64)                                           # an explicit sel is sliced the same way
    full = one.batch(0, 0, view=2, sel=sel)
    parts = [rb.batch(0, 0, view=2, sel=sel, rank=r, world=world) for r, rb in enumerate(ranks)]
    for a, ps in zip(full, zip(*parts)):
        assert torch.equal(torch.cat(ps, 0), a)


def test_empty_shard_makes_no_launch(monkeypatch):
    from nerfail_amd import _lib
    one, ranks = _batchers(2)
    full = one.batch(7, 1)
    lib, launches = _lib.load(), []
    real = lib.nerfail_train_batch
    monkeypatch.setattr(lib, 'nerfail_train_batch', lambda *a: launches.append(a[18]) or real(*a))         # a[18]: n
    a = ranks[0].batch(7, 1, rank=0, world=2)
    b = ranks[1].batch(7, 1, rank=1, world=2, return_sel=True)
    assert (a[0].shape[0], b[0].shape[0]) == (1, 0) and launches == [1]                                   # N_rand = 1 over 2 ranks: (1, 0)
    assert tuple(b[0].shape) == (0, 11) and tuple(b[1].shape) == (0, 3) and tuple(b[2].shape) == (0,) and b[2].dtype == torch.int64
    assert b[0].device == a[0].device and torch.equal(a[0], full[0]) and torch.equal(a[1], full[1])
    assert ranks[1].n_global == 1


def test_loss_share_bits_and_sum():
    from nerfail_amd.run_nerf_helpers import img2mse
    from nerfail_amd.sharding import shard_ranges
    rs = np.random.RandomState(3)
    n = 1000
    x, y = rs.uniform(size=(n, 3)).astype(np.float32), rs.uniform(size=(n, 3)).astype(np.float32)
    xa, xb = T(x).requires_grad_(True), T(x).requires_grad_(True)
    la, lb = img2mse(xa, T(y)), img2mse(xb, T(y), n_total=3 * n)                                  # n_total = n: nerfail_mse's bits
    la.backward(), lb.backward()
    assert torch.equal(la.detach().view(torch.int32), lb.detach().view(torch.int32)) and torch.equal(xa.grad, xb.grad)
    mean64 = float(((x.astype(np.float64) - y) ** 2).mean())
    assert abs(float(la.detach()) - mean64) <= 1e-5 * mean64
    shares, grads = [], []
    for lo, hi in shard_ranges(n, 3):                                                             # 334 + 333 + 333 rays
        xs = T(x[lo:hi]).requires_grad_(True)
        l = img2mse(xs, T(y[lo:hi]), n_total=3 * n)
        l.backward()
        shares.append(float(l.detach()))
        grads.append(xs.grad)
    total = float(np.sum(np.array(shares, np.float32), dtype=np.float32))
    print('loss shares %s sum %.9g, float64 mean %.9g, rel %.1e' % (shares, total, mean64, abs(total - mean64) / mean64))
    assert abs(total - mean64) <= 1e-5 * mean64                                                   # (the loss tolerance of tests/test_hip_train.py)
    assert torch.equal(torch.cat(grads, 0), xa.grad)                                              # 2 (x - y) / n_total, element by element
    with pytest.raises(ValueError):
        img2mse(xa, T(y), n_total=3 * n - 1)


@pytest.mark.parametrize('tag,D,W', TP.G7_TAGS)
def test_sharded_step_sums_to_reference_gradient(golden, tag, D, W):
    """Fixture g7's training step run as two shards, each into an arena of its own, the two arenas added: every parameter
    within 2 x spread + 2e-6 of the reference's fp32 gradient (test_training_step_gradients' bound). W = 256 takes the
    weight-gradient kernel that overwrites its outputs, W = 64 the one that zeroes and accumulates."""
    from nerfail_amd._train import GradArena, ordered_params
    from nerfail_amd.sharding import shard_ranges
    g = golden('g7_train_grads')
    coarse, fine = TP.g7_nets(D, W)
    params = [p for n in (coarse, fine) for p in ordered_params(n)]
    R = g[tag + '_rays'].shape[0]
    loss1, _ = TP.g7_shard_step(g, tag, coarse, fine, 0, R)                                       # the unsharded step, as today
    unsharded = TP.flat([p.grad for p in params])
    arenas = [GradArena([coarse, fine]) for _ in range(2)]
    for arena in arenas:
        arena.buf.fill_(float('nan'))                                                             # whatever a previous step left
    for arena, (lo, hi) in zip(arenas, shard_ranges(R, 2)):
        TP.g7_shard_step(g, tag, coarse, fine, lo, hi, arena)
        assert all(arena.holds(p.grad) for p in params)                                           # p.grad aliases the arena: nothing to gather
        lo_b, hi_b = arena.buf.data_ptr(), arena.buf.data_ptr() + 4 * arena.P
        assert all(lo_b <= p.grad.data_ptr() < hi_b for p in params)
        for p, off in zip(params, [o for offs in arena.offsets for o in offs]):
            assert p.grad.data_ptr() == lo_b + 4 * off and p.grad.shape == p.shape
    total = N(arenas[0].buf + arenas[1].buf)
    P = arenas[0].P
    assert np.isfinite(total).all()
    assert abs(total[P] - float(g[tag + '_loss'])) < 1e-5 * abs(float(g[tag + '_loss']))          # the loss shares add up, in the tail
    assert abs(total[P] - float(loss1)) < 1e-5 * abs(float(loss1)) and 0 < total[P + 1] < total[P]
    w_sharded, lines = TP.g7_worst_ratio(g, tag, TP.arena_named(arenas[0], total))
    w_one, _ = TP.g7_worst_ratio(g, tag, TP.arena_named(arenas[0], np.concatenate([unsharded, [0, 0]]).astype(np.float32)))
    print('\n'.join(lines))
    print('g7 %s: worst error / bound, two shards summed %.3f, unsharded step %.3f' % (tag, w_sharded, w_one))
    assert w_sharded <= 1.0, '\n'.join(lines)


def test_render_rays_without_arena_allocates_as_before(golden):
    from nerfail_amd._train import ordered_params
    g = golden('g7_train_grads')
    coarse, fine = TP.g7_nets(4, 64)
    TP.g7_shard_step(g, 'small', coarse, fine, 0, 8)
    ps = ordered_params(coarse)
    assert ps[1].grad.data_ptr() == ps[0].grad.data_ptr() + 4 * ps[0].numel()                     # _new_grads: one flat buffer per network
    assert dev().type == 'cuda'
