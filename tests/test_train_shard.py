"""Host logic of data-parallel NeRF training (nerfail_amd.train / _train.GradArena / sharding), no GPU: where a rank's shard of
a batch lies, the layout of the gradient arena, its reduction through 3 gloo ranks on CPU tensors (one collective of
4 (P + 2) bytes, the loss in the tail), and the ABI 14 interface of the loss share."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT


def _nets():
    from nerfail_amd.run_nerf_helpers import NeRF
    torch.manual_seed(0)
    return [NeRF(D=4, W=64, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True) for _ in range(2)]


@pytest.mark.parametrize('world', [1, 2, 3, 8])
@pytest.mark.parametrize('n', [0, 1, 5, 1024])
def test_shard_positions_partition_the_batch(n, world):
    from nerfail_amd.sharding import shard_range
    pos = []
    for r in range(world):
        lo, hi = shard_range(n, r, world)
        assert 0 <= lo <= hi <= n
        pos += list(range(lo, hi))
    assert pos == list(range(n))                                   # every position once, in order: shards concatenate
    sizes = [hi - lo for lo, hi in (shard_range(n, r, world) for r in range(world))]
    assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)


def test_arena_layout_from_shapes_alone():
    from nerfail_amd._train import GradArena, arena_layout, ordered_params
    shapes = [[(3, 5), (3,), (2, 3), (2,)], [(4, 1), (4,), (7,)]]
    offsets, P = arena_layout(shapes)
    numels = [int(np.prod(s)) for net in shapes for s in net]
    cum = np.concatenate([[0], np.cumsum(numels)])
    assert [o for net in offsets for o in net] == cum[:-1].tolist() and P == cum[-1] == 15 + 3 + 6 + 2 + 4 + 4 + 7
    assert arena_layout([]) == ([], 0)
    nets = _nets()
    arena = GradArena(nets, device='cpu')
    flat = [p for n in nets for p in ordered_params(n)]
    cum = np.concatenate([[0], np.cumsum([p.numel() for p in flat])])
    assert [o for net in arena.offsets for o in net] == cum[:-1].tolist()
    assert arena.P == cum[-1] == sum(p.numel() for n in nets for p in n.parameters())
    assert arena.buf.shape == (arena.P + 2,) and arena.buf.dtype == torch.float32 and arena.nbytes == 4 * (arena.P + 2)
    base = arena.buf.data_ptr()
    for n, offs in zip(nets, arena.offsets):                       # fresh views, of the parameters' shapes, at those offsets
        v1, v2 = arena.views(n), arena.views(n)
        for p, a, b, o in zip(ordered_params(n), v1, v2, offs):
            assert a.shape == p.shape and a.is_contiguous() and a.data_ptr() == b.data_ptr() == base + 4 * o and a is not b
    arena.put_tail(torch.tensor(3.), torch.tensor(2.))
    assert arena.buf[arena.P:].tolist() == [3., 2.] and float(arena.loss) == 3. and float(arena.mse) == 2.


class _IntoArena(torch.autograd.Function):
    """Stand-in of RenderRaysTrain.backward: parameter gradients handed to autograd as fresh views of the arena."""

    @staticmethod
    def forward(ctx, arena, net, *params):
        ctx.arena, ctx.net = arena, net
        return sum((p * p).sum() for p in params)

    @staticmethod
    def backward(ctx, g):
        views = ctx.arena.views(ctx.net, zero=True)
        from nerfail_amd._train import ordered_params
        for v, p in zip(views, ordered_params(ctx.net)):
            v.copy_(2 * p.detach() * g)
        return (None, None) + tuple(views)


def test_autograd_adopts_arena_views_as_grads():
    """What makes the arena free of copies: with p.grad None (optimizer.zero_grad()), autograd keeps the tensor a backward
    returns when nothing else holds it - so a fresh view of the arena BECOMES p.grad. adopt() then has nothing to do, and
    brings in what was accumulated elsewhere (a second backward) or is missing (an idle rank)."""
    from nerfail_amd._train import GradArena, ordered_params
    nets = _nets()
    arena = GradArena(nets, device='cpu')
    for n in nets:
        _IntoArena.apply(arena, n, *ordered_params(n)).backward()
    params = [p for n in nets for p in ordered_params(n)]
    assert all(arena.holds(p.grad) for p in params)
    want = torch.cat([2 * p.detach().reshape(-1) for p in params])
    assert torch.equal(arena.buf[:arena.P], want)
    before = [p.grad.data_ptr() for p in params]
    arena.adopt()
    assert [p.grad.data_ptr() for p in params] == before
    for p in params[:3]:                                           # gradients that live elsewhere are copied in ...
        p.grad = torch.full_like(p, 7.)
    params[3].grad = None                                          # ... and a missing one becomes the view as it is
    arena.adopt()
    assert all(arena.holds(p.grad) for p in params)
    assert all(bool((p.grad == 7.).all()) for p in params[:3]) and torch.equal(params[3].grad, 2 * params[3].detach())
    assert not arena.holds(arena.buf[arena.P:]) and not arena.holds(torch.zeros(3))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path[:0] = [ROOT]
    from nerfail_amd._train import GradArena
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    calls, real = [], dist.all_reduce

    def counted(t, *a, **k):
        calls.append(t.numel() * t.element_size())
        return real(t, *a, **k)
    dist.all_reduce = counted
    arena = GradArena(_nets(), device='cpu')
    rs = np.random.RandomState(100 + rank)
    arena.buf[:arena.P] = torch.from_numpy(rs.normal(size=arena.P).astype(np.float32))
    arena.put_tail(torch.tensor(0.25 * (rank + 1)), torch.tensor(0.125 * (rank + 1)))
    arena.reduce_()
    np.savez(os.path.join(out_dir, 'r%d.npz' % rank), buf=arena.buf.numpy(), calls=np.array(calls), P=arena.P)
    dist.destroy_process_group()


def test_arena_reduction_three_gloo_ranks(tmp_path):
    mp.spawn(_worker, args=(3, _free_port(), str(tmp_path)), nprocs=3, join=True)
    got = [np.load(tmp_path / ('r%d.npz' % r)) for r in range(3)]
    P = int(got[0]['P'])
    parts = [np.random.RandomState(100 + r).normal(size=P).astype(np.float32) for r in range(3)]
    want = parts[0].astype(np.float64) + parts[1] + parts[2]
    for g in got:
        assert np.array_equal(g['buf'], got[0]['buf'])                                     # identical on every rank
        assert g['calls'].tolist() == [4 * (P + 2)]                                         # ONE collective, gradients + loss + mse
    assert np.abs(got[0]['buf'][:P] - want).max() <= 2 * np.finfo(np.float32).eps * np.abs(parts).sum(0).max()
    assert got[0]['buf'][P:].tolist() == [1.5, 0.75]                                       # the tail carries loss and mse


def test_world_one_issues_no_collective(monkeypatch):
    from nerfail_amd._train import GradArena
    monkeypatch.delenv('NERFAIL_FORCE_COLLECTIVE', raising=False)
    arena = GradArena(_nets(), device='cpu')
    arena.buf.fill_(1.5)
    assert not dist.is_initialized()
    assert torch.equal(arena.reduce_(), torch.full((arena.P + 2,), 1.5))


def test_abi_14_loss_share_declared_everywhere():
    from nerfail_amd import _lib
    import ctypes
    header = open(os.path.join(ROOT, 'include', 'nerfail_hip.h')).read()
    assert _lib.ABI_VERSION == 14
    assert int(re.search(r'#define NERFAIL_ABI_VERSION (\d+)', header).group(1)) == 14
    decl = re.search(r'int nerfail_mse_part\(([^)]*)\);', header).group(1)
    assert [a.strip() for a in decl.split(',')] == ['const float* x', 'const float* y', 'int64_t n', 'int64_t n_total', 'float* loss',
                                                    'float* dx', 'void* stream']
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    assert _lib.SIGNATURES['nerfail_mse_part'] == (ctypes.c_int, [p, p, i64, i64, p, p, p])
    lib = _lib.load()
    assert lib.nerfail_abi_version() == 14
    assert lib.nerfail_mse_part(None, None, 0, 0, None, None, None) == 1 and b'positive' in lib.nerfail_last_error()
    assert lib.nerfail_mse_part(None, None, 8, 7, None, None, None) == 1 and b'n_total' in lib.nerfail_last_error()
    assert lib.nerfail_mse_part(None, None, 8, 8, None, None, None) == 1 and b'NULL' in lib.nerfail_last_error()
    assert lib.nerfail_mse(None, None, 8, None, None, None) == 1 and b'NULL' in lib.nerfail_last_error()


def test_public_interface_has_the_sharding_keywords():
    import inspect
    from nerfail_amd import sharding, train
    from nerfail_amd.run_nerf_helpers import img2mse
    b = inspect.signature(train.RayBatcher.batch).parameters
    assert b['rank'].default == 0 and b['world'].default == 1
    assert inspect.signature(train.train).parameters['group'].default is None
    assert inspect.signature(img2mse).parameters['n_total'].default is None
    assert callable(sharding.broadcast_)
    x, y = torch.arange(6.).reshape(2, 3), torch.ones(2, 3)
    assert float(img2mse(x, y, n_total=12)) == float(((x - y) ** 2).sum() / 12)          # (the torch expression, off the GPU)
    with pytest.raises(ValueError):
        img2mse(x, y, n_total=5)
