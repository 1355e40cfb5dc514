"""-m gpu: the weight ring of the bf16x3 kernels (mlp_x3.hip: X3Ring keeps its LDS and source offsets as bytes and advances
them by increments) at the sample counts where its bookkeeping can go wrong - one tile, a ragged second tile, exactly one
persistent round, a second round in which all waves but one only recompute, and three rounds (the source offset wraps from
the stream's end to its start while the ring slot is mid-cycle) - for one network shape per SKIP instantiation, folded
and unfolded entry points. Each result is compared with the exact kernel on the same input by the bound
test_hip_mlp_x3_fold.py uses for that comparison; canary rows behind M stay untouched; two calls give identical bits."""
import numpy as np
import pytest
import torch

from hiputil import T, N, dev
from test_hip_mlp_x3 import _select
from test_hip_mlp_x3_fold import _net, _lib

pytestmark = pytest.mark.gpu

SHAPES = [(2, []), (8, [4]), (4, [1])]          # SKIP = 0, 1, 2 (skip layer absent, odd, even)
CANARY = 64
_cache = {}


def _cu():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def _counts():
    rnd = 32 * 4 * _cu()
    return [1, 33, rnd, rnd + 1, 3 * rnd - 31]


def _case(D, skips):
    """Network, inputs for the largest count and the exact kernel's result on them: computed once per shape."""
    key = (D, tuple(skips))
    if key not in _cache:
        L, lib = _lib()
        _, net = _net(D, skips, seed=700 + D)
        rs = np.random.RandomState(13 * D + 1)
        M = _counts()[-1]
        R_, Ns = (M + 63) // 64, 64
        o = rs.uniform(-1, 1, size=(R_, 1, 3)).astype(np.float32)
        d = rs.normal(size=(R_, 1, 3)).astype(np.float32)
        z = rs.uniform(2, 6, size=(R_, Ns, 1)).astype(np.float32)
        pts = T((o + d * z).astype(np.float32))
        vd = T((d[:, 0] / np.linalg.norm(d[:, 0], axis=1, keepdims=True)).astype(np.float32))
        ref = torch.empty((R_ * Ns, 4), dtype=torch.float32, device=dev())
        prev = _select(2)                                            # NERFAIL_FWD_KERNEL=lds: the exact kernel
        try:
            L.check(lib.nerfail_mlp_fwd_x3(L.dev(net.packed()), L.dev(net.packed_x3()), D, 256, net._skip(), L.dev(pts), L.dev(vd),
                                           R_ * Ns, Ns, L.dev(ref), L.stream()))
            torch.cuda.synchronize()
        finally:
            _select(prev)
        assert bool(torch.isfinite(ref).all())
        _cache[key] = (net, pts, vd, ref)
    return _cache[key]


def _run(net, pts, vd, M, fold):
    L, lib = _lib()
    out = torch.full((M + CANARY, 4), float('nan'), dtype=torch.float32, device=dev())
    img = net.packed_x3f() if fold else net.packed_x3()
    assert img is not None
    fwd = lib.nerfail_mlp_fwd_x3f if fold else lib.nerfail_mlp_fwd_x3
    prev = _select(3)                                                # the bf16x3 kernel, not the exact one
    try:
        L.check(fwd(L.dev(net.packed()), L.dev(img), net.D, 256, net._skip(), L.dev(pts), L.dev(vd), M, 64, L.dev(out), L.stream()))
        torch.cuda.synchronize()
    finally:
        _select(prev)
    return out


@pytest.mark.parametrize('fold', [True, False], ids=['x3f', 'x3'])
@pytest.mark.parametrize('D,skips', SHAPES)
def test_ring_rounds_against_exact_kernel(D, skips, fold):
    net, pts, vd, ref = _case(D, skips)
    for M in _counts():
        a = _run(net, pts, vd, M, fold)
        b = _run(net, pts, vd, M, fold)
        assert bool(torch.isnan(a[M:]).all()), 'M = %d: canary rows written' % M
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'M = %d: two calls differ' % M
        r = ref[:M]
        err = float((a[:M] - r).abs().max())
        print('D %d skips %s fold %d M %d: max abs err %.3e (scale %.3e)' % (D, skips, fold, M, err, float(r.abs().max())))
        assert not torch.equal(a[:M], r) or M < 64                   # identical bits: the exact kernel would be running
        assert torch.allclose(a[:M], r, rtol=1e-4, atol=1e-4 * float(r.abs().max())), 'M = %d' % M
