"""-m gpu: the folded bf16x3 inference kernel (feature_linear composed into the views layer at pack time, mlp_x3.hip) -
the image byte for byte, error against float64 by the rule of the unfolded kernel's test, the bias hand-over between
persistent rounds, ragged last tiles, the entry-point forms, cache invalidation, the overflow fall-back, guard pages."""
import os
import sys

import numpy as np
import pytest
import torch

import synth
import x3fold_ref as R
from hiputil import T, N, dev
from test_hip_mlp_x3 import _f64_forward, _select
from test_hip_mlp_x3 import _embedded as _embedded_cpu
from test_hip_mlp_x3_16 import _expected_image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(D, skips, seed):
    from nerfail_amd.run_nerf_helpers import NeRF
    sd = synth.nerf_state_dict(D=D, W=256, skips=tuple(skips), seed=seed)
    net = NeRF(D=D, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=list(skips), use_viewdirs=True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return sd, net.requires_grad_(False).to(dev())


def _lib():
    from nerfail_amd import _lib as L
    return L, L.load()


def _run(net, x, M, rows, fold=True):
    """The embedded entry point (folded or not) over the first M rows of x into a NaN-filled [rows, 4] buffer."""
    L, lib = _lib()
    raw = torch.full((rows, 4), float('nan'), dtype=torch.float32, device=dev())
    img = net.packed_x3f() if fold else net.packed_x3()
    assert img is not None
    fwd = lib.nerfail_mlp_fwd_embedded_x3f if fold else lib.nerfail_mlp_fwd_embedded_x3
    L.check(fwd(L.dev(net.packed()), L.dev(img), net.D, 256, net._skip(), L.dev(x), M, L.dev(raw), L.stream()))
    torch.cuda.synchronize()
    return N(raw)


def _forward(net, x, which):
    prev = _select(which)
    try:
        return N(net(T(x)))
    finally:
        _select(prev)


# ------------------------------------------------------------------------------------------------ 1. image byte for byte
@pytest.mark.parametrize('D,skips', [(8, [4]), (2, [])])
def test_folded_image_byte_for_byte(D, skips):
    L, lib = _lib()
    sd, net = _net(D, skips, seed=41 + D)
    skip = net._skip()
    n = lib.nerfail_mlp_packed_x3f_bytes(D, 256, skip)
    buf = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev())     # unwritten bytes would show
    L.check(lib.nerfail_mlp_pack_x3f(L.dev(net.packed()), D, 256, skip, L.dev(buf), L.stream()))
    torch.cuda.synchronize()
    got = N(buf)
    assert np.array_equal(got, N(net.packed_x3f()))

    wc, bc = R.compose(sd)
    folded, unfolded = R.stream_tile_steps(D, skip)
    # the stream: layers 0 .. D-1 as the unfolded image has them, then ONE views layer = [Wc | direction columns]
    sdf = dict(sd)
    sdf['views_linears.0.weight'] = np.concatenate([wc, sd['views_linears.0.weight'][:, 256:]], 1)
    full = _expected_image(sdf, D, skip)                             # uint16; the feature layer sits between the two
    per_step = 3 * 64 * 8                                            # bf16 values of one tile-step
    head = (unfolded - 72 - 128) * per_step
    exp_stream = np.concatenate([full[:head], full[head + 128 * per_step:]])
    stream = got[:folded * 3 * 1024].view(np.uint16)
    assert stream.shape == exp_stream.shape
    bad = np.flatnonzero(stream != exp_stream)
    assert bad.size == 0, (bad.size, bad[:8])

    # the constant area: that of the f32 image, bias piece D = bc (zero behind it)
    f32 = N(net.packed())
    nconst = (D + 2) * 256 + 1024
    exp_const = f32[f32.size - nconst:].copy()
    piece = np.zeros(256, np.float32)
    piece[R.bias_index(np.arange(128))] = bc
    exp_const[D * 256:(D + 1) * 256] = piece
    tail = got[folded * 3 * 1024:].view(np.uint32)
    assert np.array_equal(tail[:nconst], exp_const.view(np.uint32))
    # the composed f32 block
    assert np.array_equal(tail[nconst:nconst + 128 * 256], wc.reshape(-1).view(np.uint32))
    exp_bc = np.zeros(256, np.float32)
    exp_bc[:128] = bc
    assert np.array_equal(tail[nconst + 128 * 256:], exp_bc.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. error against float64
def _check_error(net, x):
    assert net.packed_x3f() is not None
    ref = _f64_forward(net, x)
    scale = np.abs(ref).max()
    out = _forward(net, x, 0)
    assert np.isfinite(out).all()
    e_fold = np.abs(out.astype(np.float64) - ref).max()
    e_lds = np.abs(_forward(net, x, 2).astype(np.float64) - ref).max()
    print('e_fold %.3e e_lds %.3e scale %.3e' % (e_fold, e_lds, scale))
    assert np.array_equal(_forward(net, x, 3), out)                 # forced x and the default: the same folded path
    assert np.array_equal(out, _run(net, T(x), x.shape[0], x.shape[0]))   # ... which IS the folded kernel
    assert e_fold <= 2 * e_lds + 1e-7 * scale, (e_fold, e_lds, scale)
    assert e_fold < 2e-5 * scale, (e_fold, scale)


@pytest.mark.parametrize('D,skips', [(8, [4]), (8, [3]), (8, []), (6, [2]), (6, [3]), (4, [1]), (4, [2]), (2, [])])
def test_fold_error_against_float64_is_exact_kernel_level(D, skips):
    _, net = _net(D, skips, seed=300 + D)
    rs = np.random.RandomState(10 * D + (skips[0] if skips else 9))
    _check_error(net, N(_embedded_cpu(rs, 4099)))                    # 129 tiles: a ragged last tile


def test_fold_takes_large_and_tiny_weights():
    _, net = _net(8, [4], seed=7)
    with torch.no_grad():
        net.pts_linears[2].weight[:16] *= 1e3 / net.pts_linears[2].weight[:16].abs().max()
        net.pts_linears[5].weight[:32] *= 1e-20
        net.feature_linear.weight[40:48] *= 1e-20
    _check_error(net, N(_embedded_cpu(np.random.RandomState(3), 2048)))


# ------------------------------------------------------------------------------------------------ 3. rounds
def test_fold_bias_hand_over_between_rounds():
    """More than two rounds of a 256-CU grid: the first and the last 4 096 rows equal single-round runs over just those
    samples (a stale bias of layer 0 or of the views layer would differ), and the run repeats bit for bit."""
    _, net = _net(8, [4], seed=53)
    M = 2 * 1024 * 32 + 1000
    x = T(N(_embedded_cpu(np.random.RandomState(4), M)))
    a = _run(net, x, M, M + 32)
    b = _run(net, x, M, M + 32)
    assert np.isfinite(a[:M]).all() and np.isnan(a[M:]).all()
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    first = _run(net, x[:4096].contiguous(), 4096, 4096)
    last = _run(net, x[M - 4096:].contiguous(), 4096, 4096)
    assert np.array_equal(a[:4096].view(np.int32), first.view(np.int32))
    assert np.array_equal(a[M - 4096:M].view(np.int32), last.view(np.int32))


# ------------------------------------------------------------------------------------------------ 4. ragged last tile
@pytest.mark.parametrize('last', [1, 16, 17, 31])
def test_fold_ragged_last_tile_stores_only_its_rows(last):
    _, net = _net(8, [4], seed=51)
    full = 32 * 37
    x = T(N(_embedded_cpu(np.random.RandomState(last), full)))
    M = 32 * 36 + last
    ref = _run(net, x, full, full)
    got = _run(net, x, M, full)
    assert np.isfinite(ref).all()
    assert np.array_equal(got[:M].view(np.int32), ref[:M].view(np.int32))
    assert np.isnan(got[M:]).all()


# ------------------------------------------------------------------------------------------------ 5. entry-point forms
def _ray_case(seed, R_, Ns):
    rs = np.random.RandomState(seed)
    o = rs.uniform(-1, 1, size=(R_, 3)).astype(np.float32)
    d = rs.normal(size=(R_, 3)).astype(np.float32)
    vd = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    z = np.sort(rs.uniform(2, 6, size=(R_, Ns)).astype(np.float32), axis=1)
    pts = ((d[:, None, :] * z[:, :, None]) + o[:, None, :]).astype(np.float32)     # RN:381 rounding: multiply, then add
    rays = np.concatenate([o, d, np.full((R_, 1), 2., np.float32), np.full((R_, 1), 6., np.float32), vd], 1)
    return pts, vd, rays, z


def test_fold_entry_point_forms_give_the_same_bits():
    from nerfail_amd.run_nerf_helpers import get_embedder
    L, lib = _lib()
    _, net = _net(8, [4], seed=13)
    R_, Ns = 1031, 64
    pts, vd, rays, z = _ray_case(8, R_, Ns)
    packed, img = L.dev(net.packed()), L.dev(net.packed_x3f())
    tp, tv, tr, tz = T(pts), T(vd), T(rays), T(z)
    a = torch.empty((R_, Ns, 4), dtype=torch.float32, device=dev())
    b, c, u = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    L.check(lib.nerfail_mlp_fwd_x3f(packed, img, 8, 256, 4, L.dev(tp), L.dev(tv), R_ * Ns, Ns, L.dev(a), L.stream()))
    L.check(lib.nerfail_mlp_fwd_rays_x3f(packed, img, 8, 256, 4, L.dev(tr), L.dev(tz), R_, Ns, L.dev(b), None, L.stream()))
    ep, _ = get_embedder(10, 0)
    ed, _ = get_embedder(4, 0)
    x = torch.cat([ep(tp.reshape(-1, 3)), ed(tv[:, None, :].expand(R_, Ns, 3).reshape(-1, 3))], -1).float().contiguous()
    L.check(lib.nerfail_mlp_fwd_embedded_x3f(packed, img, 8, 256, 4, L.dev(x), R_ * Ns, L.dev(c), L.stream()))
    L.check(lib.nerfail_mlp_fwd_x3(packed, L.dev(net.packed_x3()), 8, 256, 4, L.dev(tp), L.dev(tv), R_ * Ns, Ns, L.dev(u), L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    from nerfail_amd.run_nerf import _mlp_points, _mlp_rays            # ... and the Python wrappers take the same path
    assert torch.equal(_mlp_points(net, tp, tv).view(torch.int32), a.view(torch.int32))
    assert torch.equal(_mlp_rays(net, tr, tz).view(torch.int32), a.view(torch.int32))
    assert torch.equal(net(x).reshape(R_, Ns, 4).view(torch.int32), c.view(torch.int32))
    ref = float(u.abs().max())
    assert not torch.equal(a, u)                                     # identical bits: the fold would not be running
    assert float((a - u).abs().max()) <= 2e-5 * ref


# ------------------------------------------------------------------------------------------------ 6. invalidation
@pytest.mark.parametrize('name', ['feature_linear.weight', 'feature_linear.bias', 'views_linears.0.weight', 'views_linears.0.bias'])
def test_folded_image_follows_an_in_place_change(name):
    from nerfail_amd.run_nerf import _mlp_points
    _, net = _net(8, [4], seed=11)
    pts, vd, _, _ = _ray_case(5, 64, 64)
    pts, vd = T(pts), T(vd)
    a = _mlp_points(net, pts, vd).clone()
    img = net.packed_x3f()
    assert img is not None and net.packed_x3f() is img               # cached
    with torch.no_grad():
        dict(net.named_parameters())[name].mul_(1.5)
    b = _mlp_points(net, pts, vd)
    assert net.packed_x3f() is not img
    assert not torch.equal(a, b)
    prev = _select(2)
    try:
        ref = _mlp_points(net, pts, vd)
    finally:
        _select(prev)
    assert torch.allclose(b, ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ 7. overflow fall-back
def test_overflowing_composition_falls_back_to_the_unfolded_kernel():
    L, lib = _lib()
    _, net = _net(8, [4], seed=23)
    with torch.no_grad():
        net.feature_linear.weight.mul_(1e20 / float(net.feature_linear.weight.abs().max()))
        net.views_linears[0].weight[:, :256].mul_(1e20 / float(net.views_linears[0].weight[:, :256].abs().max()))
    assert net.packed_x3f() is None and net.packed_x3() is not None
    x = T(N(_embedded_cpu(np.random.RandomState(6), 1000)))
    got = net(x)
    raw = torch.empty_like(got)
    L.check(lib.nerfail_mlp_fwd_embedded_x3(L.dev(net.packed()), L.dev(net.packed_x3()), 8, 256, 4, L.dev(x), 1000, L.dev(raw), L.stream()))
    torch.cuda.synchronize()
    assert np.array_equal(N(got).view(np.int32), N(raw).view(np.int32))


# ------------------------------------------------------------------------------------------------ 8. guard pages
def test_fold_under_guard_pages(rank_launcher):
    """Every buffer ends at an unmapped page: a read past the folded image (stream, constants) or a store past the output
    is a fault in the child's log."""
    rep = rank_launcher(os.path.abspath(__file__), 1, [], timeout=300, env={'NERFAIL_GUARD_ALLOC': '1'})
    log = '\n'.join(rep['logs'])
    assert rep['rc'] == [0], log
    assert 'Memory access fault' not in log and '[guard_alloc] active' in log and 'X3 FOLD GUARD OK' in log, log


def _guard_child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import guard
    assert guard.install_if_wanted()
    _, net = _net(8, [4], seed=29)
    M = 1024 * 32 + 37                                              # two rounds, ragged end
    x = T(N(_embedded_cpu(np.random.RandomState(2), M)))
    out = _run(net, x, M, M)
    assert np.isfinite(out).all()
    print('X3 FOLD GUARD OK', flush=True)


if __name__ == '__main__':
    _guard_child()
