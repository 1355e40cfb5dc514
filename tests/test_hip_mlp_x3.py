"""-m gpu: the bf16x3 inference kernel (mlp_x3.hip, the default of the x3 entry points) - error against a float64 forward
next to the exact-f32 kernel's, weight range, cache invalidation, equality of its entry-point forms, and the selection."""
import numpy as np
import pytest
import torch

import synth
from hiputil import T, N, dev

pytestmark = pytest.mark.gpu


def _net(D, W, skips, seed):
    from nerfail_amd.run_nerf_helpers import NeRF
    sd = synth.nerf_state_dict(D=D, W=W, skips=tuple(skips), seed=seed)
    net = NeRF(D=D, W=W, input_ch=63, input_ch_views=27, output_ch=5, skips=list(skips), use_viewdirs=True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.requires_grad_(False).to(dev())


def _f64_forward(net, x):
    """RH:100-123 in float64 on an embedded batch x [M, 90]."""
    sd = {k: v.detach().cpu().double().numpy() for k, v in net.state_dict().items()}
    x = np.asarray(x, np.float64)
    inp, views = x[:, :63], x[:, 63:]
    h = inp
    for i in range(net.D):
        h = np.maximum(h @ sd['pts_linears.%d.weight' % i].T + sd['pts_linears.%d.bias' % i], 0.)
        if i in net.skips:
            h = np.concatenate([inp, h], -1)
    alpha = h @ sd['alpha_linear.weight'].T + sd['alpha_linear.bias']
    feat = h @ sd['feature_linear.weight'].T + sd['feature_linear.bias']
    h = np.maximum(np.concatenate([feat, views], -1) @ sd['views_linears.0.weight'].T + sd['views_linears.0.bias'], 0.)
    rgb = h @ sd['rgb_linear.weight'].T + sd['rgb_linear.bias']
    return np.concatenate([rgb, alpha], -1)


def _embedded(rs, M):
    """An embedded batch as Embedder builds it (x, sin/cos bands) from random points and unit directions."""
    from nerfail_amd.run_nerf_helpers import get_embedder
    pts = torch.from_numpy(rs.uniform(-3, 3, size=(M, 3)).astype(np.float32))
    vd = rs.normal(size=(M, 3)).astype(np.float32)
    vd = torch.from_numpy(vd / np.linalg.norm(vd, axis=1, keepdims=True))
    ep, _ = get_embedder(10, 0)
    ed, _ = get_embedder(4, 0)
    return torch.cat([ep(pts), ed(vd)], -1).float().contiguous()


def _select(which):
    from nerfail_amd import _lib
    return _lib.load().nerfail_mlp_fwd_select(which)


def _forward(net, x, which):
    prev = _select(which)
    try:
        return N(net(T(x)))
    finally:
        _select(prev)


@pytest.mark.parametrize('D,skips', [(8, [4]), (8, [3]), (8, []), (6, [2]), (6, [3]), (4, [1]), (4, [2]), (2, [])])
def test_x3_error_against_float64_is_exact_kernel_level(D, skips):
    net = _net(D, 256, skips, seed=300 + D)
    rs = np.random.RandomState(10 * D + (skips[0] if skips else 9))
    x = N(_embedded(rs, 4099))                                   # 129 tiles: a ragged last tile
    ref = _f64_forward(net, x)
    scale = np.abs(ref).max()
    e_x3 = np.abs(_forward(net, x, 0).astype(np.float64) - ref).max()
    e_lds = np.abs(_forward(net, x, 2).astype(np.float64) - ref).max()
    assert np.array_equal(_forward(net, x, 3), _forward(net, x, 0))   # the default IS the x3 kernel
    assert e_x3 <= 2 * e_lds + 1e-7 * scale, (e_x3, e_lds, scale)
    assert e_x3 < 2e-5 * scale, (e_x3, scale)


def test_x3_takes_large_and_tiny_weights():
    """bf16 has the f32 exponent range: rows of magnitude 1e3 and 1e-20 stay at f32-level error, no inf / NaN."""
    net = _net(8, 256, [4], seed=7)
    with torch.no_grad():
        net.pts_linears[2].weight[:16] *= 1e3 / net.pts_linears[2].weight[:16].abs().max()
        net.pts_linears[5].weight[:32] *= 1e-20
        net.feature_linear.weight[40:48] *= 1e-20
    rs = np.random.RandomState(3)
    x = N(_embedded(rs, 2048))
    ref = _f64_forward(net, x)
    out = _forward(net, x, 0)
    assert np.isfinite(out).all()
    scale = np.abs(ref).max()
    e_x3 = np.abs(out.astype(np.float64) - ref).max()
    e_lds = np.abs(_forward(net, x, 2).astype(np.float64) - ref).max()
    assert e_x3 <= 2 * e_lds + 1e-7 * scale and e_x3 < 2e-5 * scale, (e_x3, e_lds, scale)


def test_x3_image_follows_an_in_place_change_of_a_streamed_weight():
    from nerfail_amd.run_nerf import _mlp_points
    net = _net(8, 256, [4], seed=11)
    rs = np.random.RandomState(5)
    pts = T(rs.uniform(-3, 3, size=(64, 64, 3)).astype(np.float32))
    vd = rs.normal(size=(64, 3)).astype(np.float32)
    vd = T(vd / np.linalg.norm(vd, axis=1, keepdims=True))
    a = _mlp_points(net, pts, vd).clone()
    img = net.packed_x3()
    assert img is not None and net.packed_x3() is img              # cached
    with torch.no_grad():
        net.pts_linears[3].weight.mul_(1.5)
    b = _mlp_points(net, pts, vd)
    assert not torch.equal(a, b)
    prev = _select(2)
    try:
        ref = _mlp_points(net, pts, vd)
    finally:
        _select(prev)
    assert torch.allclose(b, ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))


def test_x3_point_and_ray_forms_give_the_same_bits():
    """Default selection: the ray form (points formed in the kernel) equals the point form bitwise, over a multi-round
    persistent grid with a ragged last tile."""
    from nerfail_amd.run_nerf import _mlp_points, _mlp_rays
    net = _net(8, 256, [4], seed=13)
    rs = np.random.RandomState(8)
    R, Ns = 1031, 64
    o = rs.uniform(-1, 1, size=(R, 3)).astype(np.float32)
    d = rs.normal(size=(R, 3)).astype(np.float32)
    vd = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    z = np.sort(rs.uniform(2, 6, size=(R, Ns)).astype(np.float32), axis=1)
    pts = (d[:, None, :] * z[:, :, None]) + o[:, None, :]        # RN:381 rounding: multiply, then add
    rays = np.concatenate([o, d, np.full((R, 1), 2., np.float32), np.full((R, 1), 6., np.float32), vd], 1)
    a = _mlp_points(net, T(pts.astype(np.float32)), T(vd))
    b = _mlp_rays(net, T(rays), T(z))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    prev = _select(2)
    try:
        c = _mlp_rays(net, T(rays), T(z))
    finally:
        _select(prev)
    assert not torch.equal(b, c)                                  # the default is not the exact kernel
    assert torch.allclose(b, c, rtol=0, atol=2e-5 * float(c.abs().max()))


@pytest.mark.parametrize('which', [1, 2])
def test_forced_exact_kernels_still_run_the_exact_kernels(which):
    from nerfail_amd import _lib
    from nerfail_amd.run_nerf import _mlp_points
    lib = _lib.load()
    net = _net(8, 256, [4], seed=17)
    rs = np.random.RandomState(9)
    pts = T(rs.uniform(-3, 3, size=(100, 64, 3)).astype(np.float32))
    vd = rs.normal(size=(100, 3)).astype(np.float32)
    vd = T(vd / np.linalg.norm(vd, axis=1, keepdims=True))
    prev = _select(which)
    try:
        a = _mlp_points(net, pts, vd)
        raw = torch.empty_like(a)
        _lib.check(lib.nerfail_mlp_fwd(_lib.dev(net.packed()), 8, 256, 4, _lib.dev(pts), _lib.dev(vd), 6400, 64,
                                       _lib.dev(raw), _lib.stream()))
    finally:
        _select(prev)
    assert torch.equal(a.view(torch.int32), raw.view(torch.int32))


@pytest.mark.parametrize('D,W,skips', [(8, 128, [4]), (4, 64, [2]), (5, 256, [2])])
def test_shapes_the_x3_kernel_does_not_cover_fall_back(D, W, skips):
    from nerfail_amd import _lib
    from nerfail_amd.run_nerf import _mlp_points
    lib = _lib.load()
    net = _net(D, W, skips, seed=19)
    assert net.packed_x3() is None
    assert lib.nerfail_mlp_packed_x3_bytes(D, W, skips[0]) == 0
    rs = np.random.RandomState(10)
    pts = T(rs.uniform(-3, 3, size=(40, 64, 3)).astype(np.float32))
    vd = rs.normal(size=(40, 3)).astype(np.float32)
    vd = T(vd / np.linalg.norm(vd, axis=1, keepdims=True))
    a = _mlp_points(net, pts, vd)
    raw = torch.empty_like(a)
    _lib.check(lib.nerfail_mlp_fwd(_lib.dev(net.packed()), D, W, net._skip(), _lib.dev(pts), _lib.dev(vd), 40 * 64, 64,
                                   _lib.dev(raw), _lib.stream()))
    assert torch.equal(a.view(torch.int32), raw.view(torch.int32))
