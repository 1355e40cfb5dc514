"""The per-ray view bias of the folded bf16x3 kernel (mlp_x3.hip: x3_viewbias_kernel and the RAYBIAS form of
nerf_mlp_fwd_x3_kernel). CPU: the numpy statement of the rule vb[r][i] = f32(bc[i] + sum_m Wv[i][W + m] enc(d_r)[m]) (terms
m = 0..26 in this order in double, one rounding). -m gpu: the device's vb bit for bit against it, the density bit for bit
against the plain folded kernel, the colour by the error rule of test_hip_mlp_x3_fold.py, and the dispatch (what the new
form must leave alone, that the points form and the rays form meet in it, that only a caller inside per_ray_view_bias() -
the renderer - gets it).

The grid of the kernel is min(tiles / 4, CUs) and cannot be set from a test: 'more tiles than one round' is reached by
tile count instead (R = 1100 rays of 32 samples = 1100 tiles > 4 x 256).

Colour error against float64, max over the 13 cases as measured on an MI355X: new form 5.0e-8 .. 9.6e-8, plain folded kernel
2.6e-8 .. 5.5e-8, exact f32 kernel 3.6e-8 .. 7.5e-8, at scales 0.08 .. 0.19. Every case passes the rule of
test_hip_mlp_x3_fold.py (e <= 2 e_exact + 1e-7 scale, e < 2e-5 scale); the new form's error is NOT below the exact kernel's own
in 12 of the 13 cases (the plain folded kernel's is not in 1). Each case prints its three errors."""
import numpy as np
import pytest
import torch

import synth
import x3fold_ref as R

W = 256
F32 = np.float32


# ------------------------------------------------------------------------------------------------ the rule in numpy
def band_sel(x, f, h):
    """SinCosBands::band_sel (common.h) operation by operation: sin (h = 0) or cos (h = 1) of x * 2^f, x float32."""
    u = (np.asarray(x, F32).astype(np.float64) * 0.63661977236758134308) * float(1 << f)
    q = np.rint(u)
    phi = (u - q).astype(F32) * F32(1.57079632679489661923)
    z = phi * phi
    s = phi + phi * z * (F32(-1.6666654611e-1) + z * (F32(8.3321608736e-3) + z * F32(-1.9515295891e-4)))
    c = F32(1.0) - F32(0.5) * z + z * z * (F32(4.166664568298827e-2) + z * (F32(-1.388731625493765e-3) + z * F32(2.443315711809948e-5)))
    k = q.astype(np.int64) + h
    v = np.where(k & 1, c, s).astype(F32)
    return (v.view(np.uint32) ^ ((k & 2).astype(np.uint32) << 30)).view(F32)


def enc_dir(d):
    """[R,3] float32 -> [R,27]: x, y, z, then per band sin(3), cos(3) (the Embedder's channel order)."""
    d = np.asarray(d, F32)
    cols = [d]
    for f in range(4):
        cols += [band_sel(d, f, 0), band_sel(d, f, 1)]
    return np.concatenate(cols, 1).astype(F32)


def vb_rule(wv_dir, bc, dirs):
    """wv_dir [128,27] f32 = Wv[:, W:], bc [128] f32 (the composed bias as the image holds it), dirs [R,3] -> vb [R,128] f32."""
    e = enc_dir(dirs).astype(np.float64)
    w = np.asarray(wv_dir, F32).astype(np.float64)
    acc = np.broadcast_to(np.asarray(bc, F32).astype(np.float64), (e.shape[0], w.shape[0])).copy()
    for m in range(27):
        acc += w[None, :, m] * e[:, m:m + 1]
    return acc.astype(F32)


def _dirs(rs, n):
    d = rs.normal(size=(n, 3)).astype(F32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    d[0] = (0., 0., 1.)                                               # axis-aligned: exact zeros in the encoding
    return d


def test_vb_rule_in_numpy():
    rs = np.random.RandomState(1)
    wv = rs.normal(scale=0.1, size=(128, 27)).astype(F32)
    bc = rs.normal(size=(128,)).astype(F32)
    d = _dirs(rs, 5)
    e = enc_dir(d)
    # the encoding is sin / cos of d * 2^f to within an ulp or two of the polynomial, in the Embedder's order
    ref = np.concatenate([d.astype(np.float64)] + [fn(d.astype(np.float64) * 2. ** f) for f in range(4) for fn in (np.sin, np.cos)], 1)
    assert e.shape == (5, 27) and np.abs(e - ref).max() < 3e-7
    assert np.array_equal(e[0, :3], [0., 0., 1.]) and np.all(e[0, [3, 4, 9, 10]] == 0.) and np.all(e[0, [6, 7]] == 1.)
    vb = vb_rule(wv, bc, d)
    assert vb.dtype == F32 and vb.shape == (5, 128)
    exact = bc.astype(np.float64) + e.astype(np.float64) @ wv.astype(np.float64).T
    # one rounding of a double sum of 27 exact products: within half an ulp (+ the double sum's own 2^-53 steps) of the exact value
    assert np.all(np.abs(vb - exact) <= 0.5000001 * np.spacing(np.maximum(np.abs(vb), np.abs(exact).astype(F32))).astype(np.float64))
    # the order is part of the rule: the sum is the one a sequential loop gives
    i, r = 7, 3
    acc = np.float64(bc[i])
    for m in range(27):
        acc += np.float64(wv[i, m]) * np.float64(e[r, m])
    assert F32(acc) == vb[r, i]


# ------------------------------------------------------------------------------------------------ the device
gpu = pytest.mark.gpu
SHAPES = [(8, [4]), (4, [1]), (2, [])]                                # SKIP = 1, 2, 0 of the kernel


def _net(D, skips, seed):
    from hiputil import dev
    from nerfail_amd.run_nerf_helpers import NeRF
    sd = synth.nerf_state_dict(D=D, W=W, skips=tuple(skips), seed=seed)
    net = NeRF(D=D, W=W, input_ch=63, input_ch_views=27, output_ch=5, skips=list(skips), use_viewdirs=True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return sd, net.requires_grad_(False).to(dev())


def _case(seed, R_, Ns):
    rs = np.random.RandomState(seed)
    o = rs.uniform(-1, 1, size=(R_, 3)).astype(F32)
    vd = _dirs(rs, R_)
    d = (vd * rs.uniform(0.5, 2., size=(R_, 1))).astype(F32)
    z = np.sort(rs.uniform(2, 6, size=(R_, Ns)).astype(F32), axis=1)
    pts = ((d[:, None, :] * z[:, :, None]) + o[:, None, :]).astype(F32)           # RN:381 rounding: multiply, then add
    rays = np.concatenate([o, d, np.full((R_, 1), 2., F32), np.full((R_, 1), 6., F32), vd], 1)
    return pts, vd, rays, z


def _lib():
    from nerfail_amd import _lib as L
    return L, L.load()


class _Forced:
    """fwd_select / raybias_select for the length of a block."""
    def __init__(self, fwd=None, raybias=None):
        self.fwd, self.raybias = fwd, raybias

    def __enter__(self):
        lib = _lib()[1]
        self.pf = lib.nerfail_mlp_fwd_select(self.fwd) if self.fwd is not None else None
        self.pr = lib.nerfail_mlp_x3_raybias_select(self.raybias) if self.raybias is not None else None

    def __exit__(self, *a):
        lib = _lib()[1]
        if self.pf is not None:
            lib.nerfail_mlp_fwd_select(self.pf)
        if self.pr is not None:
            lib.nerfail_mlp_x3_raybias_select(self.pr)


def _run_rays(net, rays, z, which):
    """which: 'new' (the _raybias entry point), 'old' (the plain folded kernel), 'lds' (the exact f32 kernel)."""
    from hiputil import T, N, dev
    L, lib = _lib()
    R_, Ns = z.shape
    D, skip = net.D, net._skip()
    raw = torch.full((R_, Ns, 4), float('nan'), dtype=torch.float32, device=dev())
    tr, tz = T(rays), T(z)
    packed, img = L.dev(net.packed()), L.dev(net.packed_x3f())
    if which == 'new':
        n = lib.nerfail_mlp_x3f_raybias_floats(D, W, skip, R_, Ns)
        assert n == R_ * 128
        vb = torch.full((n,), float('nan'), dtype=torch.float32, device=dev())
        L.check(lib.nerfail_mlp_fwd_rays_x3f_raybias(packed, img, D, W, skip, L.dev(tr), L.dev(tz), R_, Ns, L.dev(raw), L.dev(vb), L.stream()))
    elif which == 'old':
        L.check(lib.nerfail_mlp_fwd_rays_x3f(packed, img, D, W, skip, L.dev(tr), L.dev(tz), R_, Ns, L.dev(raw), None, L.stream()))
    else:
        with _Forced(fwd=2):
            L.check(lib.nerfail_mlp_fwd_rays(packed, D, W, skip, L.dev(tr), L.dev(tz), R_, Ns, L.dev(raw), None, L.stream()))
    torch.cuda.synchronize()
    return N(raw)


def _f64(net, pts, vd):
    from hiputil import T, N
    from nerfail_amd.run_nerf_helpers import get_embedder
    from test_hip_mlp_x3 import _f64_forward
    R_, Ns = pts.shape[:2]
    ep, _ = get_embedder(10, 0)
    ed, _ = get_embedder(4, 0)
    tp, tv = T(pts), T(vd)
    x = torch.cat([ep(tp.reshape(-1, 3)), ed(tv[:, None, :].expand(R_, Ns, 3).reshape(-1, 3))], -1).float().contiguous()
    return _f64_forward(net, N(x)).reshape(R_, Ns, 4), x


CASES = [(D, s, 5, Ns) for D, s in SHAPES for Ns in (32, 64, 96)] + [(D, s, 300, 32) for D, s in SHAPES] + [(2, [], 1100, 32)]


@gpu
@pytest.mark.parametrize('D,skips,R_,Ns', CASES)
def test_view_bias_and_raybias_kernel(D, skips, R_, Ns):
    from hiputil import T, N, dev
    L, lib = _lib()
    sd, net = _net(D, skips, seed=500 + D)
    assert net.packed_x3f() is not None
    pts, vd, rays, z = _case(10 * D + Ns + R_, R_, Ns)
    skip = net._skip()

    # 1. vb from the device, both input forms, bit for bit the numpy rule (row r in bias piece order)
    _, bc = R.compose(sd)
    exp = np.empty((R_, 128), F32)
    exp[:, R.bias_index(np.arange(128))] = vb_rule(sd['views_linears.0.weight'][:, W:], bc, vd)
    packed, img = L.dev(net.packed()), L.dev(net.packed_x3f())
    tr, tv = T(rays), T(vd)
    for form in ('rays', 'viewdirs'):
        vb = torch.full((R_, 128), float('nan'), dtype=torch.float32, device=dev())
        src = (L.dev(tr), None) if form == 'rays' else (None, L.dev(tv))
        L.check(lib.nerfail_mlp_x3f_viewbias(packed, img, D, W, skip, src[0], src[1], R_, L.dev(vb), L.stream()))
        torch.cuda.synchronize()
        got = N(vb)
        bad = np.flatnonzero(got.view(np.int32) != exp.view(np.int32))
        assert bad.size == 0, (form, bad.size, bad[:8], got.reshape(-1)[bad[:4]], exp.reshape(-1)[bad[:4]])

    # 2. density bit for bit the plain folded kernel's; every sample written
    new, old = _run_rays(net, rays, z, 'new'), _run_rays(net, rays, z, 'old')
    assert np.isfinite(new).all()
    assert np.array_equal(new[..., 3].view(np.int32), old[..., 3].view(np.int32))

    # 3. colour against float64 by the rule of test_hip_mlp_x3_fold.py (_check_error), the exact kernel on the same input
    ref, _ = _f64(net, pts, vd)
    ref = ref[..., :3]
    scale = np.abs(ref).max()
    e_new = np.abs(new[..., :3].astype(np.float64) - ref).max()
    e_old = np.abs(old[..., :3].astype(np.float64) - ref).max()
    e_lds = np.abs(_run_rays(net, rays, z, 'lds')[..., :3].astype(np.float64) - ref).max()
    print('D %d skips %s R %d N %d: e_new %.3e e_old %.3e e_lds %.3e scale %.3e' % (D, skips, R_, Ns, e_new, e_old, e_lds, scale))
    assert e_new <= 2 * e_lds + 1e-7 * scale, (e_new, e_lds, scale)
    assert e_new < 2e-5 * scale, (e_new, scale)
    if R_ >= 300:
        assert not np.array_equal(new[..., :3], old[..., :3])          # identical bits: the new form would not be running

    # 4. the run repeats bit for bit (a stale row slot or bias tile of an earlier round would differ)
    assert np.array_equal(_run_rays(net, rays, z, 'new').view(np.int32), new.view(np.int32))


@gpu
@pytest.mark.parametrize('D,skips', SHAPES)
def test_points_form_and_wrappers_meet_in_the_new_form(D, skips):
    from hiputil import T, N, dev
    from nerfail_amd.run_nerf import _mlp_points, _mlp_rays
    L, lib = _lib()
    _, net = _net(D, skips, seed=520 + D)
    R_, Ns = 37, 64
    pts, vd, rays, z = _case(3 + D, R_, Ns)
    new = _run_rays(net, rays, z, 'new')
    raw = torch.full((R_, Ns, 4), float('nan'), dtype=torch.float32, device=dev())
    vb = torch.empty((R_ * 128,), dtype=torch.float32, device=dev())
    tp, tv = T(pts), T(vd)
    L.check(lib.nerfail_mlp_fwd_x3f_raybias(L.dev(net.packed()), L.dev(net.packed_x3f()), D, W, net._skip(), L.dev(tp), L.dev(tv),
                                            R_ * Ns, Ns, L.dev(raw), L.dev(vb), L.stream()))
    torch.cuda.synchronize()
    assert np.array_equal(N(raw).view(np.int32), new.view(np.int32))
    from nerfail_amd.run_nerf_helpers import per_ray_view_bias
    with per_ray_view_bias():                                          # a caller that asks for the form, as the renderer does
        assert np.array_equal(N(_mlp_points(net, tp, tv)).view(np.int32), new.view(np.int32))
        assert np.array_equal(N(_mlp_rays(net, T(rays), T(z))).view(np.int32), new.view(np.int32))
    old = _run_rays(net, rays, z, 'old')
    # the bare wrappers keep the plain folded kernel: their bits are those of the embedded form of the same batch
    assert np.array_equal(N(_mlp_points(net, tp, tv)).view(np.int32), old.view(np.int32))
    assert np.array_equal(N(_mlp_rays(net, T(rays), T(z))).view(np.int32), old.view(np.int32))
    with _Forced(raybias=0), per_ray_view_bias():                      # the switch: the plain folded kernel, and no vb asked for
        assert lib.nerfail_mlp_x3f_raybias_floats(D, W, net._skip(), R_, Ns) == 0
        assert np.array_equal(N(_mlp_rays(net, T(rays), T(z))).view(np.int32), old.view(np.int32))
    with _Forced(fwd=2):                                               # a forced exact kernel is not overridden
        assert lib.nerfail_mlp_x3f_raybias_floats(D, W, net._skip(), R_, Ns) == 0


@gpu
def test_dispatch_leaves_other_calls_alone():
    """48 samples per ray (tiles straddle rays) and the pre-embedded entry point: bit for bit what the forced-old path gives."""
    from hiputil import T, N
    from nerfail_amd.run_nerf import _mlp_points, _mlp_rays
    L, lib = _lib()
    _, net = _net(8, [4], seed=541)
    R_, Ns = 21, 48
    pts, vd, rays, z = _case(77, R_, Ns)
    assert lib.nerfail_mlp_x3f_raybias_floats(8, W, 4, R_, Ns) == 0 and lib.nerfail_mlp_x3f_raybias_floats(8, W, 4, R_, 64) == R_ * 128
    _, x = _f64(net, pts, vd)
    from nerfail_amd.run_nerf_helpers import per_ray_view_bias
    with per_ray_view_bias():
        a_r, a_p, a_e = N(_mlp_rays(net, T(rays), T(z))), N(_mlp_points(net, T(pts), T(vd))), N(net(x))
    with _Forced(raybias=0), per_ray_view_bias():
        b_r, b_p, b_e = N(_mlp_rays(net, T(rays), T(z))), N(_mlp_points(net, T(pts), T(vd))), N(net(x))
    for a, b in ((a_r, b_r), (a_p, b_p), (a_e, b_e)):
        assert np.isfinite(a).all() and np.array_equal(a.view(np.int32), b.view(np.int32))
    assert np.array_equal(a_r.view(np.int32), _run_rays(net, rays, z, 'old').view(np.int32))
    # the entry points of the new form refuse such a call instead of computing something else
    raw, vb = torch.empty((R_, Ns, 4), device=T(z).device), torch.empty((R_ * 128,), device=T(z).device)
    rc = lib.nerfail_mlp_fwd_rays_x3f_raybias(L.dev(net.packed()), L.dev(net.packed_x3f()), 8, W, 4, L.dev(T(rays)), L.dev(T(z)), R_, Ns,
                                              L.dev(raw), L.dev(vb), L.stream())
    assert rc != 0


@gpu
def test_renderer_takes_the_new_form():
    """render_rays (64 coarse + 128 fine samples: 64 and 192 per ray) runs the per-ray view-bias form: against the same render
    with the form switched off every density-derived map is bitwise equal and the colours agree to f32 level without being
    the same bits. The colour bound: the two raw colours lie within 2e-7 of each other (each within 1e-7 of float64 in the
    cases above), the sigmoid's slope is at most 1/4 and the compositing weights sum to at most 1, so the maps differ by
    under 1e-7 plus the f32 roundings of a sum of 192 terms in [0, 1] (6e-8 each way, a handful of them): 1e-6."""
    from hiputil import T
    from nerfail_amd import nerf_to_coord as NC
    lib = _lib()[1]
    (_, mc), (_, mf) = _net(8, [4], seed=561), _net(8, [4], seed=562)
    rays = T(synth.ray_batch(96, seed=9))

    def render():
        with torch.no_grad():
            return NC.render_rays(rays, mc, None, 64, N_importance=128, network_fine=mf, white_bkgd=True)
    a = render()
    with _Forced(raybias=0):
        b = render()
    for k in ('acc_map', 'disp_map', 'acc0', 'disp0', 'z_std', 'pts_max'):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    for k in ('rgb_map', 'rgb0'):
        assert not torch.equal(a[k], b[k]), k                          # identical bits: the new form would not be running
        assert float((a[k] - b[k]).abs().max()) <= 1e-6, k
