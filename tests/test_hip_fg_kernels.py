"""-m gpu: the three kernels of foreground-only scene maps (fg revision 1) and render_pixels, each against what it must equal bit
for bit: nerfail_fg_pixel_list against np.flatnonzero(alpha > 0), nerfail_ray_gen_list against ray_gen's rows, the list search
against view_map's rows (zero bits elsewhere), render_pixels against the full render's rows. Every comparison is an ==; only
sum_d2 has a bound (1e-10 relative: a fixed-order double fold against numpy's float64 sum of the same 8 n float32 squares, whose
worst reordering error is 8 n 2^-53 < 2e-12)."""
import numpy as np
import pytest
import torch

import synth
from hiputil import T, N, dev, hip_nerf

pytestmark = pytest.mark.gpu

C = 0.02


def _disc_list(H, W):
    """The foreground of synth.disc_alpha_image at H x W (about 44 % of the pixels), as numpy int32."""
    a = synth.disc_alpha_image(1, H, W, seed=3)[0, ..., 3]
    return np.flatnonzero(a.reshape(-1) > 0).astype(np.int32)


# ------------------------------------------------------------------------------------------------- pixel list
def _alphas():
    rs = np.random.RandomState(11)
    out = {}
    for H, W in ((40, 40), (37, 23)):
        P = H * W
        last = np.zeros(P, np.uint8)
        last[-1] = 7
        one_vs_zero = (np.arange(P) % 3 == 0).astype(np.uint8)                       # alpha = 1 against 0
        yy, xx = np.mgrid[:H, :W]
        out.update({('zeros', H, W): np.zeros(P, np.uint8), ('full', H, W): np.full(P, 255, np.uint8), ('last', H, W): last,
                    ('one', H, W): one_vs_zero, ('checker', H, W): (((yy + xx) & 1) * 200).astype(np.uint8).reshape(-1),
                    ('disc', H, W): synth.disc_alpha_image(1, H, W, seed=2)[0, ..., 3].astype(np.uint8).reshape(-1)})
    out[('random', 300, 300)] = (rs.uniform(size=90000) < 0.5).astype(np.uint8) * rs.randint(1, 256, 90000).astype(np.uint8)
    return out


ALPHAS = _alphas()


@pytest.mark.parametrize('key', sorted(ALPHAS), ids=lambda k: '%s-%dx%d' % k)
def test_pixel_list_is_flatnonzero(key):
    from nerfail_amd import ops
    from nerfail_amd.scene import foreground_pixels
    _, H, W = key
    alpha = ALPHAS[key]
    img = np.random.RandomState(5).randint(0, 256, (H, W, 4)).astype(np.uint8)       # colour bytes must not matter
    img[..., 3] = alpha.reshape(H, W)
    want = np.flatnonzero(alpha > 0).astype(np.int32)
    lst, count = ops.fg_pixel_list(T(img))
    assert lst.dtype == torch.int32 and count.dtype == torch.int32 and int(count) == len(want), key
    assert np.array_equal(N(lst)[:len(want)], want), key
    for form in (img, torch.from_numpy(img), T(img)):
        got = foreground_pixels(form)
        assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(N(got), want), key
    lst2, count2 = ops.fg_pixel_list(T(img))                                          # the same bits on a second run
    assert torch.equal(lst[:len(want)], lst2[:len(want)]) and torch.equal(count, count2)


def test_foreground_pixels_reads_four_bytes(monkeypatch):
    from nerfail_amd.scene import foreground_pixels
    img = T(synth.disc_alpha_image(1, 40, 40, seed=1)[0].astype(np.uint8))
    reads = []
    for n in ('cpu', 'item', 'tolist', 'numpy', '__int__', '__float__', '__bool__', '__index__'):
        def f(self, *a, _orig=getattr(torch.Tensor, n), _n=n, **k):
            if self.is_cuda:
                reads.append((_n, self.numel() * self.element_size()))
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, n, f)
    pix = foreground_pixels(img)
    monkeypatch.undo()
    assert reads and reads[0] == ('__int__', 4) and all(r == ('item', 4) for r in reads[1:]) and len(reads) <= 2, reads   # (int() may go through item)
    assert int(pix.shape[0]) == int((img[..., 3] > 0).sum())
    with pytest.raises(ValueError, match='uint8 BGRA'):
        foreground_pixels(img.float())


# ------------------------------------------------------------------------------------------------- rays for a list
def test_ray_gen_list_rows_are_ray_gen_rows():
    from nerfail_amd import run_nerf as RN, ops as O
    H, W = 37, 23
    P = H * W
    focal, K = synth.lego_intrinsics(H, W)
    c2w = torch.from_numpy(synth.pose_spherical(37., -30., 4.))[:3, :4]
    full = RN.ray_gen(H, W, K, c2w, 2., 6.)
    rs = np.random.RandomState(2)
    lists = [np.zeros(0, np.int32), np.array([P - 1], np.int32)] + [np.sort(rs.choice(P, n, replace=False)).astype(np.int32) for n in (63, 64, 65)]
    lists += [np.arange(P, dtype=np.int32), rs.permutation(P).astype(np.int32)]
    for pix in lists:
        got = RN.ray_gen_list(H, W, K, c2w, 2., 6., T(pix))
        assert tuple(got.shape) == (len(pix), 11) and got.dtype == torch.float32
        assert torch.equal(got.view(torch.int32), full[torch.from_numpy(pix).long().to(dev())].view(torch.int32)), len(pix)
    assert O.FG_OPS == ('ray_gen_list',)
    for pix in (lists[2], lists[0]):
        torch.library.opcheck(torch.ops.nerfail_mi.ray_gen_list.default, (torch.from_numpy(K), c2w, T(pix), H, W, 2., 6.),
                              test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_dynamic'))


# ------------------------------------------------------------------------------------------------- the list search
@pytest.fixture(scope='module')
def search():
    """40 x 40 queries of the rough sphere against three such views: 4 800 points, the grid path. view_map's map, once."""
    from nerfail_amd.scene import PointSet, view_map
    ps = PointSet(T(np.stack([synth.sphere_view_points(40, 40, th) for th in (-120., 0., 120.)]).reshape(-1, 3)))
    assert ps.Ns == 4800 and ps._grid is not None
    Q = T(synth.sphere_view_points(40, 40, 45.))
    full, _ = view_map(Q, ps, C)
    from nerfail_amd.create_index_and_dist import knn8
    dist, _ = knn8(Q, ps.points, method='grid')
    return ps, Q, full, N(dist).reshape(-1, 8)


def _lists_40():
    rs = np.random.RandomState(4)
    disc = _disc_list(40, 40)
    assert 650 < len(disc) < 760
    return {'0': np.zeros(0, np.int32), '1': np.array([1234], np.int32), '65': np.sort(rs.choice(1600, 65, replace=False)).astype(np.int32),
            'disc': disc, 'P': np.arange(1600, dtype=np.int32)}


LISTS_40 = _lists_40()


@pytest.mark.parametrize('name', list(LISTS_40))
def test_list_search_rows_are_view_map_rows(search, name):
    from nerfail_amd.scene import view_map_pixels
    ps, Q, full, dist = search
    pix = LISTS_40[name]
    n = len(pix)
    sel = torch.from_numpy(pix).long().to(dev())
    pts = Q.reshape(-1, 3)[sel]
    wi, d2 = view_map_pixels(pts, T(pix), (40, 40), ps, C)
    wi2, d2b = view_map_pixels(pts, T(pix), (40, 40), ps, C)
    assert tuple(wi.shape) == (2, 40, 40, 8) and d2.dtype == torch.float64 and d2.dim() == 0
    a, f = wi.reshape(2, 1600, 8).view(torch.int32), full.reshape(2, 1600, 8).view(torch.int32)
    assert torch.equal(a[:, sel], f[:, sel]), name                                      # listed rows: view_map's bits
    rest = torch.ones(1600, dtype=torch.bool, device=dev())
    rest[sel] = False
    assert int(rest.sum()) == 1600 - n and not bool(a[:, rest].any()), name             # every other row: zero bits
    assert torch.equal(a, wi2.reshape(2, 1600, 8).view(torch.int32)) and N(d2).tobytes() == N(d2b).tobytes()
    d = dist[pix].reshape(-1)
    ref = float((d * d).astype(np.float32).astype(np.float64).sum())
    print('n = %d: sum_d2 %.17g, numpy %.17g' % (n, float(d2), ref))
    assert abs(float(d2) - ref) <= 1e-10 * ref
    if n == 0:
        assert float(d2) == 0.0 and N(d2).tobytes() == np.float64(0.).tobytes()
    # the brute-force route below GRID_FROM writes the same rows
    wb, d2r = view_map_pixels(pts, T(pix), (40, 40), ps, C, method='brute')
    assert torch.equal(wb.view(torch.int32), wi.view(torch.int32)), name
    assert abs(float(d2r) - ref) <= 1e-10 * ref


def test_list_search_refusals_leave_the_map_alone(search):
    from nerfail_amd import _lib
    from nerfail_amd.scene import view_map_pixels
    ps, Q, full, _ = search
    lib = _lib.load()
    pix = T(LISTS_40['65'])
    pts = Q.reshape(-1, 3)[pix.long()].contiguous()
    ws, nbytes = ps.grid()
    out = torch.full((2, 1600, 8), float('nan'), device=dev())
    d2 = torch.full((1,), float('nan'), dtype=torch.float64, device=dev())
    wb = lib.nerfail_knn8_grid_weights_workspace_bytes(65)
    work = torch.empty((wb // 8,), dtype=torch.float64, device=dev())

    def call(m=4800, gb=nbytes, c=C):
        return lib.nerfail_knn8_grid_weights_list(_lib.dev(pts), 65, _lib.dev(pix), 1600, m, c, _lib.dev(out), _lib.c_p(d2.data_ptr()), _lib.dev(ws), gb,
                                                  _lib.c_p(work.data_ptr()), wb, _lib.stream())
    for kw, word in ((dict(m=4799), b'does not match the grid'), (dict(gb=nbytes - 1), b'grid workspace too small'), (dict(c=0.), b'c must be positive')):
        assert call(**kw) == 1 and word in lib.nerfail_last_error(), kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(d2).all())                 # refused before the zeroing launch
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:, pix.long()], full.reshape(2, 1600, 8)[:, pix.long()]) and not bool(torch.isnan(out).any())
    with pytest.raises(ValueError, match='n <= H'):
        view_map_pixels(pts, pix[:64], (40, 40), ps, C)
    with pytest.raises(_lib.NerfailError, match='c must be positive'):
        view_map_pixels(pts, pix, (40, 40), ps, 0.)


# ------------------------------------------------------------------------------------------------- render_pixels
SIDE = 40


def _kwargs(D, W, seeds):
    from nerfail_amd import run_nerf as RN
    _, coarse = hip_nerf(D, W, seeds[0])
    _, fine = hip_nerf(D, W, seeds[1])
    q = RN.FusedNetworkQuery(RN.get_embedder(10, 0)[0], RN.get_embedder(4, 0)[0])
    return dict(network_query_fn=q, perturb=0., N_importance=8, network_fine=fine, N_samples=8, network_fn=coarse, use_viewdirs=True,
                white_bkgd=True, raw_noise_std=0., ndc=False, lindisp=False, near=2., far=6.)


class Render:
    """One network pair under one forward selection: the full 40 x 40 render, once."""

    def __init__(self, D, W, seeds, select):
        from nerfail_amd import _lib, nerf_to_coord as NC
        self.kw, self.select = _kwargs(D, W, seeds), select
        focal, self.K = synth.lego_intrinsics(SIDE, SIDE)
        self.c2w = torch.from_numpy(synth.pose_spherical(25., -30., 4.))[:3, :4]
        prev = _lib.load().nerfail_mlp_fwd_select(select)
        try:
            with torch.no_grad():
                rgb, disp, acc, pts, extras = NC.render(SIDE, SIDE, self.K, chunk=1024, c2w=self.c2w, **self.kw)
        finally:
            _lib.load().nerfail_mlp_fwd_select(prev)
        self.full = dict(extras, rgb_map=rgb, disp_map=disp, acc_map=acc, pts_max=pts)
        self.full = {k: v.reshape((SIDE * SIDE,) + tuple(v.shape[2:])) for k, v in self.full.items()}

    def pixels(self, pix, pts_max=True):
        from nerfail_amd import _lib, nerf_to_coord as NC, run_nerf as RN
        prev = _lib.load().nerfail_mlp_fwd_select(self.select)
        try:
            with torch.no_grad():
                if pts_max:
                    rgb, disp, acc, pts, extras = NC.render_pixels(SIDE, SIDE, self.K, T(pix), chunk=1024, c2w=self.c2w, **self.kw)
                    return dict(extras, rgb_map=rgb, disp_map=disp, acc_map=acc, pts_max=pts)
                rgb, disp, acc, extras = RN.render_pixels(SIDE, SIDE, self.K, T(pix), chunk=1024, c2w=self.c2w, **self.kw)
                return dict(extras, rgb_map=rgb, disp_map=disp, acc_map=acc)
        finally:
            _lib.load().nerfail_mlp_fwd_select(prev)


RENDERS = {'D4W64-default': (4, 64, (71, 72), 0), 'D8W256-default': (8, 256, (73, 74), 0), 'D8W256-exact': (8, 256, (73, 74), 2)}


@pytest.fixture(scope='module')
def renders():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Render(*RENDERS[name])
        return cache[name]
    return get


@pytest.mark.parametrize('name', list(RENDERS))
def test_render_pixels_rows_are_the_full_render_rows(renders, name):
    r = renders(name)
    assert set(r.full) >= {'rgb_map', 'disp_map', 'acc_map', 'pts_max', 'rgb0', 'disp0', 'acc0', 'z_std'}
    for tag in ('1', '65', 'disc', 'P'):
        pix = LISTS_40[tag]
        sel = torch.from_numpy(pix).long().to(dev())
        got = r.pixels(pix)
        assert set(got) == set(r.full), (name, tag)
        for k, v in got.items():
            want = r.full[k][sel]
            assert v.shape == want.shape and v.dtype == want.dtype, (name, tag, k)
            assert torch.equal(torch.isnan(v), torch.isnan(want)), (name, tag, k)
            assert torch.equal(torch.nan_to_num(v, nan=0.), torch.nan_to_num(want, nan=0.)), (name, tag, k)
    got = r.pixels(LISTS_40['disc'], pts_max=False)                                    # run_nerf.render_pixels: the same without pts_max
    assert set(got) == set(r.full) - {'pts_max'}
    assert torch.equal(got['rgb_map'], r.full['rgb_map'][torch.from_numpy(LISTS_40['disc']).long().to(dev())])


def test_render_pixels_of_an_empty_list():
    from nerfail_amd import nerf_to_coord as NC
    focal, K = synth.lego_intrinsics(SIDE, SIDE)
    c2w = torch.from_numpy(synth.pose_spherical(25., -30., 4.))[:3, :4]
    rgb, disp, acc, pts, extras = NC.render_pixels(SIDE, SIDE, K, T(np.zeros(0, np.int32)), chunk=1024, c2w=c2w, **_kwargs(4, 64, (71, 72)))
    assert tuple(rgb.shape) == (0, 3) and tuple(pts.shape) == (0, 3) and tuple(disp.shape) == (0,) and tuple(acc.shape) == (0,) and extras == {}
