"""-m gpu: nerfail_knn8_grid_weights[_view] - the 8-NN search with the Gaussian weights as its epilogue - against the chain it
replaces, nerfail_knn8_grid_search[_view] followed by nerfail_gauss_weight: both planes bit for bit, sum_d2 against the float64
sum of the chain's float32 squares, and the refusals of the C ABI."""
import ctypes

import numpy as np
import pytest
import torch

import synth
from hiputil import T, N, dev

pytestmark = pytest.mark.gpu

CS = (0.02, 0.002, 0.5)
VIEWS = ((37, 53), (8, 8), (9, 130), (40, 40))


def chain(Q, S, c, method='grid'):
    """(weight_and_index [2,...,8], dist [...,8]) the way the file pipeline forms them: knn8, then create_gauss_w."""
    from nerfail_amd.create_index_and_dist import knn8
    from nerfail_amd.GaussNet import create_gauss_w
    d, i = knn8(Q, S, method=method)
    lead = tuple(d.shape[:-1])
    dai = torch.stack([d, i], 0).reshape(1, 2, -1, 1, 8)
    wi, _ = create_gauss_w(dev(), c)(dai)
    return wi[0].reshape((2,) + lead + (8,)), d


def fused(Q, S, c, want_d2=True, flat=False):
    """The C entry points over a grid built here: (weight_and_index, sum_d2 tensor or None)."""
    from nerfail_amd import _lib
    from nerfail_amd.create_index_and_dist import _grid_for
    lib = _lib.load()
    ws, nbytes = _grid_for(S)
    q = Q.reshape(-1, 3) if flat else Q
    n = q.numel() // 3
    out = torch.full((2,) + tuple(q.shape[:-1]) + (8,), float('nan'), dtype=torch.float32, device=dev())
    d2 = torch.full((1,), float('nan'), dtype=torch.float64, device=dev()) if want_d2 else None
    wb = lib.nerfail_knn8_grid_weights_workspace_bytes(n)
    work = torch.empty((wb // 8,), dtype=torch.float64, device=dev())
    d2p = ctypes.c_void_p(d2.data_ptr()) if want_d2 else None
    if flat:
        _lib.check(lib.nerfail_knn8_grid_weights(_lib.dev(q), n, S.shape[0], c, _lib.dev(out), d2p, _lib.dev(ws), nbytes,
                                                 ctypes.c_void_p(work.data_ptr()), wb, _lib.stream()))
    else:
        _lib.check(lib.nerfail_knn8_grid_weights_view(_lib.dev(q), q.shape[0], q.shape[1], S.shape[0], c, _lib.dev(out), d2p, _lib.dev(ws), nbytes,
                                                      ctypes.c_void_p(work.data_ptr()), wb, _lib.stream()))
    return out, d2


@pytest.fixture(scope='module')
def S():
    """Three 64 x 64 views of the rough sphere: 12 288 points (the grid path of the 'auto' rule)."""
    return T(np.stack([synth.sphere_view_points(64, 64, th) for th in (-120., 0., 120.)]).reshape(-1, 3))


def _view(H, W):
    """The top-left H x W window of a square view of the rough sphere, as test_knn_view_tiles_cover_odd_sizes_and_equal_the_flat_search
    cuts it. Share of its pixels farther than 0.5 from every point of S (other views' near-plane points lie close to some of
    this view's): 0.27 / 0.39 / 0.49 / 0.35 for VIEWS."""
    m = max(H, W)
    return T(synth.sphere_view_points(m, m, 45.)[:H, :W].copy())


@pytest.fixture(scope='module')
def chains(S):
    """The chain's result per (view, c), computed once and left alone."""
    return {(hw, c): chain(_view(*hw), S, c) for hw in VIEWS for c in CS}


@pytest.mark.parametrize('hw', VIEWS)
def test_fused_call_equals_the_chain_bitwise(S, chains, hw):
    """1: partial tiles with repeated lanes (37 x 53, 9 x 130), the one-tile view (8 x 8), whole tiles (40 x 40); c from far
    below to far above the neighbour spacing; the tiled and the flat entry. On the background pixels of the view (the far-query
    path) every g_k underflows: all eight weights are exactly 0."""
    Q = _view(*hw)
    for c in CS:
        want, dist = chains[(hw, c)]
        got, _ = fused(Q, S, c)
        assert not torch.isnan(got).any()                                   # every pixel of both planes written
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (hw, c)
        flat, _ = fused(Q, S, c, flat=True)
        assert torch.equal(flat.reshape(got.shape), want), (hw, c)
    far = dist[..., 0] > 0.5
    assert 0.2 < float(far.float().mean()) < 0.8, float(far.float().mean())            # the far-query branch really ran
    for c in (0.02, 0.002):                 # (at c = 0.5 a distance of one unit still weighs exp(-2))
        w = chains[(hw, c)][0][0]
        assert bool((w[far] == 0).all()) and bool((fused(Q, S, c)[0][0][far] == 0).all())
    assert float(chains[(hw, 0.5)][0][0][far].min()) > 0


def test_op_and_view_map_take_the_same_kernel(S, chains):
    """torch.ops.nerfail_mi.knn8_weights and scene.view_map over a PointSet: the chain's bits on the grid path."""
    from nerfail_amd.scene import PointSet, view_map
    ps = PointSet(S)
    for hw in ((37, 53), (40, 40)):
        Q = _view(*hw)
        want, dist = chains[(hw, 0.02)]
        wi, d2 = torch.ops.nerfail_mi.knn8_weights(Q, S, 0.02)
        assert torch.equal(wi, want) and d2.dtype == torch.float64
        wm, d2m = view_map(Q, ps, 0.02)
        assert torch.equal(wm, want) and float(d2m) == float(d2[0])
        wb, d2b = view_map(Q, ps, 0.02, method='brute')
        assert torch.equal(wb, want)
        assert abs(float(d2b) - float(d2m)) <= 1e-12 * float(d2m)


def test_scene_op_passes_opcheck(S):
    from nerfail_amd import ops as O
    assert O.SCENE_OPS == ('knn8_weights',)
    small = T(synth.sphere_shell_points(500, seed=3))
    for args in ((_view(9, 130), S, 0.02), (_view(9, 130).reshape(-1, 3), S, 0.02), (_view(8, 8), small, 0.5)):
        torch.library.opcheck(torch.ops.nerfail_mi.knn8_weights.default, args,
                              test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_dynamic'))
    wi, d2 = torch.ops.nerfail_mi.knn8_weights(_view(8, 8), small, 0.5)           # below 4 096 points: the brute-force scan + K9
    want, dist = chain(_view(8, 8), small, 0.5, method='brute')
    assert torch.equal(wi, want) and float(d2[0]) == float(torch.square(dist).sum(dtype=torch.float64))


def test_exact_hits_and_exact_ties():
    """2: queries that are rows of the set (d = 0, g = 1) and a set with duplicated rows (ties broken by index)."""
    rs = np.random.RandomState(5)
    base = synth.sphere_shell_points(3000, seed=11)
    Snp = np.concatenate([base, base[:1500], base[100:200]]).astype(np.float32)         # 4 600 points, 1 500 of them 2x, 100 3x
    Snp = Snp[rs.permutation(len(Snp))]
    St = T(Snp)
    Q = T(Snp[rs.randint(0, len(Snp), 24 * 24)].reshape(24, 24, 3))
    for c in CS:
        want, dist = chain(Q, St, c)
        wantb, _ = chain(Q, St, c, method='brute')
        assert torch.equal(want, wantb)
        for flat in (False, True):
            got, _ = fused(Q, St, c, flat=flat)
            assert torch.equal(got.reshape(want.shape), want), (c, flat)
        assert float(dist[..., 0].max()) == 0.0                                           # every query finds itself
        twice = dist[..., 1] == 0
        assert 0.2 < float(twice.float().mean()) < 0.9                                    # exact ties are present ...
        idx = want[1]
        assert bool((idx[..., 0][twice] < idx[..., 1][twice]).all())                      # ... and broken by index
        # the zero-distance weight is 1 / (sum g + 0.001), formed as the chain forms it (float32, k = 0..7 order)
        d = N(dist).reshape(-1, 8)
        q = d / np.float32(c)
        g = np.exp(-((q * q) / np.float32(2.0)).astype(np.float64))
        w0 = 1.0 / (g.sum(1) + 0.001)
        assert np.allclose(N(got[0]).reshape(-1, 8)[:, 0], w0, rtol=2e-6, atol=0)


def test_fused_map_holds_the_reference_bounds_on_g17(golden):
    """3: on fixture g17 the fused map is bitwise the chain's, so K10 on it stays inside the bounds
    test_knn_pipeline_vs_reference_chain asserts for the chain. 3 072 points: below the 4 096-point rule, the grid entry
    is called directly."""
    from test_oracle_knn import agreement_with_reference, pipeline_deviation
    from nerfail_amd.GaussNet import gauss_gather
    g = golden('g17_knn_pipeline')
    Q, St = T(g['Q']), T(g['S'])
    assert tuple(Q.shape) == (32, 32, 3) and St.shape[0] == 3072
    want, dist = chain(Q, St, 0.02)
    got, _ = fused(Q, St, 0.02)
    assert torch.equal(got, want)
    x, _ = gauss_gather(T(g['s']), got.unsqueeze(0), T(g['ori']), None)
    frac, worst = pipeline_deviation(N(x), g['ref_x'])
    ref = g['ref_dist_and_index']
    m = agreement_with_reference(N(dist).reshape(-1, 8), N(got[1]).reshape(-1, 8).astype(np.int64),
                                 ref[0].reshape(-1, 8), ref[1].reshape(-1, 8).astype(np.int64))
    print('fused K8+K9 -> K10 vs reference chain: sets %.4f, pixels with |dx| > 1e-4 max|x|: %.4f (worst %.3e)' % (m['sets'], frac, worst))
    assert m['sets'] > 0.97 and frac < 0.03 and worst < 0.05


@pytest.mark.parametrize('hw', VIEWS)
def test_sum_d2(S, chains, hw):
    """4: sum_d2 against the float64 numpy sum of the chain's float32 squares (1e-12: both are double sums of the same terms),
    the same bits on a second run, the mean within 1e-5 of torch's float32 mean of squares, and NULL accepted."""
    Q = _view(*hw)
    want, dist = chains[(hw, 0.02)]
    d = N(dist).reshape(-1)
    ref = float((d * d).astype(np.float32).astype(np.float64).sum())
    for flat in (False, True):
        _, a = fused(Q, S, 0.02, flat=flat)
        _, b = fused(Q, S, 0.02, flat=flat)
        a, b = N(a), N(b)
        print('%s flat=%s sum_d2 %.17g reference %.17g rel %.3e' % (hw, flat, a[0], ref, abs(a[0] - ref) / ref))
        assert a.tobytes() == b.tobytes()
        assert abs(a[0] - ref) <= 1e-12 * ref
        mean = float(torch.mean(torch.square(dist)))
        assert abs(a[0] / d.size - mean) <= 1e-5 * mean
    got, none = fused(Q, S, 0.02, want_d2=False)
    assert none is None and torch.equal(got, want)


def test_argument_errors_launch_nothing(S):
    """5: every refusal returns NERFAIL_EINVAL with a message before anything is launched - the outputs keep their NaN fill."""
    from nerfail_amd import _lib
    from nerfail_amd.create_index_and_dist import _grid_for
    lib = _lib.load()
    Q = _view(37, 53)
    ws, nbytes = _grid_for(S)
    n, M = 37 * 53, S.shape[0]
    out = torch.full((2 * n * 8 + 4,), float('nan'), dtype=torch.float32, device=dev())
    d2 = torch.full((1,), float('nan'), dtype=torch.float64, device=dev())
    wb = lib.nerfail_knn8_grid_weights_workspace_bytes(n)
    work = torch.empty((wb // 8,), dtype=torch.float64, device=dev())
    P = ctypes.c_void_p

    def view(c=0.02, o=out.data_ptr(), m=M, gb=nbytes, w=wb, grid=ws.data_ptr()):
        return lib.nerfail_knn8_grid_weights_view(_lib.dev(Q), 37, 53, m, c, P(o), P(d2.data_ptr()), P(grid), gb, P(work.data_ptr()), w, _lib.stream())

    def flat(c=0.02, o=out.data_ptr(), m=M, gb=nbytes, w=wb, grid=ws.data_ptr()):
        return lib.nerfail_knn8_grid_weights(_lib.dev(Q), n, m, c, P(o), P(d2.data_ptr()), P(grid), gb, P(work.data_ptr()), w, _lib.stream())
    cases = ((dict(c=0.0), b'c must be positive'), (dict(c=-1.0), b'c must be positive'),
             (dict(o=out.data_ptr() + 4), b'16-byte aligned'),
             (dict(w=wb - 8), b'workspace too small'), (dict(gb=nbytes - 1), b'grid workspace too small'),
             (dict(m=M - 1), b'does not match the grid'), (dict(m=M - 4096), b'does not match the grid'),
             (dict(m=M + 4096), b'grid workspace too small'))
    for call in (view, flat):
        for kw, word in cases:
            assert call(**kw) == 1, kw                                                    # NERFAIL_EINVAL
            msg = lib.nerfail_last_error()
            assert word in msg, (kw, msg)
    # a workspace that is large enough for a larger set, but was BUILT for M points
    big = lib.nerfail_knn8_grid_workspace_bytes(M + 4096)
    ws2 = torch.empty((big,), dtype=torch.uint8, device=dev())
    _lib.check(lib.nerfail_knn8_grid_build(_lib.dev(S), M, _lib.dev(ws2), big, _lib.stream()))
    assert view(m=M + 4096, gb=big, grid=ws2.data_ptr()) == 1 and b'does not match the grid' in lib.nerfail_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(d2).all())
    assert view(gb=big, grid=ws2.data_ptr()) == 0                                           # ... and the good call still works
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:2 * n * 8]).any()) and bool(torch.isnan(out[2 * n * 8:]).all()) and not bool(torch.isnan(d2).any())
    from nerfail_amd.scene import PointSet, view_map
    with pytest.raises(_lib.NerfailError, match='c must be positive'):
        view_map(Q, PointSet(S), 0.0)
    with pytest.raises(ValueError, match=r'\[H,W,3\]'):
        view_map(Q.reshape(-1, 3), PointSet(S))
