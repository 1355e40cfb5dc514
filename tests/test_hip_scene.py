"""-m gpu: scene.build_scene_maps - NeRF to attack-ready views in one call - against the file pipeline it replaces
(nerf_to_coord.render_path -> create_index_and_dist -> dist_to_weight -> GaussNet.load_view_maps), at toy size: every resident
map, every inverted index, the point set and "v"; the save_dir round trip; the attack loops on the returned ids;
perturbation_table; keep_maps=False."""
import os

import numpy as np
import pytest
import torch

import synth
from hiputil import T, N, dev, hip_nerf

pytestmark = pytest.mark.gpu

COUNTS = {'test': 4, 'train': 2, 'val': 1}
ANGLE = {'test': 0., 'train': 90., 'val': 60.}
C = 0.02
LABEL, EPOCHS = 'toy', '%06d' % 3


def _render_kwargs():
    from nerfail_amd import run_nerf as RN
    _, coarse = hip_nerf(4, 64, 71)
    _, fine = hip_nerf(4, 64, 72)
    q = RN.FusedNetworkQuery(RN.get_embedder(10, 0)[0], RN.get_embedder(4, 0)[0])
    return dict(network_query_fn=q, perturb=0., N_importance=8, network_fine=fine, N_samples=8, network_fn=coarse, use_viewdirs=True,
                white_bkgd=True, raw_noise_std=0., ndc=False, lindisp=False, near=2., far=6.)


class Routes:
    """Both routes over the same inputs, run once per view size and left alone."""

    def __init__(self, side, mask_list, base, save):
        from nerfail_amd import GaussNet as G, nerf_to_coord as NC
        from nerfail_amd.create_index_and_dist import create_index_and_dist
        from nerfail_amd.dist_to_weight import dist_to_weight
        from nerfail_amd.scene import build_scene_maps
        self.side, self.mask_list, self.base = side, mask_list, base
        kw = _render_kwargs()
        focal, K = synth.lego_intrinsics(side, side)
        hwf = [side, side, focal]
        self.poses = {s: torch.from_numpy(np.stack([synth.pose_spherical(ANGLE[s] + 40. * i, -30., 4.) for i in range(n)]).astype(np.float32))
                      for s, n in COUNTS.items()}
        self.images = {s: synth.disc_alpha_image(n, side, side, seed=len(s)).astype(np.uint8) for s, n in COUNTS.items()}
        # ---- the file pipeline (NC -> CI -> DW -> load_view_maps)
        self.exp = os.path.join(base, 'logs', 'blender_paper_' + LABEL)
        for s in COUNTS:
            d = os.path.join(self.exp, 'renderonly_%s_%s' % (s, EPOCHS))
            os.makedirs(d)
            with torch.no_grad():
                NC.render_path(self.poses[s], hwf, K, 1024, kw, savedir=d)
        create_index_and_dist(LABEL, EPOCHS, mask_list, basedir=base, train_img_num=COUNTS['train'], val_img_num=COUNTS['val'],
                              test_img_num=COUNTS['test'])
        self.v_files = dist_to_weight(LABEL, basedir=base, test_number=COUNTS['test'], val_number=COUNTS['val'], train_number=COUNTS['train'], c=C)
        self.Ns = len(mask_list) * side * side
        self.file_ids = {s: G.load_view_maps(os.path.join(self.exp, 'index_and_weight', s), list(range(n)), self.Ns,
                                             images={i: self.images[s][i] for i in range(n)}) for s, n in COUNTS.items()}
        # ---- the one call
        self.save_dir = os.path.join(base, 'saved') if save else None
        self.seen = []
        self.maps = build_scene_maps(kw, self.poses, hwf, K, mask_list, c=C, chunk=1024, images=self.images, save_dir=self.save_dir,
                                     on_view=lambda split, i, vid, wi: self.seen.append((split, i, vid, tuple(wi.shape))))
        self.kw, self.hwf, self.K = kw, hwf, K


@pytest.fixture(scope='module')
def grid_routes(tmp_path_factory):
    """40 x 40 views, mask_list [0, 2, 3]: 4 800 points, the fused grid kernel."""
    from nerfail_amd import GaussNet as G
    for c in (G._VIEW_CACHE, G._VIEW_MAPS, G._VIEW_ORI):
        c.clear()
    return Routes(40, [0, 2, 3], str(tmp_path_factory.mktemp('scene40')), save=True)


@pytest.fixture(scope='module')
def brute_routes(tmp_path_factory):
    """20 x 20 views, mask_list [0, 2]: 800 points, the brute-force scan followed by K9."""
    return Routes(20, [0, 2], str(tmp_path_factory.mktemp('scene20')), save=False)


def _same_index(va, vb, what):
    from nerfail_amd import GaussNet as G
    assert (va.Ns, va.P, va.n_entries, va.n_rows) == (vb.Ns, vb.P, vb.n_entries, vb.n_rows) and tuple(va.fp) == tuple(vb.fp), what
    for k in G.ViewIndex.ARRAYS:           # (a view without entries keeps one never-written element per entry array)
        keep = va.n_entries if k in ('packed', 'w_sorted') else None
        assert torch.equal(getattr(va, k)[:keep], getattr(vb, k)[:keep]), (what, k)


def _check_routes_agree(r):
    from nerfail_amd import GaussNet as G
    entries = {s: [] for s in COUNTS}
    m = r.maps
    side = r.side
    assert m.Ns == r.Ns == m.point_set.Ns and m.hw == (side, side) and m.c == C
    tdir = os.path.join(r.exp, 'renderonly_test_%s' % EPOCHS)
    S = np.stack([np.load(os.path.join(tdir, '%03d.npy' % i)) for i in r.mask_list]).reshape(-1, 3)
    assert np.array_equal(N(m.point_set.points), S)                                  # the point set, in mask_list order
    assert (m.point_set._grid is not None) == (r.Ns >= 4096)                          # which path 'auto' took
    assert [(s, i) for s, i, _, _ in r.seen] == [(s, i) for s in ('test', 'train', 'val') for i in range(COUNTS[s])]
    for s, n in COUNTS.items():
        assert m.view_ids[s] == [(m.scene_key, s, i) for i in range(n)]
        for i in range(n):
            ka, kb = G._view_key(m.view_ids[s][i], r.Ns), G._view_key(r.file_ids[s][i], r.Ns)
            wa, wb = G._VIEW_MAPS[ka], G._VIEW_MAPS[kb]
            assert wa.is_cuda and tuple(wa.shape) == (2, side, side, 8)
            assert torch.equal(wa, wb), (s, i)                                        # the resident map, bit for bit
            on_disk = torch.load(os.path.join(r.exp, 'index_and_weight', s, '%d.pth' % i))
            assert torch.equal(wa.cpu(), on_disk)
            _same_index(G._VIEW_CACHE[ka], G._VIEW_CACHE[kb], (s, i))
            entries[s].append(G._VIEW_CACHE[ka].n_entries)
            assert torch.equal(G._VIEW_ORI[ka], G._VIEW_ORI[kb]) and G._VIEW_ORI[ka].dtype == torch.uint8
    print('entries per view (of %d):' % (8 * side * side), entries)
    assert min(entries['test']) > 0 and max(entries['train'] + entries['val']) > 0      # the maps are not all background
    print('v: one call %.9g, file pipeline %.9g, rel %.2e' % (m.v, r.v_files, abs(m.v - r.v_files) / r.v_files))
    assert abs(m.v - r.v_files) <= 1e-5 * r.v_files
    # a view of the point set finds itself at distance 0: weight 1 / (1 + neighbours' g + 0.001) > 0 on its own row
    own = G._VIEW_MAPS[G._view_key(m.view_ids['test'][r.mask_list[1]], r.Ns)]
    assert np.array_equal(N(own[1][..., 0]).reshape(-1), side * side * 1 + np.arange(side * side, dtype=np.float32))
    assert float(own[0][..., 0].min()) > 0


def test_one_call_equals_the_file_pipeline_grid_path(grid_routes):
    """6, 40 x 40 views against 4 800 points."""
    _check_routes_agree(grid_routes)


def test_one_call_equals_the_file_pipeline_brute_path(brute_routes):
    """6, 20 x 20 views against 800 points."""
    _check_routes_agree(brute_routes)


def test_one_call_writes_nothing_unless_asked(brute_routes, grid_routes):
    assert sorted(os.listdir(brute_routes.base)) == ['logs']                              # no save_dir: nothing on disk
    assert sorted(os.listdir(grid_routes.save_dir)) == ['index_and_weight']                # no .npy, no index_and_dist
    for s, n in COUNTS.items():
        assert sorted(os.listdir(os.path.join(grid_routes.save_dir, 'index_and_weight', s))) == sorted(
            ['%d.pth' % i for i in range(n)] + ['%d.idx.pth' % i for i in range(n)])


def _toy_net():
    from nerfail_amd.GaussNet import gauss_net
    w = T(np.random.RandomState(9).normal(size=(8, 48)).astype(np.float32))

    class Cls(torch.nn.Module):
        def forward(self, x):         # evaluated in float64 and rounded once: logits that do not depend on a summation order
            return (torch.nn.functional.adaptive_avg_pool2d(x.double(), 4).reshape(x.shape[0], -1) @ w.double().t()).float()
    return gauss_net(dev(), C, Cls().eval(), 'my_model', epsilon=None)


def test_save_dir_round_trip(grid_routes, monkeypatch):
    """7: the saved maps are the file pipeline's, load_view_maps takes the saved sidecars as they are (no index is built from a
    map), and a NeRFail-S step gives the same table whichever route named its views."""
    from nerfail_amd import GaussNet as G
    from nerfail_amd.attack import nerfail_s_step
    from nerfail_amd.scene import perturbation_table
    r = grid_routes
    built = []
    orig = G.ViewIndex.__init__

    def spy(self, wi_view=None, Ns=None, state=None):
        if wi_view is not None:
            built.append(tuple(wi_view.shape))
        return orig(self, wi_view, Ns, state)
    monkeypatch.setattr(G.ViewIndex, '__init__', spy)
    saved_ids = {}
    for s, n in COUNTS.items():
        d = os.path.join(r.save_dir, 'index_and_weight', s)
        for i in range(n):
            a = torch.load(os.path.join(d, '%d.pth' % i))
            assert not a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (2, r.side, r.side, 8)
            assert torch.equal(a, torch.load(os.path.join(r.exp, 'index_and_weight', s, '%d.pth' % i)))
            side = G.ViewIndex.load(os.path.join(d, '%d.idx.pth' % i))
            assert tuple(side.src) == G._file_sig(os.path.join(d, '%d.pth' % i)) and side.Ns == r.Ns
        saved_ids[s] = G.load_view_maps(d, list(range(n)), r.Ns, images={i: r.images[s][i] for i in range(n)})
    assert built == []                                                 # every sidecar was accepted
    net = _toy_net()
    s0 = perturbation_table(r.images['test'][r.mask_list])
    out = []
    for ids in (saved_ids, r.maps.view_ids, r.file_ids):
        vids = ids['train'] + ids['val']
        s = s0
        for _ in range(2):
            s, loss = nerfail_s_step(net, s, s0, None, None, torch.tensor(3, device=dev()), a=2.0, epsilon=32.0, view_ids=vids)
        out.append(s)
    assert built == []
    assert torch.equal(out[0], out[1]) and torch.equal(out[1], out[2]) and not torch.equal(out[0], s0)


def test_the_attack_takes_the_ids(grid_routes):
    """8: attack.nerfail_s over the three train / val views named by build_scene_maps, from perturbation_table of the base
    images: the same `best`, bit for bit, as the run fed with the file pipeline's maps."""
    from nerfail_amd.attack import nerfail_s
    from nerfail_amd.scene import perturbation_table
    r = grid_routes
    s0 = perturbation_table(r.images['test'][r.mask_list])
    assert tuple(s0.shape) == (3, r.side, r.side, 4) and s0.numel() // 4 == r.maps.Ns
    batches = r.maps.batches(('train', 'val'), 2)
    assert [len(b[2]) for b in batches] == [2, 1] and batches[0][0] is None
    got = nerfail_s(_toy_net(), s0, batches, 3, 2, a=2., epsilon=32., log=None)
    fids = r.file_ids['train'] + r.file_ids['val']
    want = nerfail_s(_toy_net(), s0, [(None, None, fids[:2]), (None, None, fids[2:])], 3, 2, a=2., epsilon=32., log=None)
    assert torch.equal(got.best, want.best) and torch.equal(got.last, want.last)
    assert not torch.equal(got.best, s0) and got.best_epoch == 0
    assert [d['views'] for d in got.stats] == [3, 3] and got.stats == want.stats


def _restated(imgs, zero_init, rand_init):
    """AS:252-263."""
    t = torch.stack([torch.as_tensor(i) for i in imgs]).to(dev()).float()
    if rand_init:
        r = torch.rand_like(t) * 255
        t = torch.where(t[:, :, :, 3].unsqueeze(-1) > 0, r, t)
    if zero_init:
        z = torch.zeros_like(t)
        z[:, :, :, 3] = t[:, :, :, 3]
        t = z
    return t


def test_perturbation_table():
    """9."""
    from nerfail_amd.scene import perturbation_table
    imgs = synth.disc_alpha_image(3, 13, 11, seed=7).astype(np.uint8)
    for zero, rand in ((True, False), (False, True), (True, True), (False, False)):
        torch.manual_seed(5)
        want = _restated(imgs, zero, rand)
        outs = []
        for form in (imgs, imgs.astype(np.float32), [imgs[i] for i in range(3)], torch.from_numpy(imgs), T(imgs.astype(np.float32))):
            torch.manual_seed(5)
            outs.append(perturbation_table(form, zero_init=zero, rand_init=rand))
        for o in outs:
            assert o.is_cuda and o.dtype == torch.float32 and tuple(o.shape) == (3, 13, 11, 4) and torch.equal(o, want), (zero, rand)
    z = perturbation_table(imgs)
    assert float(z[..., :3].abs().max()) == 0 and np.array_equal(N(z[..., 3]), imgs[..., 3].astype(np.float32))
    gen = torch.Generator(device=dev())
    a = perturbation_table(imgs, zero_init=False, rand_init=True, generator=gen.manual_seed(3))
    b = perturbation_table(imgs, zero_init=False, rand_init=True, generator=gen.manual_seed(3))
    opaque = imgs[..., 3] > 0
    assert torch.equal(a, b) and np.array_equal(N(a)[~opaque], imgs.astype(np.float32)[~opaque])
    assert 0 <= float(a[T(opaque)].min()) and float(a[T(opaque)].max()) < 255 and len(np.unique(N(a)[opaque])) > 100
    with pytest.raises(ValueError, match='BGRA'):
        perturbation_table(imgs[..., :3])


def test_keep_maps_false(grid_routes):
    """10: only the inverted index and the image stay; a forward by id says so instead of faulting."""
    from nerfail_amd import GaussNet as G
    from nerfail_amd.scene import build_scene_maps
    r = grid_routes
    seen = []
    m = build_scene_maps(r.kw, {'val': r.poses['val']}, r.hwf, r.K, None, c=C, chunk=1024, images={'val': r.images['val']},
                         point_set=r.maps.point_set, keep_maps=False, on_view=lambda s, i, vid, wi: seen.append(wi))
    assert m.point_set is r.maps.point_set and list(m.view_ids) == ['val'] and m.scene_key != r.maps.scene_key
    key = G._view_key(m.view_ids['val'][0], r.Ns)
    assert key not in G._VIEW_MAPS and key in G._VIEW_CACHE and key in G._VIEW_ORI
    _same_index(G._VIEW_CACHE[key], G._VIEW_CACHE[G._view_key(r.maps.view_ids['val'][0], r.Ns)], 'val')
    assert torch.equal(seen[0], G._VIEW_MAPS[G._view_key(r.maps.view_ids['val'][0], r.Ns)])
    s = torch.zeros((3, r.side, r.side, 4), device=dev())
    with pytest.raises(KeyError, match='not resident and no weight_and_index_list'):
        G.gauss_gather(s, None, None, view_ids=m.view_ids['val'])
    x, xr = G.gauss_gather(s, seen[0].unsqueeze(0), None, view_ids=m.view_ids['val'])      # with the map at hand it runs, on the cached index
    assert torch.isfinite(xr).all()


def test_only_the_index_counts_cross_to_the_host(grid_routes, monkeypatch):
    """Per view the call reads what ViewIndex's build reads (the map's fingerprint, two counts), and `v` once at the end."""
    from nerfail_amd.scene import build_scene_maps
    r = grid_routes
    reads = []
    for n in ('cpu', 'item', 'tolist', 'numpy', '__int__', '__float__', '__bool__', '__index__'):
        def f(self, *a, _orig=getattr(torch.Tensor, n), _n=n, **k):
            if self.is_cuda:
                reads.append((_n, self.numel()))
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, n, f)
    poses = {'test': r.poses['test'][:1], 'train': r.poses['train']}
    m = build_scene_maps(r.kw, poses, r.hwf, r.K, None, c=C, chunk=1024, point_set=r.maps.point_set)
    monkeypatch.undo()
    assert len(m.view_ids['test']) == 1 and len(m.view_ids['train']) == 2
    assert max(n for _, n in reads) <= 2 and len(reads) == 3 * 3 + 1, reads
