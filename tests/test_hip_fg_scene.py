"""-m gpu: scene.build_scene_maps(foreground_only=True) against the full call over the same inputs, at toy size (the setup of
test_hip_scene.py: 40 x 40 views, test 4 / train 2 / val 1, mask_list [0, 2, 3], disc images; one train view has an all-zero
alpha). The contract: the same point set and Ns; every map == where(alpha > 0, M_full, 0), bit for bit; what the attacks read
from a view - its inverted index, gauss_net's x_rgba and logits, a NeRFail-S run - is what the masked full map gives, and
x_rgba / logits are the full map's. Every comparison is an ==."""
import os

import numpy as np
import pytest
import torch

import synth
from hiputil import T, N, dev, hip_nerf

pytestmark = pytest.mark.gpu

COUNTS = {'test': 4, 'train': 2, 'val': 1}
ANGLE = {'test': 0., 'train': 90., 'val': 60.}
C, SIDE, MASK = 0.02, 40, [0, 2, 3]
EMPTY = ('train', 1)                       # the view without foreground


def _render_kwargs():
    from nerfail_amd import run_nerf as RN
    _, coarse = hip_nerf(4, 64, 71)
    _, fine = hip_nerf(4, 64, 72)
    q = RN.FusedNetworkQuery(RN.get_embedder(10, 0)[0], RN.get_embedder(4, 0)[0])
    return dict(network_query_fn=q, perturb=0., N_importance=8, network_fine=fine, N_samples=8, network_fn=coarse, use_viewdirs=True,
                white_bkgd=True, raw_noise_std=0., ndc=False, lindisp=False, near=2., far=6.)


class Both:
    """The full call and the foreground-only call over the same inputs, run once and left alone."""

    def __init__(self, base):
        from nerfail_amd import GaussNet as G
        from nerfail_amd.scene import build_scene_maps
        for c in (G._VIEW_CACHE, G._VIEW_MAPS, G._VIEW_ORI):
            c.clear()
        self.kw = _render_kwargs()
        focal, self.K = synth.lego_intrinsics(SIDE, SIDE)
        self.hwf = [SIDE, SIDE, focal]
        self.poses = {s: torch.from_numpy(np.stack([synth.pose_spherical(ANGLE[s] + 40. * i, -30., 4.) for i in range(n)]).astype(np.float32))
                      for s, n in COUNTS.items()}
        self.images = {s: synth.disc_alpha_image(n, SIDE, SIDE, seed=len(s)).astype(np.uint8) for s, n in COUNTS.items()}
        self.images[EMPTY[0]][EMPTY[1], ..., 3] = 0
        self.full_maps, self.fg_maps = {}, {}
        self.full = build_scene_maps(self.kw, self.poses, self.hwf, self.K, MASK, c=C, chunk=1024, images=self.images,
                                     on_view=lambda s, i, vid, wi: self.full_maps.__setitem__((s, i), wi.clone()))
        self.save_dir = os.path.join(base, 'saved')
        self.fg = build_scene_maps(self.kw, self.poses, self.hwf, self.K, MASK, c=C, chunk=1024, images=self.images, save_dir=self.save_dir,
                                   foreground_only=True, on_view=lambda s, i, vid, wi: self.fg_maps.__setitem__((s, i), wi.clone()))
        self.Ns = len(MASK) * SIDE * SIDE
        # ids registered from the masked full maps: what the foreground-only views must be indistinguishable from
        self.masked, self.masked_ids = {}, {s: [] for s in COUNTS}
        for (s, i), wi in self.full_maps.items():
            m = torch.where(T(self.images[s][i][..., 3] > 0)[None, :, :, None], wi, torch.zeros_like(wi))
            self.masked[(s, i)] = m
            G.register_view(('masked', s, i), self.Ns, m, self.images[s][i])
            self.masked_ids[s].append(('masked', s, i))


@pytest.fixture(scope='module')
def both(tmp_path_factory):
    return Both(str(tmp_path_factory.mktemp('fgscene')))


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_point_set_counts_and_v(both):
    b = both
    assert b.fg.Ns == b.full.Ns == b.Ns and torch.equal(b.fg.point_set.points, b.full.point_set.points)
    assert b.fg.point_set._grid is not None                                             # 4 800 points: the list kernel ran
    alpha_counts = {s: [int((b.images[s][i][..., 3] > 0).sum()) for i in range(n)] for s, n in COUNTS.items()}
    assert b.fg.rendered == alpha_counts and b.fg.rendered[EMPTY[0]][EMPTY[1]] == 0
    assert b.full.rendered == {s: [SIDE * SIDE] * n for s, n in COUNTS.items()}
    assert all(0 < n < SIDE * SIDE for s in COUNTS for i, n in enumerate(alpha_counts[s]) if (s, i) != EMPTY)
    assert list(b.fg.view_ids) == list(b.full.view_ids) and b.fg.hw == (SIDE, SIDE)
    # v: the mean over the views with foreground of the mean squared distance of their foreground pixels (from the full maps'
    # distances: the float32 squares added in double)
    from nerfail_amd.scene import view_map
    from nerfail_amd.create_index_and_dist import knn8
    from nerfail_amd import nerf_to_coord as NC
    terms = []
    for s, n in COUNTS.items():
        for i in range(n):
            a = b.images[s][i][..., 3].reshape(-1) > 0
            if a.sum() == 0:
                continue
            with torch.no_grad():
                pts = NC.render(SIDE, SIDE, b.K, chunk=1024, c2w=b.poses[s][i][:3, :4], **b.kw)[3]
            d = N(knn8(pts.reshape(SIDE, SIDE, 3), b.full.point_set.points, method='grid')[0]).reshape(-1, 8)[a].reshape(-1)
            terms.append(float((d * d).astype(np.float32).astype(np.float64).sum()) / (8 * int(a.sum())))
    want = sum(terms) / len(terms)
    print('v: foreground-only %.12g, restated %.12g; full call %.12g' % (b.fg.v, want, b.full.v))
    assert len(terms) == 6 and abs(b.fg.v - want) <= 1e-10 * want


def test_every_map_is_the_masked_full_map(both):
    from nerfail_amd import GaussNet as G
    b = both
    assert sorted(b.fg_maps) == sorted(b.full_maps) and len(b.fg_maps) == 7
    for (s, i), wi in b.fg_maps.items():
        assert tuple(wi.shape) == (2, SIDE, SIDE, 8) and wi.dtype == torch.float32
        assert torch.equal(_bits(wi), _bits(b.masked[(s, i)])), (s, i)                   # base views (test 0, 2, 3) included
        resident = G._VIEW_MAPS[G._view_key(b.fg.view_ids[s][i], b.Ns)]
        assert torch.equal(_bits(resident), _bits(wi)), (s, i)
    z = b.fg_maps[EMPTY]
    assert not bool(_bits(z).any())                                                     # no foreground: a zero map
    assert bool((b.masked[('test', 0)][0] > 0).any())                                   # ... and the others are not


def test_saved_maps_load_as_they_are(both, monkeypatch):
    from nerfail_amd import GaussNet as G
    b = both
    built = []
    orig = G.ViewIndex.__init__

    def spy(self, wi_view=None, Ns=None, state=None):
        if wi_view is not None:
            built.append(tuple(wi_view.shape))
        return orig(self, wi_view, Ns, state)
    monkeypatch.setattr(G.ViewIndex, '__init__', spy)
    for s, n in COUNTS.items():
        d = os.path.join(b.save_dir, 'index_and_weight', s)
        for i in range(n):
            a = torch.load(os.path.join(d, '%d.pth' % i))
            assert not a.is_cuda and a.dtype == torch.float32 and torch.equal(_bits(a), _bits(b.fg_maps[(s, i)].cpu())), (s, i)
        ids = G.load_view_maps(d, list(range(n)), b.Ns, images={i: b.images[s][i] for i in range(n)})
        for i, vid in enumerate(ids):
            assert torch.equal(_bits(G._VIEW_MAPS[G._view_key(vid, b.Ns)]), _bits(b.fg_maps[(s, i)])), (s, i)
    assert built == []                                                                  # every saved sidecar was accepted


def test_every_view_index_is_the_masked_maps(both):
    from nerfail_amd import GaussNet as G
    b = both
    for s, n in COUNTS.items():
        for i in range(n):
            va = G._VIEW_CACHE[G._view_key(b.fg.view_ids[s][i], b.Ns)]
            vb = G._VIEW_CACHE[G._view_key(b.masked_ids[s][i], b.Ns)]
            assert (va.Ns, va.P, va.n_entries, va.n_rows) == (vb.Ns, vb.P, vb.n_entries, vb.n_rows) and tuple(va.fp) == tuple(vb.fp), (s, i)
            for k in G.ViewIndex.ARRAYS:       # (a view without entries keeps one never-written element per entry array)
                keep = va.n_entries if k in ('packed', 'w_sorted') else None
                assert torch.equal(getattr(va, k)[:keep], getattr(vb, k)[:keep]), (s, i, k)
    assert G._VIEW_CACHE[G._view_key(b.fg.view_ids[EMPTY[0]][EMPTY[1]], b.Ns)].n_entries == 0


def _toy_net():
    from nerfail_amd.GaussNet import gauss_net
    w = T(np.random.RandomState(9).normal(size=(8, 48)).astype(np.float32))

    class Cls(torch.nn.Module):
        def forward(self, x):         # evaluated in float64 and rounded once: logits that do not depend on a summation order
            return (torch.nn.functional.adaptive_avg_pool2d(x.double(), 4).reshape(x.shape[0], -1) @ w.double().t()).float()
    return gauss_net(dev(), C, Cls().eval(), 'my_model', epsilon=None)


def test_gauss_net_forward_is_the_full_maps(both):
    """x_rgba and the logits on a seeded table: the foreground-only ids against the FULL ids (gauss_net writes 0 wherever the
    image's alpha is <= 0, so the rows that differ are never seen)."""
    b = both
    table = T(np.random.RandomState(3).uniform(-30, 30, (len(MASK), SIDE, SIDE, 4)).astype(np.float32))
    out = {}
    for tag, ids in (('fg', b.fg.view_ids), ('full', b.full.view_ids)):
        net = _toy_net()
        vids = ids['test'] + ids['train'] + ids['val']
        with torch.no_grad():
            x, x_rgba, cla, ori, ori_cla = net(table, None, None, view_ids=vids)
        out[tag] = (x_rgba, cla, ori_cla)
    for a, f in zip(out['fg'], out['full']):
        assert a.shape == f.shape and torch.equal(_bits(a), _bits(f))
    assert bool((out['fg'][0][..., :3] != 0).any())


def test_nerfail_s_on_the_foreground_ids(both):
    from nerfail_amd.attack import nerfail_s
    from nerfail_amd.scene import perturbation_table
    b = both
    s0 = perturbation_table(b.images['test'][MASK])
    runs = []
    for ids in (b.fg.view_ids, b.masked_ids):
        vids = ids['train'] + ids['val']
        runs.append(nerfail_s(_toy_net(), s0, [(None, None, vids[:2]), (None, None, vids[2:])], 3, 2, a=2., epsilon=32., log=None))
    got, want = runs
    assert torch.equal(_bits(got.best), _bits(want.best)) and torch.equal(_bits(got.last), _bits(want.last))
    assert not torch.equal(got.last, s0) and got.stats == want.stats
