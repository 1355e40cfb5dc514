"""Scene maps in one call: a trained NeRF to attack-ready views, on the device.

The reference turns a NeRF into the pixel <-> 3-D-point maps of its attacks with three scripts glued together by the disk:
nerf_to_coord.py (NC: one `NNN.npy` point image per view), create_index_and_dist.py (CI: `index_and_dist/<split>/<i>.pth`)
and tools/dist_to_weight.py (DW: `index_and_weight/<split>/<i>.pth`), which the attack's dataset then loads back. The mirrors of
those scripts (nerf_to_coord.render_path, create_index_and_dist, dist_to_weight, GaussNet.load_view_maps) keep that file
contract. `build_scene_maps` is the same stage as a product: render (ends on the device) -> `view_map` (the 8-NN search with
the Gaussian weights as its epilogue, one launch) -> `GaussNet.register_view` (the map, the image and the inverted index stay
resident under a view id) - the ids it returns are what attack.nerfail_s / attack.nerfail / nerfail_s_step take as `view_ids=`.
Nothing is written unless `save_dir` asks for it, and every map is bit for bit the file pipeline's.
`foreground_only=True` (opt-in) renders and searches only the pixels the attacks read - alpha > 0 in the view's image:
`foreground_pixels` -> nerf_to_coord.render_pixels -> `view_map_pixels`; the maps are then the file pipeline's on those pixels and zero
elsewhere.
`shard_batch=B` (opt-in, under torch.distributed) builds the scene once across the ranks: the base views by pixel range, every
other view on the rank the attack's batches of B hand it to (sharding.batch_owner); the results are the one-rank call's bits.
Executed with gloo ranks sharing one device; no speed-up was measured on several devices.
"""
import itertools
import os

import numpy as np
import torch

from . import _lib
from . import ops
from . import GaussNet as _G
from . import nerf_to_coord as _NC
from . import sharding
from .create_index_and_dist import _grid_for, knn8
from .run_nerf_helpers import _cuda
from .views import _file_sig

GRID_FROM = 4096          # the 'auto' rule of create_index_and_dist.knn8: grid search from this many points up
SPLITS = ('test', 'train', 'val')     # CI:110

_scene_counter = itertools.count()


class PointSet:
    """The spatial point set of a scene (CI:57-61): `points` [M,3] on the device, `Ns` = M rows of the perturbation table.
    From GRID_FROM points up it owns the search grid (create_index_and_dist._grid_for), built once."""

    def __init__(self, points):
        dev = _cuda()
        self.points = _lib.f32c(torch.as_tensor(points), dev).reshape(-1, 3)
        self.Ns = int(self.points.shape[0])
        if self.Ns < 8:
            raise _lib.NerfailError('PointSet: need at least 8 points (got %d)' % self.Ns)
        self._grid = None
        if self.Ns >= GRID_FROM:
            self.grid()

    def grid(self):
        """(workspace, bytes) of the built grid; held here, so the cache of _grid_for may forget it."""
        if self._grid is None:
            self._grid = _grid_for(self.points)
        return self._grid

    @classmethod
    def from_views(cls, pts_list):
        """The [H,W,3] point images of the base views, stacked in list order (CI:57-61)."""
        dev = _cuda()
        return cls(torch.reshape(torch.stack([_lib.f32c(torch.as_tensor(p), dev) for p in pts_list]), (-1, 3)))

    @classmethod
    def from_render(cls, render_kwargs, poses, hwf, K, chunk=1024 * 32):
        """Renders the base views `poses` [n,4,4] (nerf_to_coord.render) and stacks their pts_max."""
        return cls.from_views([_render_pts(render_kwargs, c2w, hwf, K, chunk) for c2w in poses])


def _render_pts(render_kwargs, c2w, hwf, K, chunk):
    """pts_max [H,W,3] of one view, on the device (NC:160: the render of render_path, without its host copies)."""
    H, W = int(hwf[0]), int(hwf[1])
    c2w = torch.as_tensor(c2w)
    with torch.no_grad():                                  # as the reference renders (NC:640)
        pts_max = _NC.render(H, W, K, chunk=chunk, c2w=c2w[:3, :4], **render_kwargs)[3]
    return pts_max.reshape(H, W, 3)


def _render_pts_sharded(render_kwargs, c2w, hwf, K, chunk, rank, world, group):
    """_render_pts across the ranks of `group`: this rank renders its pixel range (sharding.render_shard: the slices concatenate
    bit for bit to the full render), the ranges are exchanged (sharding.all_gather_ranges_), every rank returns the same [H,W,3]."""
    H, W = int(hwf[0]), int(hwf[1])
    kw = {k: v for k, v in render_kwargs.items() if k not in ('near', 'far')}
    with torch.no_grad():
        (lo, hi), ret = sharding.render_shard(H, W, K, torch.as_tensor(c2w)[:3, :4], render_kwargs.get('near', 0.), render_kwargs.get('far', 1.),
                                              rank, world, chunk, **kw)
    pts = torch.empty((H * W, 3), dtype=torch.float32, device=_cuda())
    if hi > lo:
        pts[lo:hi] = ret['pts_max']
    sharding.all_gather_ranges_(pts, sharding.shard_ranges(H * W, world), group)
    return pts.reshape(H, W, 3)


def view_map(pts_max, point_set, c=0.02, method='auto'):
    """One view: pts_max [H,W,3] against the point set -> (weight_and_index [2,H,W,8], sum_d2), both on the device.

    The map is bit for bit create_index_and_dist.index_and_dist followed by create_gauss_w(c) (CI:126-163, DW:82-97); sum_d2 (a
    0-dim float64 tensor) is the sum over the view's 8 H W distances of the float32 square DW:92 takes, added in double.
    method 'auto': from GRID_FROM points up the fused kernel (nerfail_knn8_grid_weights_view: no distance tensor is written),
    below that the brute-force scan followed by K9; 'grid' / 'brute' force either."""
    dev = _cuda()
    if not float(c) > 0:
        raise _lib.NerfailError('view_map: c must be positive')
    q = _lib.f32c(torch.as_tensor(pts_max), dev)
    if q.dim() != 3 or q.shape[2] != 3:
        raise ValueError('pts_max must be [H,W,3] (NC:418-423), got %s' % (tuple(q.shape),))
    if method == 'auto':
        method = 'grid' if point_set.Ns >= GRID_FROM else 'brute'
    if method == 'grid':
        ws, nbytes = point_set.grid()
        wi = torch.empty((2, q.shape[0], q.shape[1], 8), dtype=torch.float32, device=dev)
        sum_d2 = torch.empty((), dtype=torch.float64, device=dev)
        ops.knn8_weights_into(q, point_set.Ns, float(c), ws, nbytes, wi, sum_d2)
        return wi, sum_d2
    if method != 'brute':
        raise ValueError('method must be auto, grid or brute')
    d, i = knn8(q, point_set.points, method='brute')
    wi = torch.ops.nerfail_mi.gauss_weight(torch.stack([d, i], 0).unsqueeze(0), float(c))[0]
    return wi, torch.square(d).sum(dtype=torch.float64)


def foreground_pixels(image):
    """The foreground of a view as gauss_net sees it: the pixels of its registered uint8 BGRA image [H,W,4] with alpha > 0, as a
    device int32 [n] tensor of indices row * W + col, strictly ascending (nerfail_fg_pixel_list: an ordered stream compaction
    on the device). One 4-byte host read: n, the length of what is returned."""
    dev = _cuda()
    img = torch.as_tensor(np.asarray(image) if not isinstance(image, torch.Tensor) else image)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 4:
        raise ValueError('image must be uint8 BGRA [H,W,4] (MyDataset.py:200), got %s %s' % (img.dtype, tuple(img.shape)))
    lst, count = ops.fg_pixel_list(img.to(dev).contiguous())
    return lst[:int(count)]                                   # THE host read


def view_map_pixels(pts, pix, hw, point_set, c=0.02, method='auto'):
    """One view over a pixel list: pts [n,3] (the rendered points of the pixels `pix`, device int32 [n]) against the point set ->
    (weight_and_index [2,H,W,8], sum_d2). Row pix[j] of both planes is bit for bit view_map's row for that point; every other
    row is zero bits (weight 0, index 0). sum_d2 (0-dim float64) sums the 8 n listed distances' float32 squares only.
    method 'auto': from GRID_FROM points up nerfail_knn8_grid_weights_list (the map zeroed and the rows scattered by one call),
    below that the brute-force scan over the compact queries, K9, and index_copy_ into zeros; 'grid' / 'brute' force either."""
    dev = _cuda()
    if not float(c) > 0:
        raise _lib.NerfailError('view_map_pixels: c must be positive')
    H, W = int(hw[0]), int(hw[1])
    q = _lib.f32c(torch.as_tensor(pts), dev).reshape(-1, 3)
    pix = torch.as_tensor(pix, dtype=torch.int32, device=dev).contiguous()
    n = int(pix.shape[0])
    if pix.dim() != 1 or q.shape[0] != n or n > H * W:
        raise ValueError('pts must be [n,3] and pix [n] with n <= H * W, got %s and %s' % (tuple(q.shape), tuple(pix.shape)))
    if method == 'auto':
        method = 'grid' if point_set.Ns >= GRID_FROM else 'brute'
    if method == 'grid':
        ws, nbytes = point_set.grid()
        wi = torch.empty((2, H, W, 8), dtype=torch.float32, device=dev)
        sum_d2 = torch.empty((), dtype=torch.float64, device=dev)
        ops.knn8_weights_list_into(q, pix, point_set.Ns, float(c), ws, nbytes, wi, sum_d2)
        return wi, sum_d2
    if method != 'brute':
        raise ValueError('method must be auto, grid or brute')
    wi = torch.zeros((2, H * W, 8), dtype=torch.float32, device=dev)
    if n == 0:
        return wi.reshape(2, H, W, 8), torch.zeros((), dtype=torch.float64, device=dev)
    d, i = knn8(q, point_set.points, method='brute')
    rows = torch.ops.nerfail_mi.gauss_weight(torch.stack([d, i], 0).reshape(1, 2, n, 1, 8), float(c))[0].reshape(2, n, 8)
    wi.index_copy_(1, pix.long(), rows)
    return wi.reshape(2, H, W, 8), torch.square(d).sum(dtype=torch.float64)


class SceneMaps:
    """What build_scene_maps returns. `point_set` / `Ns`: the scene's point set and the rows of its perturbation table;
    `view_ids`: {split: [id, ...]} in pose order - hand them to the attack loops as `view_ids=`; `v`: the "v" of DW:92-100, the
    mean over the views of each view's mean squared distance; `c`; `hw`: the views' (H, W); `rendered`: {split: [n, ...]}, the
    pixels rendered and searched per view (H W each, or the foreground counts of a foreground_only call).
    A call with `shard_batch` set is sharded: `shard_batch` and `world` record the batch size and the number of ranks the views
    were split for, `owned` ({split: [positions]}) names the views THIS rank rendered, searched and registered - under the
    attack's own rule, sharding.owned_positions per split; `view_ids`, `rendered` and `v` cover all views on every rank.
    Unsharded: shard_batch None, world 1, every position owned."""

    def __init__(self, point_set, view_ids, v, c, hw, scene_key, rendered=None, owned=None, shard_batch=None, world=1):
        self.point_set, self.Ns, self.view_ids, self.v, self.c, self.hw, self.scene_key = point_set, point_set.Ns, view_ids, v, c, hw, scene_key
        self.rendered = rendered if rendered is not None else {s: [hw[0] * hw[1]] * len(ids) for s, ids in view_ids.items()}
        self.owned = owned if owned is not None else {s: list(range(len(ids))) for s, ids in view_ids.items()}
        self.shard_batch, self.world = shard_batch, world

    def batches(self, splits, batch_size):
        """[(None, None, ids), ...]: the views of `splits` (a name or several) in order, `batch_size` per batch, as
        attack.nerfail_s takes them when the maps and images are resident. Sharded maps: each split is cut on its own (a batch
        never holds views of two splits: ownership was decided per split), and `batch_size` must be the `shard_batch` the maps
        were built for (ValueError otherwise: another cut hands a rank views it never registered)."""
        splits = (splits,) if isinstance(splits, str) else splits
        if self.shard_batch is None:
            ids = [v for s in splits for v in self.view_ids[s]]
            return [(None, None, ids[b:b + batch_size]) for b in range(0, len(ids), batch_size)]
        if int(batch_size) != self.shard_batch:
            raise ValueError('SceneMaps.batches: these maps were built for batches of shard_batch = %d views, not %r' % (self.shard_batch, batch_size))
        return [(None, None, self.view_ids[s][b:b + batch_size]) for s in splits for b in range(0, len(self.view_ids[s]), batch_size)]


def build_scene_maps(render_kwargs, poses, hwf, K, mask_list, c=0.02, chunk=1024 * 32, images=None, view_ids=None,
                     point_set=None, keep_maps=True, save_dir=None, on_view=None, foreground_only=False, shard_batch=None, group=None):
    """NC + CI + DW for a whole scene without the disk: every view of `poses` rendered, searched, weighted and registered.

    `poses`: {split: [N,4,4]} or one array (then the split is 'test'). `mask_list`: the views of the 'test' split whose points
    form the point set, in that order (CI:56-61) - unless `point_set` (a PointSet) is given. Per view: nerf_to_coord.render ->
    view_map -> GaussNet.register_view(id, Ns, map, images[split][i]); the default id is (scene_key, split, i), `view_ids`
    ({split: ids}) names them otherwise. `images`: {split: uint8 BGRA [N,H,W,4] or a list} (MyDataset.py:200), kept resident
    next to the maps. Nothing crosses PCIe but the two counts per view the inverted-index build reads.
    keep_maps=False: only the inverted index and the image of a view stay resident (the attack's forward needs the map, so
    True is the default). `save_dir`: ALSO write `index_and_weight/<split>/<i>.pth` (CPU float32 [2,H,W,8]) and its
    `<i>.idx.pth` sidecar under it - what the file pipeline leaves behind, which GaussNet.load_view_maps accepts as it is; no
    `.npy`, no `index_and_dist`. `on_view(split, i, view_id, weight_and_index)` sees every map. Returns SceneMaps.

    foreground_only=True (opt-in; for attacks that take the returned ids as `view_ids=`): a view is rendered and searched only on
    its foreground, the pixels whose images[split][i] has alpha > 0 - gauss_net's own rule: it writes 0 to x_rgba and takes no
    gradient anywhere else, and an all-zero map row adds nothing to the inverted index. Every view then needs an image
    (ValueError otherwise, before any device call). Per view: foreground_pixels -> nerf_to_coord.render_pixels -> view_map_pixels
    -> register_view. The map equals the full call's at every foreground pixel, bit for bit, and is all-zero bits (weight 0,
    index 0) elsewhere; the point set, Ns and the perturbation table are those of the full call: the mask_list views are still
    rendered in full, once, and their cached points gathered at the list. `rendered` holds the foreground counts; a view
    without foreground gets a zero map. `v` becomes the mean, over the views with n > 0, of sum_d2 / (8 n): the mean squared
    distance of FOREGROUND pixels - not DW's `v`, which also averages the background pixels' far larger distances.

    shard_batch=B (opt-in, an int >= 1) under a torch.distributed process group (`group`; None = the default group) of more than
    one rank: the scene is built once across the group, for an attack that takes `maps.batches(split, B)`. Each mask_list view
    is rendered by pixel range over the ranks and the ranges exchanged - point set, Ns and grid are the one-rank call's bits on
    every rank. Of each split, position i is rendered, searched, registered, saved and shown to on_view only on
    sharding.batch_owner(i, len(split), B, world): the rank attack._share hands it to. view_ids, rendered and v cover all
    views on every rank: each rank writes its views' terms and counts in double into one vector (zeros elsewhere), ONE all-reduce
    sums it - exactly: every slot has one non-zero contribution - and the terms are added in the one-rank call's order, so v is
    the one-rank v; that vector is the call's only host read besides the per-view counts. With one rank (or no group) the
    call owns everything and is today's call. shard_batch=None: every rank builds everything, as before."""
    if not isinstance(poses, dict):
        poses, images, view_ids = {'test': poses}, (None if images is None else {'test': images}), (None if view_ids is None else {'test': view_ids})
    if foreground_only:                                       # (host-side only: nothing has touched the device yet)
        for split in poses:
            have = images.get(split) if images is not None else None
            if have is None or len(have) < len(poses[split]) or any(have[i] is None for i in range(len(poses[split]))):
                raise ValueError("foreground_only=True: every view needs its image (images['%s'] is missing or short)" % split)
    world, rank = 1, 0
    if shard_batch is not None:
        if isinstance(shard_batch, bool) or int(shard_batch) != shard_batch or int(shard_batch) < 1:
            raise ValueError('shard_batch must be an int >= 1 (the batch size of the attack), got %r' % (shard_batch,))
        shard_batch = int(shard_batch)
        world, rank = sharding.world_and_rank(group)
    sharded = world > 1
    dev = _cuda()
    order = [s for s in SPLITS if s in poses] + [s for s in poses if s not in SPLITS]
    H, W = int(hwf[0]), int(hwf[1])
    scene_key = 'scene%d' % next(_scene_counter)
    pts_cache = {}
    if point_set is None:
        if 'test' not in poses:
            raise ValueError("the point set is made of views of the 'test' split (CI:56-61): pass poses['test'] or point_set=")
        mask_list = [int(i) for i in mask_list]
        if not mask_list or min(mask_list) < 0 or max(mask_list) >= len(poses['test']):
            raise ValueError('mask_list must name views of the test split (0..%d)' % (len(poses['test']) - 1))
        for i in sorted(set(mask_list)):                      # rendered once: as base views now, as views of their split below
            pts_cache[i] = (_render_pts_sharded(render_kwargs, poses['test'][i], hwf, K, chunk, rank, world, group) if sharded
                            else _render_pts(render_kwargs, poses['test'][i], hwf, K, chunk))
        point_set = PointSet.from_views([pts_cache[i] for i in mask_list])
    Ns = point_set.Ns
    v_sum = torch.zeros((), dtype=torch.float64, device=dev)
    n_views = 0
    out_ids, rendered, owned = {}, {}, {}
    first = dict(zip(order, itertools.accumulate([0] + [len(poses[s]) for s in order])))       # a split's first slot in `terms`
    total = sum(len(poses[s]) for s in order)
    terms = torch.zeros((2 * total,), dtype=torch.float64, device=dev) if sharded else None   # per view: its term of v, its count
    for split in order:
        ids = []
        rendered[split] = []
        owned[split] = sharding.owned_positions(len(poses[split]), shard_batch, rank, world) if sharded else list(range(len(poses[split])))
        mine = set(owned[split])
        if save_dir is not None:
            os.makedirs(os.path.join(save_dir, 'index_and_weight', split), exist_ok=True)
        for i, c2w in enumerate(poses[split]):
            pts = pts_cache.pop(i, None) if split == 'test' else None
            vid = view_ids[split][i] if view_ids is not None and split in view_ids else (scene_key, split, i)
            ids.append(vid)
            if i not in mine:                                 # another rank's view: only its id is known here
                continue
            if foreground_only:
                pix = foreground_pixels(images[split][i])
                n = int(pix.shape[0])
                if pts is not None:                           # a base view: rendered in full above, gathered here
                    fg = pts.reshape(-1, 3).index_select(0, pix.long())
                else:
                    with torch.no_grad():                     # as the reference renders (NC:640)
                        fg = _NC.render_pixels(H, W, K, pix, chunk=chunk, c2w=torch.as_tensor(c2w)[:3, :4], **render_kwargs)[3]
                wi, sum_d2 = view_map_pixels(fg, pix, (H, W), point_set, c)
                term = sum_d2 / float(8 * n) if n > 0 else None   # mean squared distance of this view's foreground
            else:
                if pts is None:
                    pts = _render_pts(render_kwargs, c2w, hwf, K, chunk)
                wi, sum_d2 = view_map(pts, point_set, c)
                n, term = H * W, sum_d2 / float(8 * H * W)    # this view's mean squared distance (DW:92), on the device
            if sharded:
                if term is not None:
                    terms[first[split] + i] = term
                terms[total + first[split] + i] = float(n)
            else:
                if term is not None:
                    v_sum += term
                    n_views += 1
                rendered[split].append(n)
            img = images[split][i] if images is not None and images.get(split) is not None else None
            if keep_maps:
                _G.register_view(vid, Ns, wi, img)
            else:
                _G.view_indices([wi], Ns, [vid])
                if img is not None:
                    _G.register_view(vid, Ns, ori_img=img)
            if save_dir is not None:
                mpath = os.path.join(save_dir, 'index_and_weight', split, '%d.pth' % i)
                torch.save(wi.cpu(), mpath)                    # DW:95-97
                vi = _G.view_indices([wi], Ns, [vid])[0]
                vi.src = _file_sig(mpath)
                vi.save(os.path.join(save_dir, 'index_and_weight', split, '%d.idx.pth' % i))
            if on_view is not None:
                on_view(split, i, vid, wi)
        out_ids[split] = ids
    if sharded:
        sharding.all_reduce_sum_(terms, group)                # exact: one rank wrote each slot, the others add zeros
        t = terms.cpu().tolist()                              # THE host read of the call
        v_sum = 0.
        for split in order:
            for k in range(first[split], first[split] + len(poses[split])):
                rendered[split].append(int(t[total + k]))
                if rendered[split][-1] > 0:                   # the one-rank call's order, view by view, in double
                    v_sum += t[k]
                    n_views += 1
        v = v_sum / max(n_views, 1)
    else:
        v = float(v_sum) / max(n_views, 1)                    # THE host read of the call
    return SceneMaps(point_set, out_ids, v, float(c), (H, W), scene_key, rendered, owned, shard_batch, world)


def perturbation_table(base_images, zero_init=True, rand_init=False, generator=None):
    """The perturbation table the attacks start from (AS:218, 252-263): uint8 (or float) BGRA base images [n,H,W,4], or a list
    of [H,W,4], -> float32 [n,H,W,4] on the device. rand_init: every channel drawn uniformly from [0, 255) where alpha > 0
    (AS:254-257; `generator`: a device torch.Generator, default the global one); zero_init: the colours zeroed, the alpha
    channel kept (AS:259-263) - applied after rand_init when both are set, as the reference applies them."""
    dev = _cuda()
    if isinstance(base_images, (list, tuple)):
        base_images = torch.stack([torch.as_tensor(np.asarray(b) if not isinstance(b, torch.Tensor) else b) for b in base_images])   # AS:218
    t = torch.as_tensor(base_images).to(dev).float().contiguous()                           # AS:252
    if t.dim() != 4 or t.shape[3] != 4:
        raise ValueError('base images must be [n,H,W,4] (BGRA), got %s' % (tuple(t.shape),))
    if rand_init:
        r = (torch.rand_like(t) if generator is None else torch.rand(t.shape, dtype=t.dtype, device=dev, generator=generator)) * 255
        t = torch.where(t[:, :, :, 3].unsqueeze(-1) > 0, r, t)
    if zero_init:
        z = torch.zeros_like(t)
        z[:, :, :, 3] = t[:, :, :, 3]
        t = z
    return t
