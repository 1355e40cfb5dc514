"""Multi-GPU decomposition of the path (one process per GPU, torch.distributed; nccl = RCCL on ROCm).

Rays are independent units: a view's pixel range is cut into contiguous per-rank ranges and rendered
with NO data-path collective (each rank writes / keeps its own slice). The attack step has one real
exchange: the sum of the per-shard perturbation gradients (attack.nerfail_s_step). Training splits the rays of each
step and sums one flat buffer of parameter gradients per step (train.train, _train.GradArena).
Which rank owns which view of a list attacked in batches is ONE rule, batch_share: attack._share cuts a batch with it,
scene.build_scene_maps(shard_batch=) builds a view on batch_owner's rank only. Results that every rank needs whole (a base view's
points, exported train views, rendered splits) travel by all_gather_ranges_: a copy from the owner, never a sum.
The range arithmetic is pure host logic: importable and testable without a GPU.
"""
import torch
import torch.distributed as dist


def shard_range(n, rank, world):
    """Contiguous near-equal split of n units: returns [lo, hi) for `rank`. The first n % world ranks get one more."""
    if world <= 0 or not (0 <= rank < world):
        raise ValueError('bad rank/world: %r/%r' % (rank, world))
    base, rem = divmod(int(n), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_ranges(n, world):
    return [shard_range(n, r, world) for r in range(world)]


def batch_bounds(position, n, batch_size):
    """[b0, b1): the batch that holds `position` when a list of n ids is cut into batches of `batch_size`, the last one short."""
    n, batch_size, position = int(n), int(batch_size), int(position)
    if batch_size < 1 or not (0 <= position < n):
        raise ValueError('bad position/n/batch_size: %r/%r/%r' % (position, n, batch_size))
    b0 = position - position % batch_size
    return b0, min(b0 + batch_size, n)


def batch_share(B, rank, world):
    """THE ownership rule of a batch of B views: rank `rank` owns shard_range(B, rank, world) of it. attack._share cuts every
    batch with this call; batch_owner / owned_positions apply it to a whole list of ids cut into batches."""
    return shard_range(B, rank, world)


def owned_positions(n, batch_size, rank, world):
    """The positions of a list of n ids that `rank` owns when the list is attacked in batches of `batch_size` (the last one
    short) over `world` ranks: per batch [b0, b1), b0 + batch_share(b1 - b0, rank, world). Ascending."""
    n, batch_size = int(n), int(batch_size)
    if batch_size < 1 or n < 0:
        raise ValueError('bad n/batch_size: %r/%r' % (n, batch_size))
    out = []
    for b0 in range(0, n, batch_size):
        lo, hi = batch_share(min(batch_size, n - b0), rank, world)
        out.extend(range(b0 + lo, b0 + hi))
    return out


def batch_owner(position, n, batch_size, world):
    """The rank that owns `position` of a list of n ids under owned_positions' rule."""
    b0, b1 = batch_bounds(position, n, batch_size)
    for r in range(int(world)):
        lo, hi = batch_share(b1 - b0, r, world)
        if lo <= position - b0 < hi:
            return r
    raise ValueError('bad world: %r' % (world,))


def world_and_rank(group=None):
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


_STAGE = {}                 # (numel, dtype) -> pinned host buffer, insertion order = LRU order
STAGE_SLOTS = 4             # gradient sizes in use at once: one per perturbation table shape


def force_collectives():
    """NERFAIL_FORCE_COLLECTIVE=1: issue the all-reduce even in a 1-rank group (a dry run of the RCCL path on a one-GPU box:
    communicator creation, stream semantics and event timing are exercised; the sum over one rank is the identity)."""
    import os
    return os.environ.get('NERFAIL_FORCE_COLLECTIVE', '0') == '1'


def _stage(t):
    """The pinned host buffer of t's size and dtype (kept per size, least recently used size dropped)."""
    key = (t.numel(), t.dtype)
    h = _STAGE.pop(key, None)
    if h is None:
        h = torch.empty(t.numel(), dtype=t.dtype, pin_memory=True)
        while len(_STAGE) >= STAGE_SLOTS:                 # bounded: the least recently used size goes
            _STAGE.pop(next(iter(_STAGE)))
    _STAGE[key] = h                                       # most recently used last
    return h


def _staged(t, group):
    """A HIP tensor under a pure 'gloo' group: the collective runs on a pinned host copy."""
    return t.is_cuda and str(dist.get_backend(group)) == 'gloo'


def _collective(group=None):
    """Is a collective issued at all: a process group is up and has more than one rank (or force_collectives())."""
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or force_collectives())


def all_reduce_(t, op, group=None):
    """In-place all-reduce with `op` over ranks. RCCL all-reduce for HIP tensors whenever the group has a device-capable backend
    ('nccl', a 'cpu:gloo,cuda:nccl' pair, or the default-initialised group that maps to it): the GPU-box path, xGMI. Only under
    a pure 'gloo' group (the CPU tests and the one-GPU rehearsal, where RCCL refuses two ranks on one device) a HIP tensor is
    staged through a pinned host buffer (kept per size), reduced there and copied back."""
    if not _collective(group):
        return t
    if _staged(t, group):
        h = _stage(t)
        h.copy_(t.reshape(-1), non_blocking=False)
        dist.all_reduce(h, op=op, group=group)
        t.copy_(h.reshape(t.shape))
        return t
    dist.all_reduce(t, op=op, group=group)
    return t


def all_reduce_sum_(t, group=None, timing=None):
    """In-place sum over ranks (all_reduce_ with SUM). `timing`: optional dict; when a collective is issued on a HIP tensor it
    gets the HIP events around it and the bytes moved, appended to timing['allreduce_events'] as (start, end, bytes)."""
    if not _collective(group):
        return t
    timed = timing is not None and t.is_cuda
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    all_reduce_(t, dist.ReduceOp.SUM, group)
    if timed:
        e1.record()
        timing.setdefault('allreduce_events', []).append((e0, e1, t.numel() * t.element_size()))
    return t


def broadcast_(t, src=0, group=None):
    """In-place broadcast of group rank `src`'s tensor to every rank, on the same two paths as all_reduce_: RCCL on the
    device, or - HIP tensor under pure gloo - through the pinned host buffer. `t` must be contiguous."""
    if not _collective(group):
        return t
    gsrc = dist.get_global_rank(group, src) if group is not None else src
    if _staged(t, group):
        h = _stage(t)
        if dist.get_rank(group) == src:
            h.copy_(t.reshape(-1), non_blocking=False)
        dist.broadcast(h, src=gsrc, group=group)
        if dist.get_rank(group) != src:
            t.copy_(h.reshape(t.shape))
        return t
    dist.broadcast(t, src=gsrc, group=group)
    return t


def all_gather_ranges_(t, ranges, group=None):
    """In place: `t` (contiguous) is cut along its first dimension into one range per rank, ranges[r] = [lo, hi) - rank r has
    filled t[lo:hi]; afterwards every rank holds every range, each bit for bit its owner's. One broadcast_ per non-empty range
    (so on broadcast_'s two paths: on the device, or - HIP tensor under pure gloo - through the pinned host buffer)."""
    if not _collective(group):
        return t
    if not t.is_contiguous() or len(ranges) != dist.get_world_size(group):
        raise ValueError('all_gather_ranges_: a contiguous tensor and one range per rank')
    for src, (lo, hi) in enumerate(ranges):
        if hi > lo:
            broadcast_(t[lo:hi], src, group)
    return t


def render_view_sharded(render_fn, H, W, rank, world):
    """Render this rank's pixel range of an H x W view. `render_fn(pix_begin, pix_count)` returns a dict of
    per-ray tensors; no collective is issued (the driver gathers or writes rank-local slices)."""
    lo, hi = shard_range(H * W, rank, world)
    return (lo, hi), render_fn(lo, hi - lo)


def render_shard(H, W, K, c2w, near, far, rank=None, world=None, chunk=1024 * 32, group=None, **render_kwargs):
    """This rank's contiguous pixel range of one view through the NC render pipeline (ray_gen of the range ->
    batchify_rays incl. pts_max). Returns ((lo, hi), dict of per-ray tensors [hi-lo, ...]). Rays are independent, so
    the per-rank slices concatenate BITWISE to the unsharded render (tests/test_hip_multigpu.py); no collective."""
    from . import run_nerf as RN
    if world is None:
        world, rank = world_and_rank(group)
    kw = {k: v for k, v in render_kwargs.items() if k not in ('ndc', 'use_viewdirs')}

    def render_fn(lo, n):
        if n == 0:
            return {}
        rays = RN.ray_gen(H, W, K, c2w, near, far, lo, n)
        return RN.batchify_rays(rays, chunk, want_pts_max=True, **kw)
    return render_view_sharded(render_fn, H, W, rank, world)
