"""`torch.ops.nerfail_mi.*`: the hot-path kernels registered with the PyTorch dispatcher (SURVEY.md section 8b "What the
C-ABI layer must export"; BASELINE north_star "exposed to Python through PyTorch-ROCm custom ops").

Each op is a `torch.library.custom_op` over ONE entry point of libnerfail_hip.so (include/nerfail_hip.h), with
  * a device implementation for 'cuda' (= HIP on ROCm): dense float32 HIP tensors in, freshly allocated outputs out, the
    launch on torch's current stream - and nothing for the CPU key: there is no CPU path;
  * a fake (meta) implementation, so the ops trace under FakeTensor / torch.compile / AOT autograd;
  * `register_autograd` where the reference differentiates through the function (raw2outputs RN:262-305 -> MLP parameters,
    gauss_net's gather GN:53-119 -> the perturbation).
`torch.library.opcheck` runs on every op in tests/test_hip_ops.py. The module-level functions of the mirrors (raw2outputs,
create_gauss_w, igsm_step, knn8, get_rays ...) call these ops. SURVEY's `render_rays_fused_fwd/bwd` is their composition:
`_train.RenderRaysTrain` (a torch.autograd.Function over ray sampling, mlp_fwd_train, composite, sample_fine and, backwards,
composite_bwd and mlp_bwd), selected by render_rays whenever a NeRF parameter requires grad."""
import math
from typing import Optional, Sequence

import torch
from torch import Tensor
from torch.library import custom_op

from . import _lib

NS = 'nerfail_mi'


def _chk(rc):
    _lib.check(rc)


def _s():
    return _lib.stream()


# ----------------------------------------------------------------------------------------------- K1 rays (RH:157-166, RN:102-123)
@custom_op(NS + '::ray_gen', mutates_args=(), device_types='cuda')
def ray_gen(K: Tensor, c2w: Tensor, anchor: Tensor, H: int, W: int, near: float, far: float, pix_begin: int, pix_count: int) -> Tensor:
    """Packed rays [pix_count, 11] (o, d, near, far, viewdir) of pixels [pix_begin, pix_begin + pix_count) of an H x W view.
    K [3,3] and c2w [3,4] may live on the host (12 + 4 floats are passed by value); `anchor` is any tensor on the target device."""
    k = K.detach().to('cpu', torch.float64)
    c = c2w.detach().to('cpu', torch.float32)[:3, :4].reshape(-1).tolist()
    rays = torch.empty((pix_count, _lib.RAY_FLOATS), dtype=torch.float32, device=anchor.device)
    _chk(_lib.load().nerfail_ray_gen(H, W, _lib.host_floats([k[0, 0], k[1, 1], k[0, 2], k[1, 2]]), _lib.host_floats(c), near, far,
                                     pix_begin, pix_count, _lib.dev(rays), _s()))
    return rays


@ray_gen.register_fake
def _(K, c2w, anchor, H, W, near, far, pix_begin, pix_count):
    return anchor.new_empty((pix_count, _lib.RAY_FLOATS), dtype=torch.float32)


@custom_op(NS + '::ray_gen_list', mutates_args=(), device_types='cuda')
def ray_gen_list(K: Tensor, c2w: Tensor, pix: Tensor, H: int, W: int, near: float, far: float) -> Tensor:
    """Packed rays [n, 11] of the pixels `pix` (device int32 [n], values row * W + col) of an H x W view: row j is bit for bit
    ray_gen's row for pixel pix[j] (nerfail_ray_gen_list, fg revision 1). K and c2w as in ray_gen. Not differentiable: data."""
    k = K.detach().to('cpu', torch.float64)
    c = c2w.detach().to('cpu', torch.float32)[:3, :4].reshape(-1).tolist()
    if pix.dtype != torch.int32 or pix.dim() != 1:
        raise TypeError('ray_gen_list: pix must be int32 [n] (got %s %s)' % (pix.dtype, tuple(pix.shape)))
    n = pix.shape[0]
    rays = torch.empty((n, _lib.RAY_FLOATS), dtype=torch.float32, device=pix.device)
    _chk(_lib.load().nerfail_ray_gen_list(H, W, _lib.host_floats([k[0, 0], k[1, 1], k[0, 2], k[1, 2]]), _lib.host_floats(c), near, far,
                                          _lib.dev(pix, 'pix'), n, _lib.dev(rays), _s()))
    return rays


@ray_gen_list.register_fake
def _(K, c2w, pix, H, W, near, far):
    return pix.new_empty((pix.shape[0], _lib.RAY_FLOATS), dtype=torch.float32)


FG_OPS = ('ray_gen_list',)


# ----------------------------------------------------------------------------------------------- K1b training batch (RN:690-773)
def _u64(key):
    """The dispatcher's int is a signed 64-bit value: keys are taken modulo 2^64 (pass the two's complement of one >= 2^63)."""
    return int(key) & 0xFFFFFFFFFFFFFFFF


def as_op_key(key):
    """A 64-bit key as the signed int the ops accept."""
    key = _u64(key)
    return key - (1 << 64) if key >= (1 << 63) else key


@custom_op(NS + '::index_shuffle', mutates_args=(), device_types='cuda')
def index_shuffle(anchor: Tensor, key: int, m: int, first: int, n: int) -> Tensor:
    """int64 [n]: P(key, m)(first + j), the range [first, first + n) of the keyed permutation of [0, m) (nerfail_index_shuffle).
    `anchor` is any tensor on the target device. Not differentiable: indices are data."""
    out = torch.empty((n,), dtype=torch.int64, device=anchor.device)
    _chk(_lib.load().nerfail_index_shuffle(_u64(key), m, first, n, _lib.dev(out), _s()))
    return out


@index_shuffle.register_fake
def _(anchor, key, m, first, n):
    return anchor.new_empty((n,), dtype=torch.int64)


@custom_op(NS + '::train_batch', mutates_args=(), device_types='cuda')
def train_batch(poses: Tensor, images: Optional[Tensor], view_ids: Optional[Tensor], sel: Optional[Tensor], H: int, W: int,
                K4: Sequence[float], near: float, far: float, window: Sequence[int], view0: int, n_views: int, key: int, first: int,
                n: int, want_sel: bool) -> tuple[Tensor, Tensor, Tensor]:
    """(rays [n,11], target [n,3], sel_out [n] int64) of one training batch from resident poses [n_img,12] and images
    [n_img,H,W,3] (nerfail_train_batch). K4 = (fx, fy, cx, cy), window = (row0, col0, wh, ww). The batch is `sel` (int64
    population indices) or, with sel None, positions [first, first + n) of the permutation `key` of the population
    n_views * wh * ww. images None: target is empty; want_sel False: sel_out is empty. Not differentiable: rays and targets
    are data."""
    dev = poses.device
    if poses.dtype != torch.float32 or poses.dim() != 2 or poses.shape[1] != 12:
        raise ValueError('train_batch: poses must be float32 [n_img, 12] (got %s %s)' % (poses.dtype, tuple(poses.shape)))
    n_img = poses.shape[0]
    if images is not None and (images.dtype != torch.float32 or tuple(images.shape) != (n_img, H, W, 3)):
        raise ValueError('train_batch: images must be float32 [%d, %d, %d, 3] (got %s %s)' % (n_img, H, W, images.dtype, tuple(images.shape)))
    if view_ids is not None and (view_ids.dtype != torch.int32 or tuple(view_ids.shape) != (n_views,)):
        raise ValueError('train_batch: view_ids must be int32 [n_views]')
    if sel is not None and (sel.dtype != torch.int64 or tuple(sel.shape) != (n,)):
        raise ValueError('train_batch: sel must be int64 [n]')
    if len(K4) != 4 or len(window) != 4:
        raise ValueError('train_batch: K4 = (fx, fy, cx, cy) and window = (row0, col0, wh, ww)')
    rays = torch.empty((n, _lib.RAY_FLOATS), dtype=torch.float32, device=dev)
    target = torch.empty((n if images is not None else 0, 3), dtype=torch.float32, device=dev)
    sel_out = torch.empty((n if want_sel else 0,), dtype=torch.int64, device=dev)
    _chk(_lib.load().nerfail_train_batch(H, W, _lib.host_floats(K4), near, far, _lib.dev(poses, 'poses'), n_img, _lib.dev(images, 'images'),
                                         window[0], window[1], window[2], window[3], _lib.dev(view_ids, 'view_ids'), view0, n_views,
                                         _lib.dev(sel, 'sel'), _u64(key), first, n, _lib.dev(rays),
                                         _lib.dev(target) if images is not None else None, _lib.dev(sel_out) if want_sel else None, _s()))
    return rays, target, sel_out


@train_batch.register_fake
def _(poses, images, view_ids, sel, H, W, K4, near, far, window, view0, n_views, key, first, n, want_sel):
    return (poses.new_empty((n, _lib.RAY_FLOATS)), poses.new_empty((n if images is not None else 0, 3)),
            poses.new_empty((n if want_sel else 0,), dtype=torch.int64))


BATCH_OPS = ('index_shuffle', 'train_batch')


# ----------------------------------------------------------------------------------------------- K5 + K7 composite (RN:262-305)
@custom_op(NS + '::composite', mutates_args=(), device_types='cuda')
def composite(raw: Tensor, z_vals: Tensor, rays: Tensor, white_bkgd: bool) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """raw2outputs: (rgb_map [R,3], disp_map [R], acc_map [R], weights [R,N], depth_map [R])."""
    R, N = z_vals.shape
    dev = raw.device
    o = [torch.empty(s, dtype=torch.float32, device=dev) for s in ((R, 3), (R,), (R,), (R, N), (R,))]
    _chk(_lib.load().nerfail_composite(_lib.dev(raw), _lib.dev(z_vals), _lib.dev(rays), None, R, N, int(white_bkgd), _lib.dev(o[0]),
                                       _lib.dev(o[1]), _lib.dev(o[2]), _lib.dev(o[3]), _lib.dev(o[4]), None, None, _s()))
    return o[0], o[1], o[2], o[3], o[4]


@composite.register_fake
def _(raw, z_vals, rays, white_bkgd):
    R, N = z_vals.shape
    return (raw.new_empty((R, 3)), raw.new_empty((R,)), raw.new_empty((R,)), raw.new_empty((R, N)), raw.new_empty((R,)))


@custom_op(NS + '::composite_bwd', mutates_args=(), device_types='cuda')
def composite_bwd(raw: Tensor, z_vals: Tensor, rays: Tensor, white_bkgd: bool, g_rgb: Tensor, g_disp: Tensor, g_acc: Tensor,
                  g_weights: Tensor, g_depth: Tensor) -> Tensor:
    """d(loss)/d(raw) for upstream gradients of all five outputs (autograd of RN:262-305)."""
    R, N = z_vals.shape
    d_raw = torch.empty((R, N, 4), dtype=torch.float32, device=raw.device)
    _chk(_lib.load().nerfail_composite_bwd(_lib.dev(raw), _lib.dev(z_vals), _lib.dev(rays), None, R, N, int(white_bkgd),
                                           _lib.dev(g_rgb), _lib.dev(g_disp), _lib.dev(g_acc), _lib.dev(g_depth), _lib.dev(g_weights),
                                           _lib.dev(d_raw), _s()))
    return d_raw


@composite_bwd.register_fake
def _(raw, z_vals, rays, white_bkgd, g_rgb, g_disp, g_acc, g_weights, g_depth):
    return raw.new_empty(raw.shape)


def _composite_setup(ctx, inputs, output):
    raw, z_vals, rays, white = inputs
    ctx.save_for_backward(raw, z_vals, rays)
    ctx.white = white


def _composite_backward(ctx, g_rgb, g_disp, g_acc, g_w, g_depth):
    raw, z_vals, rays = ctx.saved_tensors
    R, N = z_vals.shape

    def z(g, shape):
        return torch.zeros(shape, dtype=torch.float32, device=raw.device) if g is None else g.contiguous().float()
    d_raw = composite_bwd(raw, z_vals, rays, ctx.white, z(g_rgb, (R, 3)), z(g_disp, (R,)), z(g_acc, (R,)), z(g_w, (R, N)), z(g_depth, (R,)))
    return d_raw, None, None, None


composite.register_autograd(_composite_backward, setup_context=_composite_setup)


# ----------------------------------------------------------------------------------------------- K6 sample_pdf (RH:200-243)
@custom_op(NS + '::sample_pdf', mutates_args=(), device_types='cuda')
def sample_pdf(bins: Tensor, weights: Tensor, u: Tensor) -> Tensor:
    """Inverse-CDF samples [R, n]; u is [n] (shared, det=True) or [R, n] (explicit draws)."""
    R, nb = bins.shape
    n = u.shape[-1]
    out = torch.empty((R, n), dtype=torch.float32, device=bins.device)
    _chk(_lib.load().nerfail_sample_pdf(_lib.dev(bins), _lib.dev(weights), R, nb, _lib.dev(u), int(u.dim() == 1), n, _lib.dev(out), _s()))
    return out


@sample_pdf.register_fake
def _(bins, weights, u):
    return bins.new_empty((bins.shape[0], u.shape[-1]))


# ----------------------------------------------------------------------------------------------- K3 + K4 fused encode + MLP (RN:37-51)
@custom_op(NS + '::mlp_fwd', mutates_args=(), device_types='cuda')
def mlp_fwd(packed: Tensor, pts: Tensor, viewdirs: Tensor, D: int, W: int, skip: int) -> Tensor:
    """raw [R,N,4] of the NeRF MLP on points [R,N,3] with per-ray view directions [R,3] (weights: NeRF.packed())."""
    R, N = pts.shape[0], pts.shape[1]
    raw = torch.empty((R, N, 4), dtype=torch.float32, device=pts.device)
    _chk(_lib.load().nerfail_mlp_fwd(_lib.dev(packed), D, W, skip, _lib.dev(pts), _lib.dev(viewdirs), R * N, N, _lib.dev(raw), _s()))
    return raw


@mlp_fwd.register_fake
def _(packed, pts, viewdirs, D, W, skip):
    return pts.new_empty((pts.shape[0], pts.shape[1], 4))


# ----------------------------------------------------------------------------------------------- K8 exact 8-NN (CI:126-145)
@custom_op(NS + '::knn8', mutates_args=(), device_types='cuda')
def knn8(queries: Tensor, points: Tensor) -> tuple[Tensor, Tensor]:
    """(dist [Q,8] ascending, idx [Q,8] as float32 - the on-disk convention, CI:148-163) of queries [Q,3] in points [M,3]."""
    lib = _lib.load()
    Q, M = queries.shape[0], points.shape[0]
    dist = torch.empty((Q, 8), dtype=torch.float32, device=queries.device)
    idx = torch.empty((Q, 8), dtype=torch.float32, device=queries.device)
    if M >= 4096:
        nb = lib.nerfail_knn8_grid_workspace_bytes(M)
        ws = torch.empty((nb,), dtype=torch.uint8, device=queries.device)
        _chk(lib.nerfail_knn8_grid(_lib.dev(queries), Q, _lib.dev(points), M, _lib.dev(dist), _lib.dev(idx), None, _lib.dev(ws), nb, _s()))
    else:
        _chk(lib.nerfail_knn8(_lib.dev(queries), Q, _lib.dev(points), M, _lib.dev(dist), _lib.dev(idx), None, _s()))
    return dist, idx


@knn8.register_fake
def _(queries, points):
    return queries.new_empty((queries.shape[0], 8)), queries.new_empty((queries.shape[0], 8))


# ----------------------------------------------------------------------------------------------- K9 create_gauss_w (GN:169-186)
@custom_op(NS + '::gauss_weight', mutates_args=(), device_types='cuda')
def gauss_weight(dist_and_index: Tensor, c: float) -> Tensor:
    B, P = dist_and_index.shape[0], dist_and_index.shape[2] * dist_and_index.shape[3]
    out = torch.empty_like(dist_and_index)
    _chk(_lib.load().nerfail_gauss_weight(_lib.dev(dist_and_index), B, P, c, _lib.dev(out), _s()))
    return out


@gauss_weight.register_fake
def _(dist_and_index, c):
    return torch.empty_like(dist_and_index)


# ----------------------------------------------------------------------------------------------- K8 + K9 in one launch (scene revision 1)
def knn8_weights_into(queries, n_points, c, grid_ws, grid_bytes, out, sum_d2):
    """nerfail_knn8_grid_weights[_view] over a BUILT grid (scene.PointSet keeps one per scene): `out` [2,...,8] and the device
    double `sum_d2` are overwritten. queries [H,W,3] with both sides >= 8 take the 8 x 8 pixel-tile form, anything else the flat one."""
    lib = _lib.load()
    Q = queries.numel() // 3
    nb = lib.nerfail_knn8_grid_weights_workspace_bytes(Q)
    ws = torch.empty((max(nb, 8) // 8,), dtype=torch.float64, device=queries.device)
    d2 = _lib.c_p(sum_d2.data_ptr()) if sum_d2 is not None else None
    if queries.dim() == 3 and queries.shape[0] >= 8 and queries.shape[1] >= 8:
        _chk(lib.nerfail_knn8_grid_weights_view(_lib.dev(queries, 'queries'), queries.shape[0], queries.shape[1], n_points, c, _lib.dev(out), d2,
                                                _lib.dev(grid_ws), grid_bytes, _lib.c_p(ws.data_ptr()), nb, _s()))
    else:
        _chk(lib.nerfail_knn8_grid_weights(_lib.dev(queries, 'queries'), Q, n_points, c, _lib.dev(out), d2, _lib.dev(grid_ws), grid_bytes,
                                           _lib.c_p(ws.data_ptr()), nb, _s()))


def fg_pixel_list(image):
    """nerfail_fg_pixel_list: uint8 BGRA [H,W,4] on the device -> (list int32 [H*W], count int32 [1]), both on the device;
    list[:count] are the pixels with alpha > 0, ascending. No host read."""
    lib = _lib.load()
    P = image.numel() // 4
    if image.dtype != torch.uint8 or image.shape[-1] != 4 or P == 0:
        raise TypeError('fg_pixel_list: image must be uint8 BGRA [H,W,4] (got %s %s)' % (image.dtype, tuple(image.shape)))
    nb = lib.nerfail_fg_pixel_list_workspace_bytes(P)
    ws = torch.empty((max(nb, 4) // 4,), dtype=torch.int32, device=image.device)
    lst = torch.empty((P,), dtype=torch.int32, device=image.device)
    count = torch.empty((1,), dtype=torch.int32, device=image.device)
    _chk(lib.nerfail_fg_pixel_list(_lib.dev(image, 'image'), P, _lib.dev(lst), _lib.dev(count), _lib.dev(ws), nb, _s()))
    return lst, count


def knn8_weights_list_into(queries, pix, n_points, c, grid_ws, grid_bytes, out, sum_d2):
    """nerfail_knn8_grid_weights_list over a BUILT grid: `out` [2,...,8] (P = out.numel() // 16 rows per plane) is zeroed, row
    pix[j] of both planes receives query j's weights and indices, the device double `sum_d2` the fold over the listed distances."""
    lib = _lib.load()
    n = pix.shape[0]
    if queries.numel() != 3 * n or pix.dtype != torch.int32:
        raise TypeError('knn8_weights_list_into: queries [n,3] and pix int32 [n] must agree')
    nb = lib.nerfail_knn8_grid_weights_workspace_bytes(n)
    ws = torch.empty((max(nb, 8) // 8,), dtype=torch.float64, device=out.device)
    d2 = _lib.c_p(sum_d2.data_ptr()) if sum_d2 is not None else None
    _chk(lib.nerfail_knn8_grid_weights_list(_lib.dev(queries, 'queries') if n else None, n, _lib.dev(pix, 'pix') if n else None,
                                            out.numel() // 16, n_points, c, _lib.dev(out), d2, _lib.dev(grid_ws), grid_bytes,
                                            _lib.c_p(ws.data_ptr()), nb, _s()))


@custom_op(NS + '::knn8_weights', mutates_args=(), device_types='cuda')
def knn8_weights(queries: Tensor, points: Tensor, c: float) -> tuple[Tensor, Tensor]:
    """(weight_and_index [2,...,8], sum_d2 float64 [1]) of queries [...,3] in points [M,3]: the attack's map of a view - bit for
    bit knn8 followed by gauss_weight(c) - and the sum of the squared distances (float32 squares, added in double). From 4096
    points up ONE search kernel with the weights as its epilogue (the grid is built per call here; scene.view_map keeps it),
    below that the brute-force scan followed by gauss_weight."""
    lib = _lib.load()
    M = points.shape[0]
    lead = tuple(queries.shape[:-1])
    Q = queries.numel() // 3
    out = torch.empty((2,) + lead + (8,), dtype=torch.float32, device=queries.device)
    sum_d2 = torch.zeros((1,), dtype=torch.float64, device=queries.device)
    if not c > 0:
        raise _lib.NerfailError('knn8_weights: c must be positive')
    if Q == 0:
        return out, sum_d2
    if M >= 4096:
        nb = lib.nerfail_knn8_grid_workspace_bytes(M)
        ws = torch.empty((nb,), dtype=torch.uint8, device=queries.device)
        _chk(lib.nerfail_knn8_grid_build(_lib.dev(points, 'points'), M, _lib.dev(ws), nb, _s()))
        knn8_weights_into(queries, M, c, ws, nb, out, sum_d2)
    else:
        dai = torch.empty((1, 2, Q, 1, 8), dtype=torch.float32, device=queries.device)
        _chk(lib.nerfail_knn8(_lib.dev(queries, 'queries'), Q, _lib.dev(points, 'points'), M, _lib.dev(dai[0, 0]), _lib.dev(dai[0, 1]), None, _s()))
        _chk(lib.nerfail_gauss_weight(_lib.dev(dai), 1, Q, c, _lib.dev(out), _s()))
        sum_d2 = torch.square(dai[0, 0]).sum(dtype=torch.float64).reshape(1)
    return out, sum_d2


@knn8_weights.register_fake
def _(queries, points, c):
    return queries.new_empty((2,) + tuple(queries.shape[:-1]) + (8,)), queries.new_empty((1,), dtype=torch.float64)


SCENE_OPS = ('knn8_weights',)


# ----------------------------------------------------------------------------------------------- K10 / K11 gather (GN:53-119)
@custom_op(NS + '::gauss_gather', mutates_args=(), device_types='cuda')
def gauss_gather(spatial: Tensor, weight_and_index: Tensor, ori_img: Tensor, epsilon: float) -> tuple[Tensor, Tensor]:
    """(x, x_rgba) [B,H,W,4]; epsilon < 0 = no clip (epsilon=None in the reference)."""
    wi = weight_and_index
    B, P = wi.shape[0], wi.shape[2] * wi.shape[3]
    s = spatial.reshape(-1, 4)
    x = torch.empty(ori_img.shape, dtype=torch.float32, device=s.device)
    xr = torch.empty(ori_img.shape, dtype=torch.float32, device=s.device)
    _chk(_lib.load().nerfail_gauss_fwd(_lib.dev(s), s.shape[0], _lib.dev(wi), _lib.dev(ori_img), B, P, epsilon, _lib.dev(x),
                                       _lib.dev(xr), None, _s()))
    return x, xr


@gauss_gather.register_fake
def _(spatial, weight_and_index, ori_img, epsilon):
    return torch.empty_like(ori_img), torch.empty_like(ori_img)


@custom_op(NS + '::gauss_gather_bwd', mutates_args=(), device_types='cuda')
def gauss_gather_bwd(weight_and_index: Tensor, ori_img: Tensor, x: Tensor, grad_x: Tensor, grad_x_rgba: Tensor, n_rows: int,
                     epsilon: float) -> Tensor:
    """d/d(spatial) [n_rows,4]: the stateless (float-atomic) form of K11. The attack loop's deterministic form with cached
    per-view indices is nerfail_amd.GaussNet.gauss_gather / nerfail_gauss_bwd_views."""
    wi = weight_and_index
    B, P = wi.shape[0], wi.shape[2] * wi.shape[3]
    gs = torch.zeros((n_rows, 4), dtype=torch.float32, device=x.device)
    _chk(_lib.load().nerfail_gauss_bwd(_lib.dev(wi), _lib.dev(ori_img), _lib.dev(x), _lib.dev(grad_x), _lib.dev(grad_x_rgba), n_rows,
                                       B, P, epsilon, _lib.dev(gs), _s()))
    return gs


@gauss_gather_bwd.register_fake
def _(weight_and_index, ori_img, x, grad_x, grad_x_rgba, n_rows, epsilon):
    return x.new_empty((n_rows, 4))


def _gather_setup(ctx, inputs, output):
    spatial, wi, ori, eps = inputs
    ctx.save_for_backward(wi, ori, output[0])
    ctx.eps, ctx.s_shape = eps, spatial.shape


def _gather_backward(ctx, g_x, g_xr):
    wi, ori, x = ctx.saved_tensors

    def z(g):
        return torch.zeros_like(x) if g is None else g.contiguous().float()
    n = 1
    for d in ctx.s_shape[:-1]:
        n *= d
    return gauss_gather_bwd(wi, ori, x, z(g_x), z(g_xr), n, ctx.eps).reshape(ctx.s_shape), None, None, None


gauss_gather.register_autograd(_gather_backward, setup_context=_gather_setup)


# ----------------------------------------------------------------------------------------------- K12 sign step (AS:352-392)
@custom_op(NS + '::igsm_step', mutates_args=(), device_types='cuda')
def igsm_step(spatial: Tensor, grad: Tensor, spatial_init: Tensor, a: float, epsilon: float, targeted: bool) -> Tensor:
    out = torch.empty_like(spatial)
    _chk(_lib.load().nerfail_igsm_step(_lib.dev(spatial), _lib.dev(grad), _lib.dev(spatial_init), spatial.numel() // 4, a, epsilon,
                                       int(targeted), _lib.dev(out), _s()))
    return out


@igsm_step.register_fake
def _(spatial, grad, spatial_init, a, epsilon, targeted):
    return torch.empty_like(spatial)


# ----------------------------------------------------------------------------------------------- K6 fused fine sampling (RN:392-412)
@custom_op(NS + '::sample_fine', mutates_args=(), device_types='cuda')
def sample_fine(rays: Tensor, z_coarse: Tensor, weights: Tensor, u: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """sample_pdf on the mid-points (RH:200-243) + sort(cat(z_vals, z_samples)) (RN:397: SURVEY's `merge_sorted`) +
    pts = o + d z (RN:399) + z_std (RN:412) in one launch: (z_samples [R,nf], z_fine [R,nc+nf], pts [R,nc+nf,3], z_std [R]).
    u is [nf] (shared, perturb = 0) or [R,nf] (explicit draws)."""
    R, nc = z_coarse.shape
    nf = u.shape[-1]
    dev = z_coarse.device
    zs = torch.empty((R, nf), dtype=torch.float32, device=dev)
    zf = torch.empty((R, nc + nf), dtype=torch.float32, device=dev)
    pts = torch.empty((R, nc + nf, 3), dtype=torch.float32, device=dev)
    zstd = torch.empty((R,), dtype=torch.float32, device=dev)
    _chk(_lib.load().nerfail_sample_fine(_lib.dev(rays), R, _lib.dev(z_coarse), _lib.dev(weights), nc, _lib.dev(u), int(u.dim() == 1), nf,
                                         _lib.dev(zs), _lib.dev(zf), _lib.dev(pts), _lib.dev(zstd), _s()))
    return zs, zf, pts, zstd


@sample_fine.register_fake
def _(rays, z_coarse, weights, u):
    R, nc = z_coarse.shape
    nf = u.shape[-1]
    return z_coarse.new_empty((R, nf)), z_coarse.new_empty((R, nc + nf)), z_coarse.new_empty((R, nc + nf, 3)), z_coarse.new_empty((R,))


# ----------------------------------------------------------------------------------------------- K4b training kernels (RN:776-801)
@custom_op(NS + '::mlp_fwd_train', mutates_args=(), device_types='cuda')
def mlp_fwd_train(packed: Tensor, pts: Tensor, viewdirs: Tensor, D: int, W: int, skip: int) -> tuple[Tensor, Tensor]:
    """mlp_fwd that also saves what the backward needs: (raw [R,N,4], acts [nerfail_mlp_train_acts_floats])."""
    lib = _lib.load()
    R, N = pts.shape[0], pts.shape[1]
    raw = torch.empty((R, N, 4), dtype=torch.float32, device=pts.device)
    acts = torch.empty((lib.nerfail_mlp_train_acts_floats(D, W, R * N),), dtype=torch.float32, device=pts.device)
    _chk(lib.nerfail_mlp_fwd_train(_lib.dev(packed), D, W, skip, _lib.dev(pts), _lib.dev(viewdirs), R * N, N, _lib.dev(raw), _lib.dev(acts), _s()))
    return raw, acts


@mlp_fwd_train.register_fake
def _(packed, pts, viewdirs, D, W, skip):
    M = pts.shape[0] * pts.shape[1]
    return pts.new_empty((pts.shape[0], pts.shape[1], 4)), pts.new_empty((_lib.load().nerfail_mlp_train_acts_floats(D, W, M),))


def mlp_param_shapes(D, W, skip, input_ch=63, input_ch_views=27):
    """Shapes of NeRF's parameters in _train.ordered_params order (RH:72-98): pts_linears (w, b) x D, views, feature, alpha, rgb."""
    shapes = []
    for i in range(D):
        fan_in = input_ch if i == 0 else (W + input_ch if (skip >= 0 and i == skip + 1) else W)
        shapes += [(W, fan_in), (W,)]
    return shapes + [(W // 2, W + input_ch_views), (W // 2,), (W, W), (W,), (1, W), (1,), (3, W // 2), (3,)]


@custom_op(NS + '::mlp_bwd', mutates_args=(), device_types='cuda')
def mlp_bwd(packed: Tensor, packed_T: Tensor, acts: Tensor, d_raw: Tensor, D: int, W: int, skip: int) -> list[Tensor]:
    """d loss / d (NeRF parameters) from d loss / d raw [R,N,4] and the activations mlp_fwd_train saved: backward-data pass
    (layer gradients) + weight-gradient pass. Returns the 2 D + 8 gradients in _train.ordered_params order.
    packed_T = _train.packed_T(net) (nerfail_mlp_pack_T)."""
    lib = _lib.load()
    M = d_raw.shape[0] * d_raw.shape[1]
    dev = d_raw.device
    dz = torch.empty((lib.nerfail_mlp_train_dz_floats(D, W, M),), dtype=torch.float32, device=dev)
    _chk(lib.nerfail_mlp_bwd_data(_lib.dev(packed), _lib.dev(packed_T), D, W, skip, _lib.dev(d_raw), _lib.dev(acts), M, _lib.dev(dz), _s()))
    grads = [torch.empty(sh, dtype=torch.float32, device=dev) for sh in mlp_param_shapes(D, W, skip)]     # overwritten
    mp = _lib.mlp_params(D, W, 63, 27, skip, grads, None)
    nbytes = lib.nerfail_mlp_bwd_weights_scratch_bytes(D, W, skip, M, 0, 0)
    scratch = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)      # per-workgroup partials (deterministic sum)
    _chk(lib.nerfail_mlp_bwd_weights(D, W, skip, _lib.dev(acts), _lib.dev(dz), M, mp, 0, None, 0, _lib.dev(scratch), nbytes, _s()))
    return grads


@mlp_bwd.register_fake
def _(packed, packed_T, acts, d_raw, D, W, skip):
    return [d_raw.new_empty(sh) for sh in mlp_param_shapes(D, W, skip)]


ALL = ('ray_gen', 'composite', 'composite_bwd', 'sample_pdf', 'sample_fine', 'mlp_fwd', 'mlp_fwd_train', 'mlp_bwd', 'knn8', 'gauss_weight',
       'gauss_gather', 'gauss_gather_bwd', 'igsm_step')


# ----------------------------------------------------------------------------------------------- MyCNN victim (model/MyModel.py:5-52)
def _cnn_sizes(x, num_classes, keep_masks):
    lib = _lib.load()
    B, C3, H, W = x.shape
    ws = lib.nerfail_cnn_workspace_bytes(B, H, W, num_classes)
    if C3 != 3 or ws == 0:
        raise ValueError('cnn_fwd: unsupported input %s (needs [B,3,H,W] with a 4 x 4 seventh stage, H and W in 766..893)'
                         % (tuple(x.shape),))
    return ws // 4, (lib.nerfail_cnn_mask_bytes(B, H, W) if keep_masks else 0)


def _x3_image_ok(packed_x3, num_classes, what):
    if packed_x3.dtype != torch.uint8 or packed_x3.numel() != _lib.load().nerfail_cnn_x3_packed_bytes(num_classes):
        raise ValueError('%s: packed_x3 is not the bf16x3 image of cnn_pack_x3 (uint8, %d bytes)'
                         % (what, _lib.load().nerfail_cnn_x3_packed_bytes(num_classes)))


# One body per op pair. packed_x3 = None: the exact family (cnn_fwd, cnn_bwd_data[_multi]); else the bf16x3 family (csrc/cnn_x3.hip:
# stages 2..7 as six bf16 products per f32 product, f32-accurate), whose entry points take the bf16x3 image after `packed`.
# Buffers and sizes are the same: a workspace and masks of one family can be handed to the other family's backward. `op` names
# the op that was called in the error texts.
def _cnn_call(entry, packed, packed_x3, *args):
    lib = _lib.load()
    if packed_x3 is None:
        _chk(getattr(lib, 'nerfail_cnn_' + entry)(_lib.dev(packed), *args))
    else:
        _chk(getattr(lib, 'nerfail_cnn_%s_x3' % entry)(_lib.dev(packed), _lib.dev(packed_x3), *args))


def _cnn_masks_kept(op, masks, packed_x3, num_classes):
    if masks.numel() == 0:
        raise RuntimeError('%s: the forward kept no masks (%skeep_masks=False)' % (op, '' if packed_x3 is not None else 'cnn_fwd with '))
    if packed_x3 is not None:
        _x3_image_ok(packed_x3, num_classes, op)


def _cnn_fwd(op, packed, packed_x3, x, num_classes, keep_masks):
    B, _, H, W = x.shape
    n_ws, n_mask = _cnn_sizes(x, num_classes, keep_masks)
    if packed_x3 is not None:
        _x3_image_ok(packed_x3, num_classes, op)
    ws = torch.empty((n_ws,), dtype=torch.float32, device=x.device)
    masks = torch.empty((n_mask,), dtype=torch.uint8, device=x.device)
    logits = torch.empty((B, num_classes), dtype=torch.float32, device=x.device)
    _cnn_call('fwd', packed, packed_x3, num_classes, _lib.dev(x, 'x'), B, H, W, _lib.dev(ws), _lib.dev(masks) if keep_masks else None,
              _lib.dev(logits), _s())
    return logits, ws, masks


def _cnn_fwd_fake(x, num_classes, keep_masks):
    n_ws, n_mask = _cnn_sizes(x, num_classes, keep_masks)
    return (x.new_empty((x.shape[0], num_classes)), x.new_empty((n_ws,)), x.new_empty((n_mask,), dtype=torch.uint8))


def _cnn_bwd_data(op, packed, packed_x3, workspace, masks, d_logits, H, W):
    lib = _lib.load()
    B, C = d_logits.shape
    _cnn_masks_kept(op, masks, packed_x3, C)
    nb = lib.nerfail_cnn_bwd_scratch_bytes(B, H, W)
    scratch = torch.empty((nb // 4,), dtype=torch.float32, device=d_logits.device)
    dx = torch.empty((B, 3, H, W), dtype=torch.float32, device=d_logits.device)
    _cnn_call('bwd_data', packed, packed_x3, C, _lib.dev(workspace), _lib.dev(masks), _lib.dev(d_logits), B, H, W, _lib.dev(scratch),
              _lib.dev(dx), _s())
    return dx


def _cnn_bwd_data_multi(op, packed, packed_x3, workspace, masks, d_logits, H, W):
    lib = _lib.load()
    if d_logits.dtype != torch.float32:
        raise TypeError('%s: d_logits must be float32 (got %s)' % (op, d_logits.dtype))
    if d_logits.dim() != 3:
        raise ValueError('%s: d_logits must be [R,B,num_classes] (got %s)' % (op, tuple(d_logits.shape),))
    R, B, C = d_logits.shape
    _cnn_masks_kept(op, masks, packed_x3, C)
    nb = lib.nerfail_cnn_bwd_multi_scratch_bytes(R, B, H, W)
    if nb == 0 or workspace.numel() * 4 != lib.nerfail_cnn_workspace_bytes(B, H, W, C) or masks.numel() != lib.nerfail_cnn_mask_bytes(B, H, W):
        raise ValueError('%s: unsupported d_logits %s for a %d x %d forward (needs R >= 1, R * B <= 65535 and '
                         'the workspace and masks of a forward of B images)' % (op, tuple(d_logits.shape), H, W))
    scratch = torch.empty((nb // 4,), dtype=torch.float32, device=d_logits.device)
    dx = torch.empty((R, B, 3, H, W), dtype=torch.float32, device=d_logits.device)
    _cnn_call('bwd_data_multi', packed, packed_x3, C, _lib.dev(workspace), _lib.dev(masks), _lib.dev(d_logits, 'd_logits'), R, B, H, W,
              _lib.dev(scratch), _lib.dev(dx), _s())
    return dx


@custom_op(NS + '::cnn_fwd', mutates_args=(), device_types='cuda')
def cnn_fwd(packed: Tensor, x: Tensor, num_classes: int, keep_masks: bool) -> tuple[Tensor, Tensor, Tensor]:
    """MyCNN forward: (logits [B,num_classes], workspace (saved activations), masks (pool argmax codes; empty unless
    keep_masks)). packed = nerfail_amd.MyModel.MyCNN.packed(). Differentiable with respect to x when keep_masks is set."""
    return _cnn_fwd('cnn_fwd', packed, None, x, num_classes, keep_masks)


@custom_op(NS + '::cnn_fwd_x3', mutates_args=(), device_types='cuda')
def cnn_fwd_x3(packed: Tensor, packed_x3: Tensor, x: Tensor, num_classes: int, keep_masks: bool) -> tuple[Tensor, Tensor, Tensor]:
    """cnn_fwd with stages 2..7 on the bf16x3 image: (logits, workspace, masks) with cnn_fwd's shapes and contracts."""
    return _cnn_fwd('cnn_fwd_x3', packed, packed_x3, x, num_classes, keep_masks)


cnn_fwd.register_fake(lambda packed, x, num_classes, keep_masks: _cnn_fwd_fake(x, num_classes, keep_masks))
cnn_fwd_x3.register_fake(lambda packed, packed_x3, x, num_classes, keep_masks: _cnn_fwd_fake(x, num_classes, keep_masks))


@custom_op(NS + '::cnn_bwd_data', mutates_args=(), device_types='cuda')
def cnn_bwd_data(packed: Tensor, workspace: Tensor, masks: Tensor, d_logits: Tensor, H: int, W: int) -> Tensor:
    """d loss / d x [B,3,H,W] of cnn_fwd from d loss / d logits and the forward's workspace and masks (weights frozen)."""
    return _cnn_bwd_data('cnn_bwd_data', packed, None, workspace, masks, d_logits, H, W)


@custom_op(NS + '::cnn_bwd_data_x3', mutates_args=(), device_types='cuda')
def cnn_bwd_data_x3(packed: Tensor, packed_x3: Tensor, workspace: Tensor, masks: Tensor, d_logits: Tensor, H: int, W: int) -> Tensor:
    """cnn_bwd_data with stages 7..2 on the bf16x3 image."""
    return _cnn_bwd_data('cnn_bwd_data_x3', packed, packed_x3, workspace, masks, d_logits, H, W)


cnn_bwd_data.register_fake(lambda packed, workspace, masks, d_logits, H, W: d_logits.new_empty((d_logits.shape[0], 3, H, W)))
cnn_bwd_data_x3.register_fake(lambda packed, packed_x3, workspace, masks, d_logits, H, W: d_logits.new_empty((d_logits.shape[0], 3, H, W)))


@custom_op(NS + '::cnn_bwd_data_multi', mutates_args=(), device_types='cuda')
def cnn_bwd_data_multi(packed: Tensor, workspace: Tensor, masks: Tensor, d_logits: Tensor, H: int, W: int) -> Tensor:
    """cnn_bwd_data for R right-hand sides of ONE cnn_fwd in one launch chain: d_logits [R,B,num_classes] ->
    [R,B,3,H,W], slice r bitwise cnn_bwd_data(..., d_logits[r], ...). workspace and masks are that forward's (B images)."""
    return _cnn_bwd_data_multi('cnn_bwd_data_multi', packed, None, workspace, masks, d_logits, H, W)


@custom_op(NS + '::cnn_bwd_data_multi_x3', mutates_args=(), device_types='cuda')
def cnn_bwd_data_multi_x3(packed: Tensor, packed_x3: Tensor, workspace: Tensor, masks: Tensor, d_logits: Tensor, H: int, W: int) -> Tensor:
    """cnn_bwd_data_multi with stages 7..2 on the bf16x3 image: d_logits [R,B,num_classes] -> [R,B,3,H,W], slice r bitwise
    cnn_bwd_data_x3(..., d_logits[r], ...)."""
    return _cnn_bwd_data_multi('cnn_bwd_data_multi_x3', packed, packed_x3, workspace, masks, d_logits, H, W)


def _cnn_multi_fake(d_logits, H, W):
    return d_logits.new_empty((d_logits.shape[0], d_logits.shape[1], 3, H, W))


cnn_bwd_data_multi.register_fake(lambda packed, workspace, masks, d_logits, H, W: _cnn_multi_fake(d_logits, H, W))
cnn_bwd_data_multi_x3.register_fake(lambda packed, packed_x3, workspace, masks, d_logits, H, W: _cnn_multi_fake(d_logits, H, W))


# autograd of cnn_fwd and cnn_fwd_x3: the inputs are (packed[, packed_x3], x, num_classes, keep_masks); the weight images come
# first among the saved tensors. ctx.cnn_fwd_x3 (whether a bf16x3 image was saved) also is how cnn_fwd_saved() knows the node.
def _cnn_setup(ctx, inputs, output):
    *images, x, num_classes, keep_masks = inputs
    _, ws, masks = output
    ctx.save_for_backward(*images, ws, masks)
    ctx.hw = (x.shape[2], x.shape[3])
    ctx.cnn_fwd_x3 = len(images) == 2
    ctx.mark_non_differentiable(ws, masks)


def _cnn_backward(ctx, g_logits, g_ws, g_masks):
    *images, ws, masks = ctx.saved_tensors
    dx = None
    if g_logits is not None:
        dx = (cnn_bwd_data_x3 if ctx.cnn_fwd_x3 else cnn_bwd_data)(*images, ws, masks, g_logits.contiguous().float(), *ctx.hw)
    return (None,) * len(images) + (dx, None, None)


cnn_fwd.register_autograd(_cnn_backward, setup_context=_cnn_setup)
cnn_fwd_x3.register_autograd(_cnn_backward, setup_context=_cnn_setup)


def cnn_fwd_saved(logits):
    """(packed, workspace, masks, (H, W), packed_x3) that the cnn_fwd / cnn_fwd_x3 call which returned `logits` saved for its
    backward: read off the tensor's autograd node, so nothing is copied and nothing outlives the graph. packed_x3 is None for
    the exact family (cnn_fwd) and the bf16x3 image for cnn_fwd_x3: it says which backward family matches. None when `logits`
    is not the direct output of a differentiable cnn_fwd[_x3], or when its graph was already freed (a backward without
    retain_graph)."""
    node = getattr(logits, 'grad_fn', None)
    x3 = getattr(node, 'cnn_fwd_x3', None)
    if x3 is None:
        return None
    try:
        packed, *image_x3, ws, masks = node.saved_tensors
    except RuntimeError:
        return None
    return packed, ws, masks, node.hw, (image_x3[0] if x3 else None)


def cnn_grad_layout(num_classes):
    """[(offset, shape)] of the 18 parameter gradients in the flat d_params buffer of nerfail_cnn_bwd_weights: nn.Module
    layout in state-dict order, every region starting on a multiple of 4 floats (include/nerfail_hip.h, ABI 11)."""
    chans = (3, 32, 64, 128, 256, 256, 128, 64)
    shapes = []
    for i in range(7):
        shapes += [(chans[i + 1], chans[i], 3, 3), (chans[i + 1],)]
    shapes += [(512, 1024), (512,), (num_classes, 512), (num_classes,)]
    out, o = [], 0
    for sh in shapes:
        out.append((o, sh))
        o += (math.prod(sh) + 3) // 4 * 4
    return out, o


@custom_op(NS + '::cnn_bwd_weights', mutates_args=(), device_types='cuda')
def cnn_bwd_weights(packed: Tensor, x: Tensor, workspace: Tensor, masks: Tensor, d_logits: Tensor, need_dx: bool) -> tuple[Tensor, Tensor]:
    """(d_params, d_x) of cnn_fwd from d loss / d logits [B,num_classes], the forward's input, workspace and masks: d_params
    is the flat gradient of all 18 parameters (cnn_grad_layout), d_x [B,3,H,W] is bitwise cnn_bwd_data's (empty unless
    need_dx). No float atomics: two calls give the same bits."""
    lib = _lib.load()
    if d_logits.dtype != torch.float32 or x.dtype != torch.float32:
        raise TypeError('cnn_bwd_weights: x and d_logits must be float32 (got %s, %s)' % (x.dtype, d_logits.dtype))
    if d_logits.dim() != 2 or x.dim() != 4 or x.shape[0] != d_logits.shape[0] or x.shape[1] != 3:
        raise ValueError('cnn_bwd_weights: x must be [B,3,H,W] and d_logits [B,num_classes] (got %s, %s)'
                         % (tuple(x.shape), tuple(d_logits.shape)))
    B, C = d_logits.shape
    H, W = x.shape[2], x.shape[3]
    if masks.numel() == 0:
        raise RuntimeError('cnn_bwd_weights: the forward kept no masks (cnn_fwd with keep_masks=False)')
    nb = lib.nerfail_cnn_bwd_weights_scratch_bytes(B, H, W, C)
    if nb == 0 or workspace.numel() * 4 != lib.nerfail_cnn_workspace_bytes(B, H, W, C) or masks.numel() != lib.nerfail_cnn_mask_bytes(B, H, W):
        raise ValueError('cnn_bwd_weights: unsupported d_logits %s for a forward of x %s (needs the workspace and masks of a '
                         'forward of these B images)' % (tuple(d_logits.shape), tuple(x.shape)))
    dev = d_logits.device
    scratch = torch.empty((nb // 4,), dtype=torch.float32, device=dev)
    d_params = torch.zeros((lib.nerfail_cnn_grad_floats(C),), dtype=torch.float32, device=dev)   # zeros: the alignment padding
    dx = torch.empty((B, 3, H, W) if need_dx else (0,), dtype=torch.float32, device=dev)
    _chk(lib.nerfail_cnn_bwd_weights(_lib.dev(packed), C, _lib.dev(x, 'x'), _lib.dev(workspace), _lib.dev(masks),
                                     _lib.dev(d_logits, 'd_logits'), B, H, W, _lib.dev(scratch), _lib.dev(d_params),
                                     _lib.dev(dx) if need_dx else None, _s()))
    return d_params, dx


@cnn_bwd_weights.register_fake
def _(packed, x, workspace, masks, d_logits, need_dx):
    _, total = cnn_grad_layout(d_logits.shape[1])
    return d_logits.new_empty((total,)), d_logits.new_empty(tuple(x.shape) if need_dx else (0,))


class CnnTrainFn(torch.autograd.Function):
    """logits = MyCNN(x) with gradients for the parameters: cnn_fwd keeping its masks, cnn_bwd_weights backwards. `module`
    supplies the weight image; the parameters are passed so that autograd routes their gradients."""

    @staticmethod
    def forward(ctx, module, x, *params):
        packed = module.packed()
        logits, ws, masks = cnn_fwd(packed, x, module.num_classes, True)
        ctx.save_for_backward(packed, x, ws, masks)
        ctx.num_classes = module.num_classes
        ctx.mark_non_differentiable()
        return logits

    @staticmethod
    def backward(ctx, g_logits):
        packed, x, ws, masks = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[1]
        d_params, dx = cnn_bwd_weights(packed, x, ws, masks, g_logits.contiguous().float(), need_dx)
        layout, _ = cnn_grad_layout(ctx.num_classes)
        grads = []
        for i, (o, sh) in enumerate(layout):
            grads.append(d_params[o:o + math.prod(sh)].view(sh) if ctx.needs_input_grad[2 + i] else None)
        return (None, dx if need_dx else None) + tuple(grads)


CNN_OPS = ('cnn_fwd', 'cnn_bwd_data', 'cnn_bwd_data_multi', 'cnn_bwd_weights')


# ---- the bf16x3 weight image of the cnn_*_x3 ops above
@custom_op(NS + '::cnn_pack_x3', mutates_args=(), device_types='cuda')
def cnn_pack_x3(packed: Tensor, num_classes: int) -> Tensor:
    """The bf16x3 weight image (uint8 bytes; layout in include/nerfail_hip.h) split on the device from MyCNN.packed()."""
    lib = _lib.load()
    if packed.dtype != torch.float32 or packed.numel() != lib.nerfail_cnn_packed_floats(num_classes):
        raise ValueError('cnn_pack_x3: packed is not the weight image of a %d-class MyCNN' % num_classes)
    out = torch.empty((lib.nerfail_cnn_x3_packed_bytes(num_classes),), dtype=torch.uint8, device=packed.device)
    _chk(lib.nerfail_cnn_pack_x3(_lib.dev(packed, 'packed'), num_classes, _lib.dev(out), _s()))
    return out


@cnn_pack_x3.register_fake
def _(packed, num_classes):
    return packed.new_empty((_lib.load().nerfail_cnn_x3_packed_bytes(num_classes),), dtype=torch.uint8)


CNN_X3_OPS = ('cnn_pack_x3', 'cnn_fwd_x3', 'cnn_bwd_data_x3', 'cnn_bwd_data_multi_x3')


# ----------------------------------------------------------------------------------------------- NeRFail-S epoch statistics (AS:319-344, 405-431; ABI 15)
def _ori_pointers(ori, n_views, P):
    """Host array of the per-view image pointers of a dense [n_views, ..., 4] image tensor (float32 or uint8)."""
    if ori.dtype not in (torch.float32, torch.uint8) or not ori.is_contiguous() or ori.numel() != n_views * P * 4:
        raise ValueError('ori must be a contiguous float32 or uint8 tensor with the shape of x_rgba')
    step = P * 4 * ori.element_size()
    return (_lib.c_p * n_views)(*[ori.data_ptr() + b * step for b in range(n_views)])


def _row_ok(row, name='row'):
    if row.dtype != torch.float32 or row.numel() != _lib.ATTACK_ROW_FLOATS or not row.is_contiguous():
        raise ValueError('%s must be %d contiguous float32' % (name, _lib.ATTACK_ROW_FLOATS))


@custom_op(NS + '::attack_logit_stats', mutates_args=('row',), device_types='cuda')
def attack_logit_stats(cla: Tensor, ori_cla: Tensor, label: int, row: Tensor) -> None:
    """Adds sum CE(ori_cla), sum CE(cla), correct(ori_cla), correct(cla), B of one batch's [B,C] logits into the stats row."""
    _row_ok(row)
    if cla.dim() != 2 or cla.shape != ori_cla.shape:
        raise ValueError('cla and ori_cla must both be [B,C]')
    _chk(_lib.load().nerfail_attack_logit_stats(_lib.dev(_lib.f32c(cla)), _lib.dev(_lib.f32c(ori_cla)), cla.shape[0], cla.shape[1], label,
                                                _lib.dev(row), _s()))


@custom_op(NS + '::img_sqerr', mutates_args=('row',), device_types='cuda')
def img_sqerr(x_rgba: Tensor, ori: Tensor, row: Tensor) -> None:
    """Adds sum (x_rgba - ori)^2 over [B,...,4] and the element count into the stats row; ori float32 or uint8."""
    _row_ok(row)
    B, P = x_rgba.shape[0], x_rgba.numel() // (4 * max(x_rgba.shape[0], 1))
    lib = _lib.load()
    scratch = torch.empty((lib.nerfail_img_sqerr_scratch_bytes() // 8,), dtype=torch.float64, device=x_rgba.device)
    _chk(lib.nerfail_img_sqerr(_lib.dev(x_rgba), _ori_pointers(ori, B, P), B, P, int(ori.dtype == torch.uint8), _lib.c_p(scratch.data_ptr()),
                               _lib.dev(row), _s()))


@custom_op(NS + '::img_sqerr_grad_add', mutates_args=('g',), device_types='cuda')
def img_sqerr_grad_add(x_rgba: Tensor, ori: Tensor, scale: float, g: Tensor) -> None:
    """g += scale (x_rgba - ori): the beta term of AS:336 in d loss / d x_rgba."""
    B, P = x_rgba.shape[0], x_rgba.numel() // (4 * max(x_rgba.shape[0], 1))
    if g.shape != x_rgba.shape:
        raise ValueError('g must have the shape of x_rgba')
    _chk(_lib.load().nerfail_img_sqerr_grad_add(_lib.dev(x_rgba), _ori_pointers(ori, B, P), B, P, int(ori.dtype == torch.uint8), scale,
                                                _lib.dev(g), _s()))


@custom_op(NS + '::attack_epoch_close', mutates_args=('best', 'record', 'flag'), device_types='cuda')
def attack_epoch_close(row: Tensor, best: Tensor, epoch: int, targeted: bool, record: Tensor, flag: Tensor) -> None:
    """AS:405-431: the row's sums -> the epoch record; the best-so-far rule against `best` (float32 [4]); flag (int32 [1])."""
    _row_ok(row)
    _row_ok(record, 'record')
    if best.dtype != torch.float32 or best.numel() != 4 or flag.dtype != torch.int32 or flag.numel() != 1:
        raise ValueError('best must be float32 [4] and flag int32 [1]')
    _chk(_lib.load().nerfail_attack_epoch_close(_lib.dev(row), _lib.dev(best), epoch, int(targeted), _lib.dev(record), _lib.dev(flag), _s()))


@custom_op(NS + '::copy_if', mutates_args=('dst',), device_types='cuda')
def copy_if(flag: Tensor, src: Tensor, dst: Tensor) -> None:
    """dst <- src when the int32 flag word on the device is set."""
    if src.dtype != torch.float32 or dst.dtype != torch.float32 or src.numel() != dst.numel() or flag.dtype != torch.int32:
        raise ValueError('src and dst must be float32 of one size, flag int32')
    _chk(_lib.load().nerfail_copy_if(_lib.dev(flag), _lib.dev(src), _lib.dev(dst), src.numel(), _s()))


@custom_op(NS + '::export_u8', mutates_args=(), device_types='cuda')
def export_u8(src: Tensor) -> Tensor:
    """uint8 of a float image as cv2.imwrite stores it: clamp to [0, 255], round half to even, NaN -> 0."""
    out = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
    _chk(_lib.load().nerfail_export_u8(_lib.dev(src), src.numel(), _lib.dev(out), _s()))
    return out


@export_u8.register_fake
def _(src):
    return src.new_empty(src.shape, dtype=torch.uint8)


ATTACK_STATS_OPS = ('attack_logit_stats', 'img_sqerr', 'img_sqerr_grad_add', 'attack_epoch_close', 'copy_if', 'export_u8')


# ----------------------------------------------------------------------------------------------- attack evaluation (model_test.py:226-348; eval revision 1)
_EVAL_LAYOUT = {_lib.EVAL_U8C4: (torch.uint8, 4), _lib.EVAL_U8C3: (torch.uint8, 3), _lib.EVAL_F32C4: (torch.float32, 4),
                _lib.EVAL_FLAT: (torch.float32, 1)}


def _eval_pixels(views, fmt, name):
    """P of a list of views in one NERFAIL_EVAL_* format (every view: same device, dtype and size, contiguous)."""
    if fmt not in _EVAL_LAYOUT:
        raise ValueError('%s: unknown image format %r' % (name, fmt))
    dtype, ch = _EVAL_LAYOUT[fmt]
    n = views[0].numel()
    for v in views:
        if v.dtype != dtype or not v.is_contiguous() or v.numel() != n or n % ch:
            raise ValueError('%s: every view must be a contiguous %s tensor of one size, a multiple of %d elements' % (name, dtype, ch))
    return n // ch


@custom_op(NS + '::eval_view_metrics', mutates_args=(), device_types='cuda')
def eval_view_metrics(attacked: Sequence[Tensor], a_format: int, originals: Sequence[Tensor], o_format: int,
                      want_cla_in: bool) -> tuple[Tensor, Tensor]:
    """(rows float64 [B,6] = {max, min, sum, sum of squares, non-zero count, n} of |attacked - original| per view,
    cla_in float32 [B,3,P] = the attacked views on white, planar - or an empty tensor when not wanted). One view per tensor."""
    B = len(attacked)
    if B < 1 or len(originals) != B:
        raise ValueError('eval_view_metrics: as many originals as attacked views, at least one')
    P = _eval_pixels(attacked, a_format, 'attacked')
    if _eval_pixels(originals, o_format, 'originals') != P:
        raise ValueError('eval_view_metrics: attacked and original views differ in size')
    lib, dev = _lib.load(), attacked[0].device
    rows = torch.empty((B, _lib.EVAL_VIEW_DOUBLES), dtype=torch.float64, device=dev)
    cla_in = torch.empty((B, 3, P) if want_cla_in else (0,), dtype=torch.float32, device=dev)
    scratch = torch.empty((lib.nerfail_eval_scratch_bytes() // 8,), dtype=torch.float64, device=dev)
    for v in list(attacked) + list(originals):
        _lib.dev(v, 'view')
    _chk(lib.nerfail_eval_view_metrics((_lib.c_p * B)(*[v.data_ptr() for v in attacked]), a_format,
                                       (_lib.c_p * B)(*[v.data_ptr() for v in originals]), o_format, B, P, _lib.c_p(scratch.data_ptr()),
                                       _lib.c_p(rows.data_ptr()), _lib.c_p(cla_in.data_ptr()) if want_cla_in else None, _s()))
    return rows, cla_in


@eval_view_metrics.register_fake
def _(attacked, a_format, originals, o_format, want_cla_in):
    B, P = len(attacked), attacked[0].numel() // _EVAL_LAYOUT[a_format][1]
    return (attacked[0].new_empty((B, _lib.EVAL_VIEW_DOUBLES), dtype=torch.float64),
            attacked[0].new_empty((B, 3, P) if want_cla_in else (0,), dtype=torch.float32))


@custom_op(NS + '::eval_logit_stats', mutates_args=(), device_types='cuda')
def eval_logit_stats(logits: Tensor, label: int) -> tuple[Tensor, Tensor]:
    """(pred int32 [B]: the first maximum, -1 for a row holding a NaN; ce float64 [B]) of [B,C] logits."""
    if logits.dim() != 2:
        raise ValueError('logits must be [B,C]')
    lg = _lib.f32c(logits)
    pred = torch.empty((lg.shape[0],), dtype=torch.int32, device=lg.device)
    ce = torch.empty((lg.shape[0],), dtype=torch.float64, device=lg.device)
    _chk(_lib.load().nerfail_eval_logit_stats(_lib.dev(lg), lg.shape[0], lg.shape[1], label, _lib.dev(pred), _lib.c_p(ce.data_ptr()), _s()))
    return pred, ce


@eval_logit_stats.register_fake
def _(logits, label):
    return logits.new_empty((logits.shape[0],), dtype=torch.int32), logits.new_empty((logits.shape[0],), dtype=torch.float64)


@custom_op(NS + '::eval_fold', mutates_args=('record',), device_types='cuda')
def eval_fold(rows: Tensor, pred: Tensor, ce: Tensor, num_classes: int, record: Tensor) -> None:
    """Folds one batch's rows [B,6], predictions [B] and CEs [B] into the float64 set record (zeroed before the first batch)."""
    B = pred.numel()
    if record.dtype != torch.float64 or record.numel() != _lib.EVAL_RECORD_DOUBLES or not record.is_contiguous():
        raise ValueError('record must be %d contiguous float64' % _lib.EVAL_RECORD_DOUBLES)
    if (rows.dtype != torch.float64 or tuple(rows.shape) != (B, _lib.EVAL_VIEW_DOUBLES) or not rows.is_contiguous() or pred.dtype != torch.int32
            or ce.dtype != torch.float64 or ce.numel() != B or not pred.is_contiguous() or not ce.is_contiguous()):
        raise ValueError('rows must be float64 [B,6], pred int32 [B], ce float64 [B], all contiguous')
    for t in (rows, pred, ce, record):
        if not t.is_cuda:
            raise RuntimeError('eval_fold: a tensor is on %s: nerfail_amd runs on the MI355X only (no CPU path)' % t.device)
    _chk(_lib.load().nerfail_eval_fold(_lib.c_p(rows.data_ptr()), _lib.dev(pred), _lib.c_p(ce.data_ptr()), B, num_classes,
                                       _lib.c_p(record.data_ptr()), _s()))


EVAL_OPS = ('eval_view_metrics', 'eval_logit_stats', 'eval_fold')


# ----------------------------------------------------------------------------------------------- victim training (model_train.py:107-193; cls revision 1)
def _cls_format(images):
    if images.dtype != torch.uint8 or images.dim() < 3 or images.shape[-1] not in (3, 4) or not images.is_contiguous():
        raise ValueError('images must be a contiguous uint8 store [N,...,4] (BGRA) or [N,...,3] (got %s %s)'
                         % (images.dtype, tuple(images.shape)))
    return _lib.EVAL_U8C4 if images.shape[-1] == 4 else _lib.EVAL_U8C3


@custom_op(NS + '::cls_batch', mutates_args=(), device_types='cuda')
def cls_batch(images: Tensor, labels_all: Tensor, idx: Tensor) -> tuple[Tensor, Tensor]:
    """(x float32 [B,3,...], labels int32 [B]): the views idx (int64 [B], on the device) of a resident uint8 store [N,...,4|3] as
    the classifier's planar input - four-channel views on the white background of MD:98-105 - and their labels. An index
    outside 0..N-1 gives a view of NaN and the label -1."""
    fmt = _cls_format(images)
    N = images.shape[0]
    if labels_all.dtype != torch.int32 or labels_all.numel() != N or idx.dtype != torch.int64 or idx.dim() != 1:
        raise ValueError('labels_all must be int32 [N] and idx int64 [B]')
    B = idx.shape[0]
    P = images[0].numel() // images.shape[-1] if N else 0
    x = torch.empty((B, 3) + tuple(images.shape[1:-1]), dtype=torch.float32, device=images.device)
    labels = torch.empty((B,), dtype=torch.int32, device=images.device)
    _chk(_lib.load().nerfail_cls_batch(_lib.dev(images, 'images'), fmt, _lib.dev(labels_all, 'labels_all'), N, P, _lib.dev(idx, 'idx'), B,
                                       _lib.dev(x), _lib.dev(labels), _s()))
    return x, labels


@cls_batch.register_fake
def _(images, labels_all, idx):
    return (images.new_empty((idx.shape[0], 3) + tuple(images.shape[1:-1]), dtype=torch.float32),
            images.new_empty((idx.shape[0],), dtype=torch.int32))


@custom_op(NS + '::cls_ce', mutates_args=('row',), device_types='cuda')
def cls_ce(logits: Tensor, labels: Tensor, row: Tensor, want_grad: bool) -> Tensor:
    """Adds one batch's sum of per-view CE, correct count and B into the phase's stats row; returns d loss / d logits of
    nn.CrossEntropyLoss()'s mean, (softmax - onehot) / B [B,C] - or an empty tensor unless want_grad."""
    _row_ok(row)
    if logits.dim() != 2 or logits.dtype != torch.float32 or labels.dtype != torch.int32 or labels.numel() != logits.shape[0]:
        raise ValueError('logits must be float32 [B,C] and labels int32 [B]')
    B, C = logits.shape
    d = torch.empty((B, C) if want_grad else (0,), dtype=torch.float32, device=logits.device)
    _chk(_lib.load().nerfail_cls_ce(_lib.dev(logits, 'logits'), _lib.dev(labels, 'labels'), B, C, _lib.dev(d) if want_grad else None,
                                    _lib.dev(row), _s()))
    return d


@cls_ce.register_fake
def _(logits, labels, row, want_grad):
    return logits.new_empty(tuple(logits.shape) if want_grad else (0,))


@custom_op(NS + '::cnn_sgd_step', mutates_args=('params', 'momentum_buf', 'packed'), device_types='cuda')
def cnn_sgd_step(params: Tensor, grads: Tensor, momentum_buf: Tensor, packed: Tensor, num_classes: int, lr: float, momentum: float,
                 first: bool) -> None:
    """One torch.optim.SGD(lr, momentum) step on MyCNN's flat parameters (cnn_grad_layout) and, in the same launch, the
    weight image: afterwards `packed` is bitwise nerfail_cnn_pack of the updated parameters."""
    lib = _lib.load()
    n = lib.nerfail_cnn_grad_floats(num_classes)
    for t, name in ((params, 'params'), (grads, 'grads'), (momentum_buf, 'momentum_buf')):
        if t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
            raise ValueError('%s must be %d contiguous float32 (cnn_grad_layout)' % (name, n))
    if packed.dtype != torch.float32 or packed.numel() != lib.nerfail_cnn_packed_floats(num_classes) or not packed.is_contiguous():
        raise ValueError('packed must be the weight image of %d classes' % num_classes)
    _chk(lib.nerfail_cnn_sgd_step(_lib.dev(params, 'params'), _lib.dev(grads, 'grads'), _lib.dev(momentum_buf, 'momentum_buf'),
                                  _lib.dev(packed, 'packed'), num_classes, lr, momentum, int(first), _s()))


@custom_op(NS + '::cls_epoch_close', mutates_args=('best', 'record', 'flag'), device_types='cuda')
def cls_epoch_close(train_row: Tensor, val_row: Tensor, n_train: int, n_val: int, best: Tensor, epoch: int, record: Tensor,
                    flag: Tensor) -> None:
    """MTR:170-186: the two phases' rows and the DATASET lengths -> the epoch record; the strict best-so-far rule against
    `best` (float32 [2] = {best val acc, its epoch}); flag (int32 [1])."""
    _row_ok(train_row, 'train_row')
    _row_ok(val_row, 'val_row')
    _row_ok(record, 'record')
    if best.dtype != torch.float32 or best.numel() != 2 or flag.dtype != torch.int32 or flag.numel() != 1:
        raise ValueError('best must be float32 [2] and flag int32 [1]')
    _chk(_lib.load().nerfail_cls_epoch_close(_lib.dev(train_row), _lib.dev(val_row), n_train, n_val, _lib.dev(best), epoch,
                                             _lib.dev(record), _lib.dev(flag), _s()))


@custom_op(NS + '::cnn_bwd_weights_into', mutates_args=('scratch', 'd_params'), device_types='cuda')
def cnn_bwd_weights_into(packed: Tensor, x: Tensor, workspace: Tensor, masks: Tensor, d_logits: Tensor, scratch: Tensor,
                         d_params: Tensor) -> None:
    """cnn_bwd_weights into buffers the caller keeps across steps: d_params (cnn_grad_layout floats; the alignment floats are
    never written, so a buffer zeroed once stays clean) and scratch (at least nerfail_cnn_bwd_weights_scratch_bytes). Bitwise
    cnn_bwd_weights' d_params."""
    lib = _lib.load()
    if d_logits.dtype != torch.float32 or x.dtype != torch.float32 or d_logits.dim() != 2 or x.dim() != 4 or x.shape[0] != d_logits.shape[0]:
        raise ValueError('cnn_bwd_weights_into: x must be float32 [B,3,H,W] and d_logits float32 [B,num_classes]')
    B, C = d_logits.shape
    H, W = x.shape[2], x.shape[3]
    nb = lib.nerfail_cnn_bwd_weights_scratch_bytes(B, H, W, C)
    if (nb == 0 or masks.numel() == 0 or masks.numel() != lib.nerfail_cnn_mask_bytes(B, H, W)
            or workspace.numel() * 4 != lib.nerfail_cnn_workspace_bytes(B, H, W, C)):
        raise ValueError('cnn_bwd_weights_into: needs the workspace and masks of a mask-keeping forward of these %d images' % B)
    if scratch.dtype != torch.float32 or scratch.numel() * 4 < nb or d_params.dtype != torch.float32 or d_params.numel() != lib.nerfail_cnn_grad_floats(C):
        raise ValueError('cnn_bwd_weights_into: scratch needs %d float32, d_params %d' % (nb // 4, lib.nerfail_cnn_grad_floats(C)))
    _chk(lib.nerfail_cnn_bwd_weights(_lib.dev(packed), C, _lib.dev(x, 'x'), _lib.dev(workspace), _lib.dev(masks), _lib.dev(d_logits, 'd_logits'),
                                     B, H, W, _lib.dev(scratch, 'scratch'), _lib.dev(d_params, 'd_params'), None, _s()))


def cnn_bwd_weights_scratch_floats(B, H, W, num_classes):
    return _lib.load().nerfail_cnn_bwd_weights_scratch_bytes(B, H, W, num_classes) // 4


CLS_OPS = ('cls_batch', 'cls_ce', 'cnn_bwd_weights_into', 'cnn_sgd_step', 'cls_epoch_close')


# ----------------------------------------------------------------------------------------------- 2-D baseline (attack_IGSM_2D.py:263-416, GN:340-385; u2d revision 1)
def _u2d_shapes(images, idx, name):
    fmt = _cls_format(images)
    if idx.dtype != torch.int64 or idx.dim() != 1:
        raise ValueError('%s: idx must be int64 [B]' % name)
    N = images.shape[0]
    P = images[0].numel() // images.shape[-1] if N else 0
    return fmt, N, P, idx.shape[0], tuple(images.shape[1:-1])


@custom_op(NS + '::u2d_fwd', mutates_args=(), device_types='cuda')
def u2d_fwd(images: Tensor, idx: Tensor, r: Tensor, want_x_rgb: bool, want_cls_in: bool, want_mask: bool) -> tuple[Tensor, Tensor, Tensor]:
    """GN:356-370 for the views idx (int64 [B], on the device) of a resident uint8 store [N,...,4|3]: (x_rgb float32 [B,...,3] =
    clip(white(ori) + r, 0, 255), cls_in float32 [B,3,...] = the same planar, pass_mask uint8 [B,...] = where the clip's backward
    passes, one bit per channel) - an empty tensor for each output not wanted. r: the table [N,...,3], view b using row idx[b],
    or one shared plane [...,3]."""
    fmt, N, P, B, hw = _u2d_shapes(images, idx, 'u2d_fwd')
    if not (want_x_rgb or want_cls_in):
        raise ValueError('u2d_fwd: x_rgb or cls_in must be wanted')
    shared = r.dim() == images.dim() - 1
    if r.dtype != torch.float32 or not r.is_contiguous() or r.numel() != (1 if shared else N) * P * 3:
        raise ValueError('u2d_fwd: r must be contiguous float32 [N,...,3], or one plane [...,3]')
    dev = images.device
    x_rgb = torch.empty((B,) + hw + (3,) if want_x_rgb else (0,), dtype=torch.float32, device=dev)
    cls_in = torch.empty((B, 3) + hw if want_cls_in else (0,), dtype=torch.float32, device=dev)
    mask = torch.empty((B,) + hw if want_mask else (0,), dtype=torch.uint8, device=dev)
    _chk(_lib.load().nerfail_u2d_fwd(_lib.dev(images, 'images'), fmt, N, P, _lib.dev(idx, 'idx'), B, _lib.dev(r, 'r'), int(shared),
                                     _lib.dev(x_rgb) if want_x_rgb else None, _lib.dev(cls_in) if want_cls_in else None,
                                     _lib.dev(mask) if want_mask else None, _s()))
    return x_rgb, cls_in, mask


@u2d_fwd.register_fake
def _(images, idx, r, want_x_rgb, want_cls_in, want_mask):
    B, hw = idx.shape[0], tuple(images.shape[1:-1])
    return (images.new_empty((B,) + hw + (3,) if want_x_rgb else (0,), dtype=torch.float32),
            images.new_empty((B, 3) + hw if want_cls_in else (0,), dtype=torch.float32),
            images.new_empty((B,) + hw if want_mask else (0,), dtype=torch.uint8))


@custom_op(NS + '::u2d_step', mutates_args=('r',), device_types='cuda')
def u2d_step(r: Tensor, idx: Tensor, d_cls_in: Tensor, pass_mask: Tensor, r_init: Optional[Tensor], a: float, epsilon: float,
             targeted: bool) -> None:
    """IG:335-379 in place on rows idx (int64 [B], distinct) of the table r [N,...,3]: the clip's backward (pass_mask) applied to
    d_cls_in [B,3,...], the sign step, the clamp to r_init +- epsilon (r_init None: the zero table)."""
    if r.dtype != torch.float32 or not r.is_contiguous() or r.dim() < 3 or r.shape[-1] != 3:
        raise ValueError('u2d_step: r must be a contiguous float32 table [N,...,3]')
    if idx.dtype != torch.int64 or idx.dim() != 1:
        raise ValueError('u2d_step: idx must be int64 [B]')
    N, B = r.shape[0], idx.shape[0]
    P = r[0].numel() // 3 if N else 0
    if d_cls_in.dtype != torch.float32 or not d_cls_in.is_contiguous() or d_cls_in.numel() != B * 3 * P:
        raise ValueError('u2d_step: d_cls_in must be contiguous float32 [B,3,...]')
    if pass_mask.dtype != torch.uint8 or not pass_mask.is_contiguous() or pass_mask.numel() != B * P:
        raise ValueError('u2d_step: pass_mask must be contiguous uint8 [B,...]')
    if r_init is not None and (r_init.dtype != torch.float32 or not r_init.is_contiguous() or r_init.shape != r.shape):
        raise ValueError('u2d_step: r_init must be a contiguous float32 tensor with the shape of r')
    _chk(_lib.load().nerfail_u2d_step(_lib.dev(r, 'r'), N, P, _lib.dev(idx, 'idx'), B, _lib.dev(d_cls_in, 'd_cls_in'),
                                      _lib.dev(pass_mask, 'pass_mask'), _lib.dev(r_init, 'r_init'), a, epsilon, int(targeted), _s()))


def u2d_sqerr(x_rgb, images, idx, scratch, row):
    """IG:316: adds sum (x_rgb - white(ori))^2 over the views idx and the element count into the stats row (nerfail_u2d_sqerr)."""
    fmt, N, P, B, _ = _u2d_shapes(images, idx, 'u2d_sqerr')
    _row_ok(row)
    if x_rgb.dtype != torch.float32 or not x_rgb.is_contiguous() or x_rgb.numel() != B * P * 3:
        raise ValueError('u2d_sqerr: x_rgb must be contiguous float32 [B,...,3]')
    if scratch.numel() * scratch.element_size() < _lib.load().nerfail_img_sqerr_scratch_bytes():
        raise ValueError('u2d_sqerr: scratch is smaller than nerfail_img_sqerr_scratch_bytes()')
    _chk(_lib.load().nerfail_u2d_sqerr(_lib.dev(x_rgb, 'x_rgb'), _lib.dev(images, 'images'), fmt, N, P, _lib.dev(idx, 'idx'), B,
                                       _lib.c_p(scratch.data_ptr()), _lib.dev(row), _s()))


def u2d_epoch_close(row, best, epoch, targeted, record, flag):
    """IG:392-416: attack_epoch_close with the strict rule (a tie keeps the earlier epoch)."""
    _row_ok(row)
    _row_ok(record, 'record')
    if best.dtype != torch.float32 or best.numel() != 4 or flag.dtype != torch.int32 or flag.numel() != 1:
        raise ValueError('best must be float32 [4] and flag int32 [1]')
    _chk(_lib.load().nerfail_u2d_epoch_close(_lib.dev(row), _lib.dev(best), epoch, int(targeted), _lib.dev(record), _lib.dev(flag), _s()))


U2D_OPS = ('u2d_fwd', 'u2d_step')


# ----------------------------------------------------------------------------------------------- 2-D universal baseline (attack_UAP_2D.py:241-358; uap2d revision 1)
def uap2d_step_scratch(n_rhs, P, device):
    """(scratch as float64, its size in bytes) of uap2d_step: the partials, then {norms2[8], best, scale}."""
    nb = _lib.load().nerfail_uap2d_step_scratch_bytes(int(n_rhs), int(P))
    if nb == 0:
        raise ValueError('uap2d_step: n_rhs must be in 2..8 and P in 1..2^31 (got %d, %d)' % (n_rhs, P))
    return torch.empty((nb // 8,), dtype=torch.float64, device=device), nb


def uap2d_step(grads, pass_mask, record, scratch, overshoot, r0, rot, r_out, trace_slot):
    """DF:68-102 with universal_2d in one call (nerfail_uap2d_step): grads float32 [n_rhs,...] holding n_rhs x 3 x P planar
    class gradients of ONE view, row 0 the clean class; pass_mask uint8 [P] of that view's u2d_fwd; record: the gate's;
    r0 / rot / r_out float32 [P,3] interleaved (views into larger buffers allowed, as long as each is dense); trace_slot: one
    int32. rot is updated in place, r_out written."""
    P = pass_mask.numel()
    n_rhs = grads.shape[0]
    for t, name in ((grads, 'grads'), (r0, 'r0'), (rot, 'rot'), (r_out, 'r_out')):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('uap2d_step: %s must be contiguous float32' % name)
    if grads.numel() != n_rhs * 3 * P or r0.numel() != 3 * P or rot.numel() != 3 * P or r_out.numel() != 3 * P:
        raise ValueError('uap2d_step: grads must hold n_rhs x 3 x P floats and r0, rot, r_out 3 P each (P = %d)' % P)
    if pass_mask.dtype != torch.uint8 or not pass_mask.is_contiguous():
        raise ValueError('uap2d_step: pass_mask must be contiguous uint8 [P]')
    if record.dtype != torch.int32 or record.numel() != _lib.DEEPFOOL_RECORD_WORDS or trace_slot.dtype != torch.int32 or trace_slot.numel() != 1:
        raise ValueError('uap2d_step: record must be int32 [%d] and trace_slot int32 [1]' % _lib.DEEPFOOL_RECORD_WORDS)
    nb = scratch.numel() * scratch.element_size()
    _chk(_lib.load().nerfail_uap2d_step(_lib.dev(grads, 'grads'), n_rhs, P, _lib.dev(pass_mask, 'pass_mask'), _lib.dev(record, 'record'),
                                        _lib.c_p(scratch.data_ptr()), nb, float(overshoot), _lib.dev(r0, 'r0'), _lib.dev(rot, 'rot'),
                                        _lib.dev(r_out, 'r_out'), _lib.dev(trace_slot, 'trace_slot'), _s()))


def uap2d_accumulate(table, r_final, epsilon):
    """UA:317-319 with DF:109 in place: table <- clamp(table + (r_final - table), -epsilon, +epsilon) (nerfail_uap2d_accumulate)."""
    for t, name in ((table, 'table'), (r_final, 'r_final')):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('uap2d_accumulate: %s must be contiguous float32' % name)
    if table.numel() != r_final.numel():
        raise ValueError('uap2d_accumulate: table and r_final differ in size')
    _chk(_lib.load().nerfail_uap2d_accumulate(_lib.dev(table, 'table'), _lib.dev(r_final, 'r_final'), float(epsilon), table.numel(), _s()))


# ----------------------------------------------------------------------------------------------- poisoned retrain hand-off (LB:62-65, RN:587-588; poison revision 1)
@custom_op(NS + '::export_train_views', mutates_args=('adv_u8', 'target'), device_types='cuda')
def export_train_views(x: Tensor, slots: Sequence[int], adv_u8: Tensor, target: Tensor) -> None:
    """The export of B views, x float32 [B,...,4] (BGRA) or [B,...,3] (BGR), into slots `slots` (host ints, distinct) of two
    resident stores: adv_u8 uint8 [n,...,C], bit for bit export_u8(x[b]), and target float32 [n,...,3] in RGB order, bit for bit
    what load_blender_data(train_dir=...) and training_images(white_bkgd=True) make of that uint8 image."""
    if x.dtype != torch.float32 or x.dim() < 3 or x.shape[-1] not in (3, 4) or not x.is_contiguous():
        raise ValueError('export_train_views: x must be contiguous float32 [B,...,4] (BGRA) or [B,...,3] (BGR)')
    B, C = x.shape[0], x.shape[-1]
    P = x[0].numel() // C if B else 0
    n = adv_u8.shape[0] if adv_u8.dim() else 0
    if adv_u8.dtype != torch.uint8 or not adv_u8.is_contiguous() or adv_u8.numel() != n * P * C:
        raise ValueError('export_train_views: adv_u8 must be a contiguous uint8 store [n,...,%d] of views of %d pixels' % (C, P))
    if target.dtype != torch.float32 or not target.is_contiguous() or target.numel() != n * P * 3 or target.shape[0] != n:
        raise ValueError('export_train_views: target must be a contiguous float32 store [n,...,3] with adv_u8\'s n')
    if len(slots) != B:
        raise ValueError('export_train_views: one slot per view of x')
    if B == 0:
        return
    if any(not 0 <= int(s) < n for s in slots):                           # (also the C side's answer; here before the int32 conversion)
        raise ValueError('export_train_views: a slot is outside 0..%d' % (n - 1))
    tab = (_lib.ctypes.c_int32 * B)(*[int(s) for s in slots])
    _chk(_lib.load().nerfail_export_train_views(_lib.dev(x, 'x'), C, B, P, tab, n, _lib.dev(adv_u8, 'adv_u8'), _lib.dev(target, 'target'), _s()))


@export_train_views.register_fake
def _(x, slots, adv_u8, target):
    return None


POISON_OPS = ('export_train_views',)


# ----------------------------------------------------------------------------------------------- classifier-input resize (GN:121-157; resize revision 1)
def _resize_axes(H, W, oh, ow, device):
    from ._resize import axis_tables
    return axis_tables(H, oh, device), axis_tables(W, ow, device)


@custom_op(NS + '::cls_input_resize', mutates_args=(), device_types='cuda')
def cls_input_resize(src: Tensor, layout: int, oh: int, ow: int) -> Tensor:
    """The classifier input [B,3,oh,ow] of src: layout 0 = [B,H,W,4] (white where alpha > 0 is false), layout 1 = [B,3,H,W]."""
    if layout not in (0, 1) or src.dim() != 4 or src.dtype != torch.float32 or src.shape[3 if layout == 0 else 1] != (4 if layout == 0 else 3):
        raise ValueError('cls_input_resize: src must be float32 [B,H,W,4] (layout 0) or [B,3,H,W] (layout 1)')
    B = src.shape[0]
    H, W = (src.shape[1], src.shape[2]) if layout == 0 else (src.shape[2], src.shape[3])
    ty, tx = _resize_axes(H, W, oh, ow, src.device)
    out = torch.empty((B, 3, oh, ow), dtype=torch.float32, device=src.device)
    _chk(_lib.load().nerfail_cls_input_resize_fwd(_lib.dev(src, 'src'), layout, B, H, W, oh, ow, ty.ref, tx.ref, _lib.dev(out), _s()))
    return out


@cls_input_resize.register_fake
def _(src, layout, oh, ow):
    return src.new_empty((src.shape[0], 3, oh, ow))


@custom_op(NS + '::cls_input_resize_bwd', mutates_args=(), device_types='cuda')
def cls_input_resize_bwd(g: Tensor, src: Optional[Tensor], layout: int, H: int, W: int) -> Tensor:
    """The adjoint of cls_input_resize for g [R,B,3,oh,ow], 1 <= R <= 8: [R,B,H,W,4] (layout 0; src = the forward's input, read for
    its alpha) or [R,B,3,H,W] (layout 1; src unused). Slice r is bitwise the R = 1 result for g[r]."""
    if layout not in (0, 1) or g.dim() != 5 or g.dtype != torch.float32 or g.shape[2] != 3:
        raise ValueError('cls_input_resize_bwd: g must be float32 [R,B,3,oh,ow]')
    R, B, _, oh, ow = g.shape
    if layout == 0 and (src is None or tuple(src.shape) != (B, H, W, 4) or src.dtype != torch.float32):
        raise ValueError('cls_input_resize_bwd: layout 0 needs the forward\'s float32 src [B,H,W,4]')
    ty, tx = _resize_axes(H, W, oh, ow, g.device)
    out = torch.empty((R, B, H, W, 4) if layout == 0 else (R, B, 3, H, W), dtype=torch.float32, device=g.device)
    _chk(_lib.load().nerfail_cls_input_resize_bwd(_lib.dev(g, 'g'), R, _lib.dev(src, 'src') if layout == 0 else None, layout, B, H, W, oh, ow,
                                                  ty.ref, tx.ref, _lib.dev(out), _s()))
    return out


@cls_input_resize_bwd.register_fake
def _(g, src, layout, H, W):
    return g.new_empty((g.shape[0], g.shape[1], H, W, 4) if layout == 0 else (g.shape[0], g.shape[1], 3, H, W))


def _resize_setup(ctx, inputs, output):
    src, layout, oh, ow = inputs
    ctx.layout = layout
    ctx.hw = (src.shape[1], src.shape[2]) if layout == 0 else (src.shape[2], src.shape[3])
    ctx.save_for_backward(*((src,) if layout == 0 else ()))


def _resize_backward(ctx, g):
    src = ctx.saved_tensors[0] if ctx.layout == 0 else None
    return cls_input_resize_bwd(g.contiguous()[None], src, ctx.layout, ctx.hw[0], ctx.hw[1])[0], None, None, None


cls_input_resize.register_autograd(_resize_backward, setup_context=_resize_setup)

RESIZE_OPS = ('cls_input_resize', 'cls_input_resize_bwd')
