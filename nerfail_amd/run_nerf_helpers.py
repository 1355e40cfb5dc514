"""MI355X mirror of Create_spatial_point_set/nerf_pytorch/run_nerf_helpers.py (reference = RH).

Same names, argument meaning and return structure as the reference; every numeric path runs in
libnerfail_hip.so (HIP, gfx950). No CPU fallback: CPU tensors are moved to the GPU, results live there.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._images import ImageCache

# Misc (RH:9-11) - host-side one-liners, kept for drop-in completeness
class _Img2Mse(torch.autograd.Function):
    """sum((x - y)^2) / n_total and its gradient w.r.t. x from ONE launch (nerfail_mse_part; n_total None = x.numel(): the
    mean, nerfail_mse's bits); the backward is one multiply."""

    @staticmethod
    def forward(ctx, x, y, n_total=None):
        xc, yc = _lib.f32c(x), _lib.f32c(y)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(xc) if x.requires_grad else None
        n = xc.numel()
        _lib.check(_lib.load().nerfail_mse_part(_lib.dev(xc), _lib.dev(yc), n, n if n_total is None else int(n_total), _lib.dev(loss),
                                                _lib.dev(dx), _lib.stream()))
        ctx.dx = dx
        return loss

    @staticmethod
    def backward(ctx, g):
        return (None if ctx.dx is None else ctx.dx * g), None, None


# the fused kernel is ONE workgroup (fixed-order tree, bitwise reproducible): right for a training batch (1024 rays x 3 = 3072
# values: 3 sweeps per thread), a serial crawl for an image - anything larger takes torch's multi-workgroup reduction
MSE_FUSED_MAX = 1 << 16


def img2mse(x, y, n_total=None):
    """RH:9. On the MI355X (float32 HIP tensors of equal shape, target without gradient) one fused kernel; any other
    input takes the reference's expression.
    n_total (data-parallel training): x and y are this rank's share of a batch of n_total >= x.numel() VALUES; the result is
    sum((x - y)^2) / n_total, so that the ranks' losses add up to the global mean and their gradients to its gradient."""
    if n_total is not None and int(n_total) < x.numel():
        raise ValueError('img2mse: n_total = %d is smaller than the %d values given' % (int(n_total), x.numel()))
    if (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.is_cuda and y.is_cuda and x.dtype == torch.float32
            and y.dtype == torch.float32 and x.shape == y.shape and not y.requires_grad and 0 < x.numel() <= MSE_FUSED_MAX):
        return _Img2Mse.apply(x, y, n_total)
    if n_total is not None:
        return torch.sum((x - y) ** 2) / float(int(n_total))
    return torch.mean((x - y) ** 2)


mse2psnr = lambda x: -10. * torch.log(x) / torch.log(torch.Tensor([10.]).to(x.device))
to8b = lambda x: (255 * np.clip(x, 0, 1)).astype(np.uint8)


def _cuda():
    if not torch.cuda.is_available():
        raise RuntimeError('nerfail_amd needs an MI355X (torch.cuda.is_available() is False); no CPU path exists')
    return torch.device('cuda', torch.cuda.current_device())


# ----------------------------------------------------------------------------- positional encoding
class Embedder:
    """RH:15-50 with include_input=True, log_sampling=True, periodic_fns=[sin, cos] (get_embedder's kwargs)."""

    def __init__(self, multires):
        self.multires = int(multires)
        self.out_dim = 3 + 6 * self.multires

    def embed(self, inputs):
        x = _lib.f32c(inputs, _cuda())
        assert x.shape[-1] == 3, 'input_dims is 3 (RH:58)'
        flat = x.reshape(-1, 3)
        out = torch.empty((flat.shape[0], self.out_dim), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().nerfail_embed(_lib.dev(flat, 'inputs'), flat.shape[0], self.multires,
                                             _lib.dev(out), _lib.stream()))
        return out.reshape(x.shape[:-1] + (self.out_dim,))

    __call__ = embed


def get_embedder(multires, i=0, device=None):
    """RH:52-67. Returns (embed_fn, out_dim); embed_fn carries .multires so run_network can fuse it."""
    if i == -1:
        return nn.Identity(), 3
    eo = Embedder(multires)
    return eo, eo.out_dim


# ----------------------------------------------------------------------------- model
class NeRF(nn.Module):
    """RH:71-123: identical constructor, parameter names (state_dict keys) and forward contract.

    forward(x) takes the embedded batch [M, input_ch + input_ch_views] like the reference and runs the
    whole MLP in one HIP kernel. The render path does not go through forward(): run_network() hands
    raw points to the fused encode+MLP kernel. Every path goes through mlp_forward() below.

    The kernels read device weight images, not the parameters: f32 (packed()), its bf16x3 splits x3 and x3f (packed_x3(),
    packed_x3f()), the fp16 hi/lo image f16 (packed_f16()) and, for the backward-data pass, the transposed f32_T and f16_T
    (_train.packed_T(), packed_f16_T()). All six live in ONE cache (_images.ImageCache, whose docstring has the rules): packed
    when first asked for, dropped together when any parameter is written in place or moved."""

    def __init__(self, D=8, W=256, input_ch=3, input_ch_views=3, output_ch=4, skips=[4], use_viewdirs=False):
        super(NeRF, self).__init__()
        self.D = D
        self.W = W
        self.input_ch = input_ch
        self.input_ch_views = input_ch_views
        self.skips = skips
        self.use_viewdirs = use_viewdirs
        self.pts_linears = nn.ModuleList(
            [nn.Linear(input_ch, W)] + [nn.Linear(W, W) if i not in self.skips else nn.Linear(W + input_ch, W)
                                        for i in range(D - 1)])
        self.views_linears = nn.ModuleList([nn.Linear(input_ch_views + W, W // 2)])
        if use_viewdirs:
            self.feature_linear = nn.Linear(W, W)
            self.alpha_linear = nn.Linear(W, 1)
            self.rgb_linear = nn.Linear(W // 2, 3)
        else:
            self.output_linear = nn.Linear(W, output_ch)
        self._images = ImageCache(self.ordered_params, {          # name: (packer, the image it is made from)
            'f32': (self._pack_f32, None), 'f32_T': (self._pack_f32_T, None), 'x3': (self._pack_x3, 'f32'),
            'x3f': (self._pack_x3f, 'f32'), 'f16': (self._pack_f16, None), 'f16_T': (self._pack_f16_T, None)})
        self._f16_checked_once = False                            # state of check_f16x3_range: the first pack waits,
        self._f16_pending = self._f16_host = None                 # later ones leave an event and a pinned float to look at
        # 'f32' : exact-f32 MFMA kernel (default).  'f16x3': split-precision fp16 MFMA kernel, fp32-equivalent
        # results (each product as a_hi*w_hi + a_hi*w_lo + a_lo*w_hi with fp32 accumulation), inference only.
        self.precision = 'f32'

    def _skip(self):
        s = [i for i in self.skips if i < self.D - 1]
        if len(s) > 1:
            raise NotImplementedError('one skip connection supported (the reference always uses skips=[4])')
        return s[0] if s else -1

    def ordered_params(self):
        """The parameters in the one order of the image key, nerfail_mlp_params and the gradients of the training step:
        pts_linears (w, b) * D, views, feature, alpha, rgb."""
        if not self.use_viewdirs:
            raise NotImplementedError('HIP path implements use_viewdirs=True (all NeRFail configs, configs/*.txt)')
        ps = []
        for l in list(self.pts_linears) + [self.views_linears[0], self.feature_linear, self.alpha_linear, self.rgb_linear]:
            ps += [l.weight, l.bias]
        return ps

    def _mlp_params(self, keep):
        return _lib.mlp_params(self.D, self.W, self.input_ch, self.input_ch_views, self._skip(), self.ordered_params(), keep)

    # -- the packers of the image table: each allocates and fills, the cache decides when
    def _pack(self, pack, *sizes):
        """Fresh buffers of the sizes the named queries give, filled from the parameters by ONE launch of the named packer."""
        lib, dev, shape = _lib.load(), self.pts_linears[0].weight.device, (self.D, self.W, self._skip())
        if dev.type != 'cuda':
            raise RuntimeError('NeRF parameters are on %s: call .cuda() - there is no CPU path' % dev)
        bufs = []
        for query in sizes:
            n = getattr(lib, query)(*shape)
            if n == 0:
                raise NotImplementedError('unsupported NeRF shape D=%d W=%d (W in {64,128,256})' % (self.D, self.W))
            bufs.append(torch.empty((n,), dtype=torch.float32 if query.endswith('_floats') else torch.uint8, device=dev))
        keep = []
        mp = self._mlp_params(keep)
        _lib.check(getattr(lib, pack)(mp, *[_lib.dev(b) for b in bufs], _lib.stream()))
        return bufs

    def _pack_f32(self):
        return self._pack('nerfail_mlp_pack', 'nerfail_mlp_packed_floats')[0]

    def _pack_f32_T(self):
        return self._pack('nerfail_mlp_pack_T', 'nerfail_mlp_packed_T_floats')[0]

    def _pack_both(self):
        return self._pack('nerfail_mlp_pack_train', 'nerfail_mlp_packed_floats', 'nerfail_mlp_packed_T_floats')

    def _pack_f16(self):
        self.check_f16x3_range()
        return self._pack('nerfail_mlp_pack_f16', 'nerfail_mlp_f16_image_bytes')[0]

    def _pack_f16_T(self):
        self.check_f16x3_range()
        return self._pack('nerfail_mlp_pack_f16_T', 'nerfail_mlp_f16_image_T_bytes')[0]

    def _pack_x3(self, f32, pack='nerfail_mlp_pack_x3', size='nerfail_mlp_packed_x3_bytes'):
        lib, shape = _lib.load(), (self.D, self.W, self._skip())
        n = getattr(lib, size)(*shape)
        if n == 0:
            return None                                           # a shape the bf16x3 kernel does not cover
        buf = torch.empty((n,), dtype=torch.uint8, device=f32.device)
        _lib.check(getattr(lib, pack)(_lib.dev(f32), *shape, _lib.dev(buf), _lib.stream()))
        return buf

    def _pack_x3f(self, f32):
        buf = self._pack_x3(f32, 'nerfail_mlp_pack_x3f', 'nerfail_mlp_packed_x3f_bytes')
        if buf is not None:                                       # ONE host synchronisation per weight version
            n = _lib.load().nerfail_mlp_x3f_composed_floats(self.D, self.W, self._skip())
            if not bool(torch.isfinite(buf[buf.numel() - 4 * n:].view(torch.float32)).all()):
                return None
        return buf

    # -- the images by name
    def packed(self):
        """f32 image in MFMA fragment order (nerfail_mlp_pack): what every kernel takes first."""
        return self._images.get('f32')

    def packed_both(self):
        """(f32, f32_T) from ONE launch (nerfail_mlp_pack_train): the training step re-packs both after every optimizer step."""
        return self._images.get_joint(('f32', 'f32_T'), self._pack_both)

    def packed_x3(self):
        """bf16x3 weight image of the inference kernel (nerfail_mlp_pack_x3, split on the device from packed()). None for
        shapes the bf16x3 kernel does not cover: the x3 entry points then run the f32 path."""
        return self._images.get('x3')

    def packed_x3f(self):
        """Folded bf16x3 image (nerfail_mlp_pack_x3f): feature_linear composed into views_linears[0] on the device. None for
        shapes the kernel does not cover, and when the composed block Wc / bc is not finite (weights so large that the
        product leaves f32): inference then takes the unfolded image of packed_x3()."""
        return self._images.get('x3f')

    def x3_image(self):
        """(folded, image) of the bf16x3 inference kernel: the folded image where it exists, else the unfolded one (or None)."""
        img = self.packed_x3f()
        return (True, img) if img is not None else (False, self.packed_x3())

    def packed_f16(self):
        """fp16 hi/lo weight image of the split-precision kernel (nerfail_mlp_pack_f16)."""
        self._f16_poll()                                  # an earlier pack's range check, if its value has arrived
        return self._images.get('f16')

    F16X3_MAX_WEIGHT = 60.0       # the split-precision image holds fp16(w * 2^10): |w| * 1024 must stay below 65504

    def check_f16x3_range(self, sync=False):
        """The 'f16x3' kernels pre-scale the weights by 2^10 before the fp16 hi/lo split: a weight of magnitude >= ~64 would
        become inf (and its lo part NaN) - silently wrong results in a mode advertised as fp32-equivalent. EVERY pack
        measures max |weight| on the device (three small kernels). The first pack of a model waits for the value; later ones
        (training re-packs after every optimizer step) copy it to pinned host memory without stalling the stream and the
        NEXT call that touches the split-precision image (`packed_f16`, a pack of the transposed image, this method) looks
        at it: a weight that leaves the range is reported one forward later at the latest, whatever changed it (optimizer
        step, load_state_dict, a manual edit). sync=True waits for the value of this call. Activations are bounded by the same
        mechanism only through the weights: NeRF activations are O(1..100), fp16 range is 65504."""
        self._f16_poll()
        ws = [p.detach() for n_, p in self.named_parameters() if n_.endswith('weight')]
        with torch.no_grad():
            m = torch.stack(torch._foreach_norm(ws, float('inf'))).max()
        if sync or not m.is_cuda or not self._f16_checked_once:
            self._f16_checked_once = True
            self._f16_verdict(float(m))
            return
        # a measurement still on its way is WAITED for before its slot is reused: no verdict is ever overwritten unread
        # (every pack is checked, one forward later at the latest - the training loop packs once per step)
        self._f16_poll(wait=True)
        if self._f16_host is None:
            self._f16_host = torch.empty((1,), dtype=torch.float32).pin_memory()
        self._f16_host.copy_(m.reshape(1), non_blocking=True)
        self._f16_pending = torch.cuda.Event()
        self._f16_pending.record()

    def _f16_poll(self, wait=False):
        """Looks at the max |weight| an earlier pack measured, if it has arrived (or waits for it)."""
        ev = self._f16_pending
        if ev is None:
            return
        if wait:
            ev.synchronize()
        if ev.query():
            self._f16_pending = None
            self._f16_verdict(float(self._f16_host[0]))

    def _f16_verdict(self, m):
        if not m < self.F16X3_MAX_WEIGHT:          # (also catches NaN)
            raise ValueError("NeRF.precision = 'f16x3': max |weight| = %g is outside the range of the split-precision kernels "
                             "(|w| < %g); use precision = 'f32'" % (m, self.F16X3_MAX_WEIGHT))

    def forward(self, x):
        x = _lib.f32c(x, _cuda())
        assert x.shape[-1] == self.input_ch + self.input_ch_views
        flat = x.reshape(-1, x.shape[-1])
        raw = torch.empty((flat.shape[0], 4), dtype=torch.float32, device=flat.device)
        return mlp_forward(self, raw, embedded=flat).reshape(x.shape[:-1] + (4,))


class per_ray_view_bias:
    """Context of a caller that accepts the per-ray view-bias form of the folded bf16x3 kernel for the inference calls it makes
    (the renderer does, run_nerf._render_rays_pipeline): density bitwise the plain folded kernel's, colour f32-accurate but not
    its bits. Outside such a context mlp_forward keeps the plain kernels: the rays, points and embedded forms of one batch
    then give the same bits."""
    depth = 0

    def __enter__(self):
        per_ray_view_bias.depth += 1
        return self

    def __exit__(self, *exc):
        per_ray_view_bias.depth -= 1


def mlp_forward(net, raw, pts=None, viewdirs=None, embedded=None, rays=None, z_vals=None, acts=None):
    """The ONE choice of forward entry point. Input, one of: pts [R,N,3] + viewdirs [R,3] | embedded [M,90] | packed rays
    [R,11] + z_vals [R,N] (the points o + d z are formed inside the kernel). Fills and returns `raw`. With `acts` (the
    activation buffer of a training forward) the pass saves what the backward needs.

      net.precision == 'f16x3', points only  nerfail_mlp_fwd_f16 / nerfail_mlp_fwd_f16_train on the f32 and the f16 image
      inference                              nerfail_mlp_fwd[_embedded|_rays]_x3f on the folded bf16x3 image if there is one,
                                             else ..._x3 on the unfolded one, which runs exact f32 when that is None too
                                             (inside per_ray_view_bias(), rays / points on the folded image with
                                             N % 32 == 0: the ..._x3f_raybias entry points - the view-direction term once
                                             per ray - unless NERFAIL_X3_RAYBIAS=0)
      training (points, rays)                nerfail_mlp_fwd_train / nerfail_mlp_fwd_rays on the f32 image, after the joint
                                             pack: the backward needs the transposed image of the same weights"""
    lib, train = _lib.load(), acts is not None
    if embedded is not None:
        form, inputs = '_embedded', [_lib.dev(embedded, 'x'), embedded.shape[0]]
    elif rays is not None:
        form, inputs = '_rays', [_lib.dev(rays, 'rays'), _lib.dev(z_vals, 'z_vals'), z_vals.shape[0], z_vals.shape[1]]
    else:
        form, inputs = '', [_lib.dev(pts, 'pts'), _lib.dev(viewdirs, 'viewdirs'), pts.shape[0] * pts.shape[1], pts.shape[1]]
    if net.precision == 'f16x3' and form == '':
        name, images = 'nerfail_mlp_fwd_f16' + ('_train' if train else ''), [net.packed(), net.packed_f16()]
    elif train:
        if form == '_embedded':
            raise NotImplementedError('no training forward on an embedded batch')
        name, images = 'nerfail_mlp_fwd' + (form or '_train'), [net.packed_both()[0]]
    else:
        fold, img = net.x3_image()
        name, images = 'nerfail_mlp_fwd%s_x3%s' % (form, 'f' if fold else ''), [net.packed(), img]
        # a caller inside per_ray_view_bias(), folded image, rays or points with view directions, whole 32-sample tiles per ray:
        # the view-direction term once per ray (nerfail_mlp_x3f_raybias_floats says whether the library runs that form for
        # this call, and how large vb is)
        n_rays = 0 if form == '_embedded' else (inputs[2] if form == '_rays' else inputs[2] // inputs[3])
        n_vb = lib.nerfail_mlp_x3f_raybias_floats(net.D, net.W, net._skip(), n_rays, inputs[-1]) \
            if fold and n_rays and per_ray_view_bias.depth > 0 else 0
        if n_vb:
            vb = torch.empty((n_vb,), dtype=torch.float32, device=raw.device)     # a temporary of the call, like raw
            _lib.check(getattr(lib, name + '_raybias')(*[_lib.dev(i) for i in images], net.D, net.W, net._skip(), *inputs,
                                                       _lib.dev(raw), _lib.dev(vb), _lib.stream()))
            return raw
    tail = [_lib.dev(acts)] if train or form == '_rays' else []       # the rays entry points take acts (or NULL) always
    _lib.check(getattr(lib, name)(*[_lib.dev(i) for i in images], net.D, net.W, net._skip(), *inputs, _lib.dev(raw), *tail,
                                  _lib.stream()))
    return raw


# ----------------------------------------------------------------------------- rays
def _k4(K):
    return _lib.host_floats([K[0][0], K[1][1], K[0][2], K[1][2]])


def _c2w12(c2w):
    c = torch.as_tensor(c2w).detach().to('cpu', torch.float32)[:3, :4].reshape(-1).tolist()
    return _lib.host_floats(c)


def get_rays(H, W, K, c2w):
    """RH:157-166 -> rays_o [H,W,3], rays_d [H,W,3] on the GPU."""
    dev = _cuda()
    rays_o = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    rays_d = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().nerfail_get_rays(int(H), int(W), _k4(K), _c2w12(c2w), _lib.dev(rays_o), _lib.dev(rays_d),
                                            _lib.stream()))
    return rays_o, rays_d


def get_rays_np(H, W, K, c2w):
    """RH:169-176 (numpy twin used by the batching loader): same kernel, copied back to the host."""
    o, d = get_rays(H, W, K, c2w)
    return o.cpu().numpy(), d.cpu().numpy()


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    raise NotImplementedError('ndc_rays (RH:179-196) is LLFF-only; every NeRFail config sets ndc=False (RN:250-252)')


# ----------------------------------------------------------------------------- hierarchical sampling
_LINSPACE = {}


def linspace01(n, device):
    """torch.linspace(0,1,n) computed by the CPU kernel (the reference's bits), cached on the device."""
    key = (int(n), str(device))
    if key not in _LINSPACE:
        _LINSPACE[key] = torch.linspace(0., 1., steps=int(n)).to(device)
    return _LINSPACE[key]


def sample_pdf(bins, weights, N_samples, det=False, pytest=False, u=None):
    """RH:200-243. `u` (optional [R, N_samples]) supplies the uniform draws explicitly ("identical seeds")."""
    dev = _cuda()
    bins = _lib.f32c(bins, dev)
    weights = _lib.f32c(weights, dev)
    lead = bins.shape[:-1]
    nb = bins.shape[-1]
    assert weights.shape[-1] == nb - 1
    b2, w2 = bins.reshape(-1, nb), weights.reshape(-1, nb - 1)
    R = b2.shape[0]
    if pytest:                                             # RH:215-223
        np.random.seed(0)
        if det:
            u = torch.Tensor(np.linspace(0., 1., N_samples)).to(dev)
        else:
            u = torch.Tensor(np.random.rand(*(list(lead) + [N_samples]))).to(dev)
    elif u is None:
        u = linspace01(N_samples, dev) if det else torch.rand(list(lead) + [N_samples], device=dev)
    u = _lib.f32c(u, dev)
    is_row = int(u.dim() == 1)
    if not is_row:
        u = u.reshape(R, N_samples)
    from . import ops  # noqa: F401
    out = torch.ops.nerfail_mi.sample_pdf(b2, w2, u)                                        # K6 as a registered op
    return out.reshape(tuple(lead) + (N_samples,))
