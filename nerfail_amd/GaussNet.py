"""MI355X mirror of model/GaussNet.py (reference = GN): the differentiable pixel <-> 3-D-point map.

gauss_net.forward keeps its signature and 5-tuple return. The hot part (GN:53-119: 8-NN gather, weighted
sum, alpha, epsilon clip, composite onto the image) is one HIP kernel with a hand-written backward
(scatter-add with float atomics); the cold tail (GN:121-157: layout change, white background, Resize,
classifier) stays stock PyTorch, as SURVEY.md section 8(a16) scopes it.
"""
import ctypes
import functools

import torch
from torch import nn

from . import _lib
from . import ops  # noqa: F401  (registers torch.ops.nerfail_mi.*)
from ._resize import resize, classifier_input, axis_tables
from .run_nerf_helpers import _cuda
# the view store, the batch object and the logit cache: nerfail_amd/views.py (its module docstring lists their rules); the names
# stay importable from here
from .views import (GaussCSR, csr_for, ViewIndex, view_table, fingerprints, _view_key, _file_sig, view_indices,  # noqa: F401
                    load_view_indices, register_view_index, register_view, load_view_maps, resident, BatchViews, resolve_views,
                    OriLogitCache, ori_logit_key, _CSR_CACHE, CSR_CACHE_SIZE, _VIEW_CACHE, VIEW_CACHE_BYTES, _BATCH_KEYS,
                    _VIEW_MAPS, _VIEW_ORI, _VIEW_ORI_EPOCH, _VIEW_PASSED_OK, VIEW_MAPS_BYTES)


def hot_forward(spatial_rgb, views, epsilon=None, eps_minmax=None, need_x=True, need_aux=False):
    """K10 over a BatchViews: (x or None, x_rgba, (aux_alpha, aux_mask) or None); no autograd."""
    dev = _cuda()
    s = _lib.f32c(spatial_rgb, dev).reshape(-1, 4)
    B, H, W = views.B, views.H, views.W
    x = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev) if need_x else None
    x_rgba = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
    aux = (torch.empty((B, H, W), dtype=torch.float32, device=dev), torch.empty((B, H, W), dtype=torch.uint8, device=dev)) if need_aux else None
    eps = -1.0 if epsilon is None else float(epsilon)
    _lib.check(_lib.load().nerfail_gauss_fwd_views(_lib.dev(s, 'spatial_rgb'), s.shape[0], views.table(), B, views.P, int(views.ori_u8), eps,
                                                   _lib.dev(x), _lib.dev(x_rgba), _lib.dev(aux[0]) if aux else None,
                                                   _lib.dev(aux[1]) if aux else None, _lib.dev(eps_minmax), _lib.stream()))
    return x, x_rgba, aux


def hot_backward_rgb(aux, grad_x_rgba, views, out=None):
    """K11, rgb-gradient-only form: d/d(spatial rgb) as [Ns,3] (flat buffer `out` of >= 3 Ns floats, e.g. with a tail slot
    for the loss so that ONE all-reduce moves both)."""
    dev = grad_x_rgba.device
    Ns = views.Ns
    table, scratch = views.index_table()
    if out is None:
        out = torch.empty((3 * Ns,), dtype=torch.float32, device=dev)
    gr = _lib.f32c(grad_x_rgba)
    _lib.check(_lib.load().nerfail_gauss_bwd_views_rgb(_lib.dev(aux[0]), _lib.dev(aux[1]), _lib.dev(gr), table, views.B, Ns, views.P,
                                                       _lib.dev(scratch), _lib.dev(out), _lib.stream()))
    return out


def hot_backward_rgb_step(aux, grad_x_rgba, views, spatial, spatial_init, a, epsilon, targeted, grad_out=None):
    """K11 (rgb form) + K12 in one pass (nerfail_gauss_bwd_views_rgb_step, round 6): the new perturbation table after the sign step
    AS:352-392; the gradient itself is written only if `grad_out` (>= 3 Ns floats) is given. Bit-identical to hot_backward_rgb
    followed by attack.igsm_step_rgb."""
    dev = grad_x_rgba.device
    Ns = views.Ns
    table, scratch = views.index_table()
    s, s0 = _lib.f32c(spatial, dev), _lib.f32c(spatial_init, dev)
    if s.numel() != 4 * Ns or s0.numel() != 4 * Ns:
        raise ValueError('spatial / spatial_init must hold Ns = %d rows of 4 floats' % Ns)
    if grad_out is None and views.B > 16:
        grad_out = torch.empty((3 * Ns,), dtype=torch.float32, device=dev)
    out = torch.empty_like(s)
    _lib.check(_lib.load().nerfail_gauss_bwd_views_rgb_step(_lib.dev(aux[0]), _lib.dev(aux[1]), _lib.dev(_lib.f32c(grad_x_rgba)), table, views.B,
                                                           Ns, views.P, _lib.dev(scratch), _lib.dev(grad_out), _lib.dev(s), _lib.dev(s0),
                                                           float(a), float(epsilon), int(bool(targeted)), _lib.dev(out), _lib.stream()))
    return out


class _GaussGather(torch.autograd.Function):
    """x, x_rgba = f(spatial_rgb); d/d(spatial_rgb) by the hand-written backward. The views carry no grad.

    deterministic=True : gather-reduce over the cached per-view inverted indices (no atomics, bitwise reproducible).
    deterministic=False: scatter with float atomics (nerfail_gauss_bwd; no setup, order-dependent last bits)."""

    @staticmethod
    def forward(ctx, spatial, views, epsilon, eps_minmax, deterministic):
        x, x_rgba, _ = hot_forward(spatial, views, epsilon, eps_minmax, need_x=True)
        ctx.save_for_backward(x)
        ctx.views = views
        ctx.eps = -1.0 if epsilon is None else float(epsilon)
        ctx.s_shape = tuple(spatial.shape)
        ctx.deterministic = bool(deterministic)
        return x, x_rgba

    @staticmethod
    def backward(ctx, grad_x, grad_x_rgba):
        (x,) = ctx.saved_tensors
        views = ctx.views
        lib = _lib.load()
        B, P = views.B, views.P
        n = 1
        for d in ctx.s_shape[:-1]:
            n *= d
        gx = _lib.f32c(grad_x) if grad_x is not None else None
        gr = _lib.f32c(grad_x_rgba) if grad_x_rgba is not None else None
        ori = views.ori_float()
        if ctx.deterministic:
            # every view reduced over its own index, the views' row sums added in view order (fixed order: bitwise
            # reproducible whatever else is in the cache)
            gs = torch.empty((n, 4), dtype=torch.float32, device=x.device)
            table, scratch = views.index_table()
            _lib.check(lib.nerfail_gauss_bwd_views(_lib.dev(ori), _lib.dev(x), _lib.dev(gx), _lib.dev(gr), table, B, n, P,
                                                   ctx.eps, _lib.dev(scratch), _lib.dev(gs), _lib.stream()))
        else:
            gs = torch.zeros((n, 4), dtype=torch.float32, device=x.device)
            _lib.check(lib.nerfail_gauss_bwd(_lib.dev(views.wi_batch()), _lib.dev(ori), _lib.dev(x), _lib.dev(gx), _lib.dev(gr),
                                             n, B, P, ctx.eps, _lib.dev(gs), _lib.stream()))
        return gs.reshape(ctx.s_shape), None, None, None, None


def gauss_gather(spatial_rgb, weight_and_index_list, ori_img, epsilon=None, eps_minmax=None, deterministic=True, view_ids=None):
    """Functional form of the hot part: returns (x, x_rgba), differentiable w.r.t. spatial_rgb. `view_ids` (optional):
    stable names of the batch's views (dataset indices) - keys of the per-view inverted indices (see view_indices) and of
    the device-resident maps / images (load_view_maps, register_view)."""
    dev = _cuda()
    if spatial_rgb.dim() < 2 or spatial_rgb.shape[-1] != 4 or spatial_rgb.numel() == 0:
        raise ValueError('spatial_rgb must be [..., 4] (BGRA rows of the point set), got %s' % (tuple(spatial_rgb.shape),))
    if spatial_rgb.device != dev:
        spatial_rgb = spatial_rgb.to(dev)
    views = resolve_views(spatial_rgb, weight_and_index_list, ori_img, view_ids)
    return _GaussGather.apply(spatial_rgb, views, epsilon, eps_minmax, deterministic)


def _stock_classifier_input(x_nhwc, size, contiguous):
    """GN:121-147 in stock PyTorch: NHWC -> NCHW, white background where alpha is 0, then the Resize to `size` (None: none;
    torchvision's if present, as the reference, else the same bilinear op in torch). `contiguous`: copied to packed NCHW
    before the resize (see gauss_net.classifier_input_contiguous)."""
    c = x_nhwc.transpose(2, 3).transpose(1, 2)
    c3 = torch.where(c[:, 3:4] > 0, c[:, :3], torch.full_like(c[:, :3], 255.))
    if contiguous:
        c3 = c3.contiguous()
    return c3 if size is None else resize(c3, size)


class _EpsilonRange:
    """The running [min, max] of x_rgb*alpha (GN:89-103) of gauss_net and gauss_get_r: kept on the device, read lazily."""
    update_epsilon_3d = True
    _eps_minmax = None

    def _mm(self):
        if self._eps_minmax is None:
            self._eps_minmax = torch.zeros(2, dtype=torch.float32, device=_cuda())
        return self._eps_minmax

    @property
    def epsilon_3d_max(self):
        return float(self._mm()[1])

    @property
    def epsilon_3d_min(self):
        return float(self._mm()[0])

    def epsilon_3d_zero(self):
        self._mm().zero_()

    def close_update_epsilon_3d(self):
        self.update_epsilon_3d = False

    def open_update_epsilon_3d(self):
        self.update_epsilon_3d = True

    def print_epsilon(self):
        print("epsilon_3d_min: ", self.epsilon_3d_min)
        print("epsilon_3d_max: ", self.epsilon_3d_max)


class gauss_net(_EpsilonRange, nn.Module):
    """GN:8-159."""

    def __init__(self, device, c, model, model_name, epsilon=None):
        super(gauss_net, self).__init__()
        self.top_number = 8
        self.c = torch.nn.Parameter(torch.tensor([c]), requires_grad=False)
        self.device = device
        self.model = model
        self.model_name = model_name
        self.epsilon = epsilon
        self.deterministic = True    # backward = gather-reduce over a cached inverted index (False: float atomics)
        self.rgb_grad_only = True    # nerfail_s_step: rgb-gradient-only step path (False: full autograd path, four channels)
        self.fused_sign_step = True  # nerfail_s_step on ONE rank: the sign step as the epilogue of the gather backward (round 6)
        # The reference re-runs the classifier on the unperturbed images in EVERY forward (GN:157) although they never
        # change during an attack. None (default, round 6) = automatic: the logits are kept per set of VIEW
        # IDS (view_ids=: stable names of views whose map and image do not change) for as long as the classifier is a pure,
        # frozen function - every module in eval() mode (AS:281-282: model.train(False)), no parameter requiring grad
        # (AS:284-287) - and none of its parameters / buffers was written (their (address, version) pairs are part of the
        # key). True: also per image TENSOR (address, version) and whatever the classifier's mode. False: never.
        self.cache_ori_cla = None
        self._ori_logits = OriLogitCache()
        # The cold tail hands the classifier a NCHW *view* of NHWC data (GN:121-131). MIOpen has no fp32 solver for that
        # layout and falls back to naive_conv_* kernels (17 ms per 8-view forward of the 800x800 victim CNN, 73 % of an
        # attack iteration). True: same values, copied to packed NCHW first (the layout torchvision models are tuned for).
        self.classifier_input_contiguous = True
        # True: a view that is named (view_ids=) and not yet resident is kept on the device after its first upload - the
        # reference-shaped loop (CPU tensors from a DataLoader every iteration) then pays PCIe once per view, not per step
        self.keep_views_resident = False
        # logit_gradients' classifier part. None (default) = automatic: a native MyCNN victim gives the input gradients of all
        # classes in ONE backward pass (MyCNN.input_gradients); every other classifier (timm models, a stock nn.Sequential)
        # takes one autograd.grad per class. False: the per-class loop for MyCNN too. True: as None for MyCNN; for any other
        # classifier one autograd.grad with is_grads_batched=True (legacy vmap: measured slower on the stock 800x800 CNN).
        # Same bits every way. While the batched path is open the last forward's classifier input and raw logits are kept
        # (with their graph, i.e. MyCNN's saved activations) until the next forward.
        self.batched_classifier_backward = None
        self._last_cla_in = self._last_cla = None
        # True (opt-in; not "my_model"): the attacked and the original classifier inputs come from ONE native kernel each
        # (_resize.classifier_input: white background, NCHW and the antialiased resize with fixed-order float32 arithmetic and an
        # exact adjoint without float atomics - stock-victim runs become repeatable bit for bit), and logit_gradients carries all
        # class rows from the resized input to x_rgba in one R = C adjoint call. A shape whose table is refused (more than 16
        # taps) takes the stock path.
        self.native_classifier_input = False
        self._last_native = None     # (classifier input, x_rgba) of the last forward through the native stage

    def forward(self, spatial_rgb, weight_and_index_list, ori_img, zero_init_mask: bool = False, view_ids=None):
        dev = _cuda()
        if spatial_rgb.device != dev:
            spatial_rgb = spatial_rgb.to(dev)
        views = resolve_views(spatial_rgb, weight_and_index_list, ori_img, view_ids, self.keep_views_resident)
        ori_img = views.ori_float()                                      # GN:55
        self._last_views = views                                         # for logit_gradients()
        self._last_ori = ori_img
        x, x_rgba = _GaussGather.apply(spatial_rgb, views, self.epsilon, self._mm() if self.update_epsilon_3d else None,
                                       self.deterministic)
        cla, ori_cla = self.cold_tail(x_rgba, ori_img, views)
        return x, x_rgba, cla, ori_img, ori_cla

    def cold_tail(self, x_rgba, ori_img, views):
        """GN:121-157 (stock PyTorch): NHWC -> NCHW, white background, Resize, the classifier on the perturbed and on the
        original images. `ori_img` may be a callable that yields the float images (evaluated at most once, and only when
        their logits or their identity are needed); `views`: the batch, which keys the original images' logits
        (ori_logit_key: cached by default when the caller names its views, see cache_ori_cla)."""
        size = u2d_classifier_size(self.model_name)
        native = self._native_input_ok(x_rgba, size)
        self._last_native = None
        if native:
            cla_x_3channel = classifier_input(x_rgba, size)
            if cla_x_3channel.requires_grad:
                self._last_native = (cla_x_3channel, x_rgba)             # for logit_gradients()
        else:
            cla_x_3channel = _stock_classifier_input(x_rgba, size, self.classifier_input_contiguous)
        cla = self.model(cla_x_3channel)
        if self._native_batched() and cla.grad_fn is not None:
            self._last_cla_in, self._last_cla = cla_x_3channel, cla      # for logit_gradients()
        else:
            self._last_cla_in = self._last_cla = None
        ori = functools.lru_cache(None)(ori_img if callable(ori_img) else lambda: ori_img)        # evaluated at most once

        def ori_logits():
            o = ori()
            if native and self._native_input_ok(o, size):
                return self.model(classifier_input(o, size))
            return self.model(_stock_classifier_input(o, size, self.classifier_input_contiguous))
        if not (self.cache_ori_cla is True or (self.cache_ori_cla is None and views.view_ids is not None and self._classifier_is_frozen())):
            return cla, ori_logits()
        key, keep = ori_logit_key(views, ori)
        ori_cla = self._ori_logits.get(self._classifier_state_key(), key)
        if ori_cla is None:
            with torch.no_grad():
                ori_cla = ori_logits()
            self._ori_logits.put(key, ori_cla, keep)
        return cla, ori_cla

    def _native_input_ok(self, x, size):
        """The native classifier-input stage takes this tensor: the flag is set, the model is resized for, x is what the kernel
        reads, and neither axis' table is refused (then: the stock path for that shape)."""
        if not self.native_classifier_input or size is None:
            return False
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[3] == 4):
            return False
        try:
            axis_tables(x.shape[1], size, x.device), axis_tables(x.shape[2], size, x.device)
        except _lib.NerfailError:
            return False
        return True

    def _native_batched(self):
        """logit_gradients may take all class gradients from one MyCNN.input_gradients call."""
        from .MyModel import MyCNN
        return self.batched_classifier_backward is not False and isinstance(self.model, MyCNN)

    def _classifier_is_frozen(self):
        """The automatic logit cache's precondition: the classifier is a pure function of its input and nothing is being
        learned through it - every module in eval() mode (no dropout, no batch-norm statistics update) and no parameter
        requiring grad (the reference's attack loops set exactly this up: AS:281-287, attack_NeRFail.py:315-321)."""
        m = self.model
        if not isinstance(m, nn.Module):
            return False
        return not any(x.training for x in m.modules()) and not any(p.requires_grad for p in m.parameters())

    def _classifier_state_key(self):
        m = self.model
        if not isinstance(m, nn.Module):
            return None
        # (a victim's arithmetic, MyCNN.precision, is part of its state: logits cached under one mode are not the other's)
        return tuple((t.data_ptr(), t._version) for t in list(m.parameters()) + list(m.buffers())) + (getattr(m, 'precision', None),)

    def attack_forward(self, spatial_rgb, weight_and_index_list, ori_img, view_ids=None):
        """The forward of one NeRFail-S step (AS:317) without what that step never uses: no `x` tensor (GN:83), no float copy
        of the images unless the original logits have to be computed, alpha + pass mask kept for the rgb-only backward.
        Returns (x_rgba leaf with requires_grad, cla, ori_cla, views, aux); differentiate cla down to x_rgba with autograd,
        then hot_backward_rgb(aux, x_rgba.grad, views)."""
        _, x_rgba, cla, ori_cla, views, aux = self._hot_and_tail(spatial_rgb, weight_and_index_list, ori_img, view_ids, export=False)
        return x_rgba, cla, ori_cla, views, aux

    def export_forward(self, spatial_rgb, weight_and_index_list, ori_img, view_ids=None):
        """The forward of the export epoch (AS:310-317): no gradient, and the unclipped mask image `x` kept for the export.
        Returns (x, x_rgba, cla, ori_cla, views)."""
        with torch.no_grad():
            return self._hot_and_tail(spatial_rgb, weight_and_index_list, ori_img, view_ids, export=True)[:5]

    def _hot_and_tail(self, spatial_rgb, weight_and_index_list, ori_img, view_ids, export):
        """The body of attack_forward (x_rgba a leaf that requires grad, aux, no x) and of export_forward (x, no aux)."""
        dev = _cuda()
        s = spatial_rgb.detach()
        if s.device != dev:
            s = s.to(dev)
        views = resolve_views(s, weight_and_index_list, ori_img, view_ids, self.keep_views_resident)
        x, x_rgba, aux = hot_forward(s, views, self.epsilon, self._mm() if self.update_epsilon_3d else None, need_x=export,
                                     need_aux=not export)
        if not export:
            x_rgba.requires_grad_(True)
        cla, ori_cla = self.cold_tail(x_rgba, views.ori_float, views)
        return x, x_rgba, cla, ori_cla, views, aux

    # ---- all class-logit gradients of one forward in ONE pass over the inverted index (DeepFool)
    def logit_gradients(self, spatial_rgb, weight_and_index_list, x, x_rgba, cla, classes):
        """d cla[0, k] / d spatial_rgb for every k in `classes` (<= 8): tensor [len(classes), *spatial_rgb.shape].

        `x, x_rgba, cla` are what forward() just returned for this spatial_rgb (graph still alive; `cla` may have gone through
        further differentiable ops, as deepfool's bump). The classifier is differentiated down to x_rgba in one pass when it
        is a native MyCNN (MyCNN.input_gradients: one multi-right-hand-side backward, then the cheap elementwise ops of the
        cold tail per class), else by stock PyTorch with one backward per class (see batched_classifier_backward); the
        pixel<->3-D map - the part the reference pays len(classes) scatter passes for - is one nerfail_gauss_bwd_view_multi
        call. Each slice is bitwise what autograd through forward() returns."""
        if cla.shape[0] != 1:
            raise ValueError('logit_gradients differentiates one view at a time (deepfool runs at batch 1, AN:82)')
        classes = [int(k) for k in classes]
        C = len(classes)
        if not 1 <= C <= 8:
            raise ValueError('1..8 classes per call')
        sel = torch.zeros((C, 1, cla.shape[1]), dtype=cla.dtype, device=cla.device)
        sel[torch.arange(C), 0, torch.tensor(classes)] = 1.0
        raw, cla_in = self._last_cla, self._last_cla_in
        if self._native_batched() and raw is not None and _derives_from(cla, raw):
            # native MyCNN: the class rows are taken back to the classifier's own logits (deepfool's `cla + bump`: unchanged),
            # go through the classifier in ONE backward pass, and each is carried on to x_rgba through the cold tail's
            # elementwise ops - the nodes autograd would run per class, on the same values
            d_raw = sel if cla is raw else torch.stack([torch.autograd.grad(cla, raw, grad_outputs=sel[i], retain_graph=True)[0]
                                                        for i in range(C)])
            G = self.model.input_gradients(raw, d_raw)
            J = torch.stack([torch.autograd.grad(cla_in, x_rgba, grad_outputs=G[i], retain_graph=True)[0] for i in range(C)])
        elif self._last_native is not None and self._last_native[1] is x_rgba:
            # stock classifier behind the native input stage: one autograd.grad per class down to the resized input, then all C
            # rows to x_rgba in ONE adjoint call (R = C) - the kernel autograd would run per class, on the same values
            cin = self._last_native[0]
            G = torch.stack([torch.autograd.grad(cla, cin, grad_outputs=sel[i], retain_graph=True)[0] for i in range(C)])
            from . import ops
            J = ops.cls_input_resize_bwd(_lib.f32c(G), x_rgba.detach(), 0, x_rgba.shape[1], x_rgba.shape[2])
        # stock PyTorch / MIOpen: one backward per class. A single batched backward (is_grads_batched=True) is available
        # with self.batched_classifier_backward = True; on the 800x800 stock CNN it measured slower (8.9 vs 7.9 ms for 8
        # classes).
        elif self.batched_classifier_backward is True:
            J = torch.autograd.grad(cla, x_rgba, grad_outputs=sel, retain_graph=True, is_grads_batched=True)[0]
        else:
            J = torch.stack([torch.autograd.grad(cla, x_rgba, grad_outputs=sel[i], retain_graph=True)[0] for i in range(C)])
        views = self._last_views
        B, P = views.B, views.P
        n = spatial_rgb.numel() // 4
        vi = views.indices()[0]                                                 # one view (batch 1): its per-view index
        J = _lib.f32c(J).reshape(C, B * P, 4)
        ori = _lib.f32c(self._last_ori)
        out = torch.empty((C, n, 4), dtype=torch.float32, device=J.device)
        lib = _lib.load()
        st = _lib.ViewIndexStruct()
        vi.fill(st)
        scratch = torch.empty((lib.nerfail_gauss_bwd_views_scratch_floats(ctypes.byref(st), 1, P, C),), dtype=torch.float32, device=J.device)
        eps = -1.0 if self.epsilon is None else float(self.epsilon)
        x_c = _lib.f32c(x)            # bound to a name: see deepfool.py on pointers of temporaries
        _lib.check(lib.nerfail_gauss_bwd_view_multi(_lib.dev(ori), _lib.dev(x_c), _lib.dev(J), C, ctypes.byref(st), n, P, eps,
                                                    _lib.dev(scratch), _lib.dev(out), _lib.stream()))
        return out.reshape((C,) + tuple(spatial_rgb.shape))


def u2d_classifier_size(model_name):
    """Side length the 2-D baselines resize the classifier input to (GN:372-380), or None for "my_model": the reference's else
    branch resizes to 299, at which MyCNN cannot run (its seventh stage needs 4 x 4); gauss_net (GN:147) and model_test
    (MT:195-196) leave my_model at full size, and so does this package - the ONE deviation from GN:340-385."""
    return None if model_name == "my_model" else (224 if model_name == "vit_b_16" else 299)


def u2d_resize(x, model_name):
    """GN:372-380 on an NCHW batch. No call when the image already has the target size (torchvision returns it unchanged)."""
    size = u2d_classifier_size(model_name)
    if size is None or (x.shape[-2] == size and x.shape[-1] == size):
        return x
    return resize(x, size)


class universal_2D_net(nn.Module):
    """GN:340-385, the net of the 2-D baselines, in stock torch ops: differentiable with respect to `r` on any device.
    forward(r, ori_img) -> (r, x_rgb, cla, ori_img, ori_cla) with x_rgb = clip(ori_img + r, 0, 255); `r` is per view
    [B,H,W,3] or one shared plane [H,W,3] (GN:359-363). The resize rule: u2d_classifier_size / u2d_resize. The classifier sees
    a contiguous NCHW tensor (the same values as the reference's transposed view). attack.igsm_2d computes the same x_rgb and
    classifier input with one launch from a resident uint8 store (nerfail_u2d_fwd), bit for bit."""

    def __init__(self, device, c, model, model_name):
        super(universal_2D_net, self).__init__()
        self.top_number = 8
        self.c = torch.nn.Parameter(torch.tensor([c]), requires_grad=False)
        self.device = device
        self.model = model
        self.model_name = model_name
        self.theta = torch.tensor([[1, 0, 0], [0, 1, 0]], dtype=torch.float, device=device)

    def forward(self, r, ori_img):
        ori_img = torch.as_tensor(ori_img).detach().to(torch.float)       # GN:357
        if r.size() != ori_img.size():
            x_rgb = ori_img + r.unsqueeze(0).broadcast_to(ori_img.size())   # GN:359-363
        else:
            x_rgb = ori_img + r
        x_rgb = torch.clip(x_rgb, min=0, max=255)
        cla_x = x_rgb.transpose(2, 3).transpose(1, 2).contiguous()
        cla_ori_img = ori_img.transpose(2, 3).transpose(1, 2).contiguous()
        cla = self.model(u2d_resize(cla_x, self.model_name))
        ori_cla = self.model(u2d_resize(cla_ori_img, self.model_name))
        return r, x_rgb, cla, ori_img, ori_cla


def _derives_from(t, src, depth=4):
    """`t` is `src` or was computed from it by at most `depth` autograd nodes."""
    want, level = src.grad_fn, [t.grad_fn]
    for _ in range(depth + 1):
        if any(n is want for n in level):
            return want is not None
        level = [m for n in level if n is not None for m, _ in n.next_functions]
    return False


class _Compose(torch.autograd.Function):
    """x_rgba = compose(ori, r) of gauss_get_img (GN:309-319) on nerfail_gauss_compose; the gradient w.r.t. r is the plain chain
    rule of those three lines (elementwise, cold: nobody differentiates this in the reference's scripts)."""

    @staticmethod
    def forward(ctx, ori, r):
        out = torch.empty_like(r)
        _lib.check(_lib.load().nerfail_gauss_compose(_lib.dev(ori, 'ori_img'), _lib.dev(r, 'r'), r.numel() // 4, _lib.dev(out), _lib.stream()))
        ctx.save_for_backward(ori, r)
        return out

    @staticmethod
    def backward(ctx, g):
        ori, r = ctx.saved_tensors
        opaque = (ori[..., 3:4] > 0).to(g.dtype)
        g_rgb = g[..., :3] * opaque
        g_r = torch.cat([g_rgb * (r[..., 3:4] / 255), (g_rgb * r[..., :3]).sum(-1, keepdim=True) / 255], -1)
        return None, g_r


class gauss_get_r(_EpsilonRange, nn.Module):
    """GN:189-268: the perturbation gathered onto the pixels of a batch of views straight from RAW distances,
    r = sum_k s[idx_k] g_k / (sum g + 0.001), g = exp(-(d/c)^2 / 2). Composition of K9 (nerfail_gauss_weight) and K10's gather
    (nerfail_gauss_fwd: its `x` output), differentiable w.r.t. spatial_rgb like the reference's."""

    def __init__(self, device, c, model, model_name):
        super(gauss_get_r, self).__init__()
        self.top_number = 8
        self.c = torch.nn.Parameter(torch.tensor([c]), requires_grad=False)
        self.device = device
        self.model = model
        self.model_name = model_name
        self.w = 299
        self.h = 299

    def forward(self, spatial_rgb, dist_and_index_list):
        dev = _cuda()
        dai = _lib.f32c(dist_and_index_list, dev)
        if dai.dim() != 5 or dai.shape[1] != 2 or dai.shape[4] != 8:
            raise ValueError('dist_and_index_list must be [B,2,H,W,8] (CI:148-163)')
        if not float(self.c) > 0:
            raise _lib.NerfailError('gauss_get_r: c must be positive')
        wi = torch.ops.nerfail_mi.gauss_weight(dai, float(self.c))                         # K9
        ori0 = torch.zeros((dai.shape[0], dai.shape[2], dai.shape[3], 4), dtype=torch.float32, device=dev)   # r does not depend on the image
        x, _ = gauss_gather(spatial_rgb, wi, ori0, None, self._mm() if self.update_epsilon_3d else None, True)
        return x


class gauss_get_img(nn.Module):
    """GN:271-337: composite an already gathered r onto the images and classify. Hot part = nerfail_gauss_compose (no epsilon
    clip, no [0,255] clip - GN:309-319); the tail (NHWC -> NCHW, white background, Resize to 299 / 224 - here ALSO for
    "my_model", GN:339-347 - and the two classifier passes) is stock PyTorch like gauss_net's."""

    def __init__(self, device, c, model, model_name):
        super(gauss_get_img, self).__init__()
        self.top_number = 8
        self.c = torch.nn.Parameter(torch.tensor([c]), requires_grad=False)
        self.device = device
        self.model = model
        self.model_name = model_name
        self.w = 299
        self.h = 299

    def compose(self, ori_img, r):
        """(ori_img float [B,H,W,4], x_rgba): the part before the classifier."""
        dev = _cuda()
        ori = _lib.f32c(torch.as_tensor(ori_img), dev)                                     # GN:290
        r_ = r if (isinstance(r, torch.Tensor) and r.is_cuda and r.dtype == torch.float32 and r.is_contiguous()) else _lib.f32c(torch.as_tensor(r), dev)
        if ori.dim() != 4 or ori.shape[-1] != 4 or tuple(r_.shape) != tuple(ori.shape):
            raise ValueError('ori_img and r must both be [B,H,W,4], got %s and %s' % (tuple(ori.shape), tuple(r_.shape)))
        return ori, _Compose.apply(ori, r_)

    def forward(self, ori_img, r):
        ori, x_rgba = self.compose(ori_img, r)
        size = 224 if self.model_name == "vit_b_16" else 299              # (its own size rule: 299 for "my_model" too)
        cla = self.model(_stock_classifier_input(x_rgba, size, True))
        ori_cla = self.model(_stock_classifier_input(ori, size, True))
        return r, x_rgba, cla, ori, ori_cla


class create_gauss_w(nn.Module):
    """GN:161-186: distances -> normalised Gaussian weights; returns (cat([w, idx], 1), dist)."""

    def __init__(self, device, c):
        super(create_gauss_w, self).__init__()
        self.top_number = 8
        self.device = device
        self.c = c

    def forward(self, dist_and_index_list):
        dai = _lib.f32c(dist_and_index_list, _cuda())
        if dai.dim() != 5 or dai.shape[1] != 2 or dai.shape[4] != 8:
            raise ValueError('dist_and_index_list must be [B,2,H,W,8] (CI:148-163)')
        if not float(self.c) > 0:
            raise _lib.NerfailError('create_gauss_w: c must be positive')
        return torch.ops.nerfail_mi.gauss_weight(dai, float(self.c)), dai[:, 0:1]          # K9 as a registered op
