"""MI355X mirror of deepfool.py (reference root, `deepfool(...)` lines 10-111): the per-view inner loop of NeRFail
(attack_NeRFail.py:396-402). Same signature and 5-tuple return (rot, loop_i, ori_cla_max_index, cla_max_index,
spatial_rgb).

The control flow (margins m1 / m2, per-class minimal step, accumulation, clamp, alpha restore) is host logic and
stays Python, as SURVEY.md section 2 #10 scopes it; every forward / backward through the pixel<->3-D map runs in the
HIP kernels behind `net` (gauss_net: K10 forward, K11 backward). Two savings over the reference that cannot change
the result: the gradient of the original class logit is computed once per iteration instead of once per competing
class (the reference recomputes the identical tensor up to 7 times at deepfool.py:76-77), and when `net` is
nerfail_amd's gauss_net all class gradients of an iteration come from ONE multi-right-hand-side pass over the
inverted index (gauss_net.logit_gradients -> nerfail_gauss_bwd_csr_multi) instead of one autograd.grad call each; the
competing class is then chosen on the device (first minimum, NaN never chosen: deepfool.py:85's strict `<`).

`deepfool_native` is the same loop in product shape for this package's gauss_net: the break test and the margins in one launch
(nerfail_deepfool_gate), one 8-byte host read per iteration, norms + choice + update in one call (nerfail_deepfool_step), every
buffer allocated once per call, and the class chosen in every iteration reported. `deepfool` stays exactly as it is.

`deepfool(universal_2d=True)` keeps raising NotImplementedError (tests/test_hip_errors.py pins it): the 2-D baseline's DeepFool
(attack_UAP_2D.py:306-312) is `deepfool_2d`, the same loop on the ONE image-plane table through universal_2D_net without the
alpha restore, and `deepfool_2d_native`, its product shape around nerfail_uap2d_step (csrc/uap2d.hip).
"""
import torch

from . import _lib


def _grad(out_scalar, wrt):
    return torch.autograd.grad(out_scalar, wrt, retain_graph=True, create_graph=False)[0]


def _bump_and_test(cla, o, target_label, m1):
    """deepfool.py:53-66: +m1 on the clean class (targeted: on every class but the target), out of place, the first maximum and
    the break test. Returns (bumped logits, their argmax, done). Stock torch, any device."""
    bump = torch.zeros_like(cla)
    if target_label is None:
        bump[:, o] = m1
    else:
        bump[:, :int(target_label)] = m1
        bump[:, int(target_label) + 1:] = m1
    cla = cla + bump
    cla_max_index = torch.max(cla, 1)[1]
    done = int(cla_max_index) != o if target_label is None else int(cla_max_index) == int(target_label)
    return cla, cla_max_index, done


def _competitors(o, num_classes, target_label):
    """deepfool.py:68-72: the classes an iteration steps towards."""
    return [k for k in range(num_classes) if k != o] if target_label is None else [int(target_label)]


def _choose(cla, o, ks, m2, nrm, target_label):
    """deepfool.py:79-96 once the norms `nrm` of grad_k - grad_o are known: (index into ks of the class chosen, the step's scale).
    Untargeted the first minimum of |f'| / (norm + 1e-4) - the reference's strict `<` scan; a NaN is never chosen, and when
    nothing can be chosen the scale is 0. Stock torch, any device."""
    f_prime = (cla[0, ks] - (cla[0, o] + m2)).detach()                                  # deepfool.py:79
    if target_label is not None:
        return torch.zeros((), dtype=torch.int64, device=nrm.device), torch.abs(f_prime[0]) / ((nrm[0] ** 2) + 0.0001)   # :92-96
    value_r = torch.abs(f_prime) / (nrm + 0.0001)                                       # deepfool.py:81
    value_r = torch.where(torch.isnan(value_r), torch.full_like(value_r, float('inf')), value_r)
    best = torch.argmin(value_r)
    scale = torch.abs(f_prime[best]) / ((nrm[best] ** 2) + 0.0001)                      # deepfool.py:86
    return best, torch.where(torch.isinf(value_r[best]), torch.zeros_like(scale), scale)


def deepfool(net_input, e, net, num_classes=8, max_iter=20, target_label: int = None, overshoot: float = 0.02,
             m1: float = 1, m2: float = 30, universal_2d=False):
    if universal_2d:
        raise NotImplementedError('universal_2d is the 2-D baseline (attack_UAP_2D.py): out of scope, SURVEY.md section 2 #12')
    spatial_rgb, weight_and_index, ori_img = net_input
    if torch.cuda.is_available():          # the reference keeps everything on `device` (AN:354-362); CPU tensors are uploaded once
        dev = torch.device('cuda', torch.cuda.current_device())
        spatial_rgb = _lib.f32c(torch.as_tensor(spatial_rgb), dev)
        weight_and_index = _lib.f32c(torch.as_tensor(weight_and_index), dev)
        ori_img = _lib.f32c(torch.as_tensor(ori_img), dev)
    spatial_rgb_0 = spatial_rgb.clone().detach()
    spatial_rgb = spatial_rgb.detach().clone().requires_grad_(True)

    _, _, cla, _, ori_cla = net(spatial_rgb, weight_and_index, ori_img)                 # deepfool.py:33
    cla_max_index = torch.max(cla, 1)[1]
    ori_cla_max_index = torch.max(ori_cla, 1)[1]
    rot = torch.zeros_like(spatial_rgb_0)

    loop_i = 0
    while loop_i < max_iter:
        spatial_rgb = spatial_rgb.detach().clone().requires_grad_(True)
        x_out, x_rgba, cla, _, ori_cla = net(spatial_rgb, weight_and_index, ori_img)     # deepfool.py:51
        ori_cla_max_index = torch.max(ori_cla, 1)[1]
        o = int(ori_cla_max_index)
        cla, cla_max_index, done = _bump_and_test(cla, o, target_label, m1)
        if done:
            break

        ks = _competitors(o, num_classes, target_label)
        # the multi-RHS pass takes 2..8 logits ([o] + ks): with o >= num_classes all num_classes competitors remain (9 at
        # num_classes = 8), with a single class none does - those cases iterate class by class like the reference
        multi = hasattr(net, 'logit_gradients') and getattr(net, 'deterministic', False) and 2 <= len(ks) + 1 <= 8
        if multi:
            # all class gradients in one pass over the inverted index (K11 multi-RHS), then the step arithmetic in two
            # streaming kernels (K14): ||G_k - G_o||^2 for every k, device-side choice, rot / clamp / alpha restore
            G = net.logit_gradients(spatial_rgb, None, x_out, x_rgba, cla, [o] + ks)
            lib = _lib.load()
            C, n = G.shape[0], G[0].numel() // 4
            nb = lib.nerfail_deepfool_norms_scratch_bytes(C, n)
            scratch = torch.empty((nb,), dtype=torch.uint8, device=G.device)
            norms2 = torch.empty((C - 1,), dtype=torch.float32, device=G.device)
            _lib.check(lib.nerfail_deepfool_norms(_lib.dev(G), C, n, _lib.dev(scratch), nb, _lib.dev(norms2), _lib.stream()))
            nrm = torch.sqrt(norms2)                                                    # torch.norm(grad_prime), every k
        else:
            grad_o = _grad(cla[:, o].sum(), spatial_rgb)
            grads_k = torch.stack([_grad(cla[:, k].sum(), spatial_rgb) for k in ks])
            grad_prime = grads_k - grad_o.unsqueeze(0)                                  # deepfool.py:78 for every k
            nrm = torch.linalg.vector_norm(grad_prime.reshape(len(ks), -1), dim=1)
        best, scale = _choose(cla, o, ks, m2, nrm, target_label)
        if multi:
            rot = _lib.f32c(rot)
            new_s = torch.empty_like(spatial_rgb_0)
            # the device scalars are bound to names: a temporary freed right after its pointer was taken could be handed
            # to the next allocation and overwritten before the kernel (enqueued afterwards) reads it
            best_i, scale_f, s0_c = (best + 1).to(torch.int32), scale.to(torch.float32).reshape(1), _lib.f32c(spatial_rgb_0)
            _lib.check(lib.nerfail_deepfool_apply(_lib.dev(G), C, n, _lib.dev(best_i), _lib.dev(scale_f), float(overshoot),
                                                  _lib.dev(s0_c), _lib.dev(rot), _lib.dev(new_s), _lib.stream()))
            spatial_rgb = new_s                                                         # deepfool.py:98-102 fused
        else:
            rot = (rot + scale * grad_prime[best]).detach()
            spatial_rgb = torch.clamp((spatial_rgb_0 + (overshoot * rot)).detach(), -255, 255)
            spatial_rgb = torch.cat([spatial_rgb[:, :, :, :3], spatial_rgb_0[:, :, :, 3].unsqueeze(-1)], -1)   # alpha unchanged
        loop_i += 1

    spatial_rgb = spatial_rgb.detach()
    rot = (spatial_rgb - spatial_rgb_0).detach()
    return rot, loop_i, ori_cla_max_index, cla_max_index, spatial_rgb


def _target_word(target_label, C):
    """The gate's target word: -1 untargeted, else the class; None when it names none of the C classes (the call falls through)."""
    target = -1 if target_label is None else int(target_label)
    return target if -1 <= target < C else None


class _NativeCall:
    """What deepfool_native and deepfool_2d_native allocate once per call and do alike: the gradient rows [o] + competitors,
    record / trace / rot / out, the gate with the iteration's one host read, the six-value result. `r_0`: the table the call
    started from (a device copy of its own); `o`: the clean argmax; `target`: _target_word's."""

    def __init__(self, r_0, C, o, target, max_iter):
        self.lib = _lib.load()
        self.r_0, self.C, self.o, self.target = r_0, C, o, target
        self.rows = [o] + _competitors(o, C, None if target < 0 else target)
        self.record = torch.zeros((_lib.DEEPFOOL_RECORD_WORDS,), dtype=torch.int32, device=r_0.device)
        self.trace = torch.full((max(int(max_iter), 1),), -1, dtype=torch.int32, device=r_0.device)
        self.rot = torch.zeros_like(r_0)
        self.out = torch.empty_like(r_0)
        self.loop_i, self.arg = 0, None

    def gate(self, cla, m1, m2):
        """nerfail_deepfool_gate on this iteration's logits, then the iteration's one host read: done?"""
        cla_c = _lib.f32c(cla)
        _lib.check(self.lib.nerfail_deepfool_gate(_lib.dev(cla_c), self.C, self.o, self.target, float(m1), float(m2), _lib.dev(self.record),
                                                  _lib.stream()))
        done, self.arg = self.record[:2].tolist()
        return done

    def trace_slot(self):
        return self.trace[self.loop_i:self.loop_i + 1]

    def result(self, ori_cla_max_index, cla):
        """`cla`: the logits whose argmax is reported when no gate ran (max_iter < 1)."""
        cla_max_index = torch.max(cla, 1)[1] if self.arg is None else torch.full((1,), self.arg, dtype=torch.int64, device=self.r_0.device)
        r = self.out if self.loop_i > 0 else self.r_0.clone()
        classes = self.trace[:self.loop_i].tolist() if self.loop_i > 0 else []
        return (r - self.r_0).detach(), self.loop_i, ori_cla_max_index, cla_max_index, r.detach(), classes


def _native_applies(net, num_classes, universal_2d):
    from .GaussNet import gauss_net
    return (not universal_2d and isinstance(net, gauss_net) and getattr(net, 'deterministic', False)
            and 2 <= int(num_classes) <= _lib.DEEPFOOL_MAX_COMPETITORS and torch.cuda.is_available())


def deepfool_native(net_input, e, net, num_classes=8, max_iter=20, target_label: int = None, overshoot: float = 0.02,
                    m1: float = 1, m2: float = 30, universal_2d=False, view_ids=None):
    """deepfool(...) with the step arithmetic of an iteration in two library calls and nothing of torch between them:
    nerfail_deepfool_gate (bump, first maximum, break test, |f'| of every competitor: deepfool.py:53-66, :79 / :93) and
    nerfail_deepfool_step (norms, choice of the class, rot, clamp, alpha restore: deepfool.py:68-105).

    Same arguments as deepfool plus `view_ids` (the view's name, handed to net: its cached inverted index and clean logits).
    Returns SIX values: deepfool's (rot, loop_i, ori_cla_max_index, cla_max_index, spatial_rgb) and, sixth, the list of the
    class chosen in each of the loop_i iterations (None when the call fell through). An iteration in which no class could be
    chosen - every value_r NaN or infinite - still counts as one of the loop_i steps, as in the mirror: its entry is -1 and rot
    is left as it was.

    For `net` = this package's gauss_net on its deterministic path and 2..8 classes (2..8 gradient rows). Everything else -
    another net, other class counts, a classifier whose row is not num_classes wide, universal_2d - falls through to
    deepfool(...). The clean argmax `o` is read once per call (the clean image does not change during a call); per iteration:
    net(...), gate, ONE host read of the record's first two words, net.logit_gradients, step. The first iteration uses the
    forward of deepfool.py:33 instead of repeating it on the same table. Record, scratch, rot, the output table and the trace
    array are allocated once per call."""
    def mirror():
        inp = net_input
        if view_ids is not None and not universal_2d and (inp[1] is None or inp[2] is None):
            with torch.no_grad():                                                           # a resident view: the mirror takes tensors
                net(inp[0], inp[1], inp[2], view_ids=view_ids)
            inp = (inp[0], net._last_views.wi_batch(), net._last_ori)
        return deepfool(inp, e, net, num_classes, max_iter, target_label, overshoot, m1, m2, universal_2d) + (None,)
    if not _native_applies(net, num_classes, universal_2d):
        return mirror()
    spatial_rgb, weight_and_index, ori_img = net_input
    dev = torch.device('cuda', torch.cuda.current_device())
    spatial_rgb_0 = _lib.f32c(torch.as_tensor(spatial_rgb), dev).clone()
    if view_ids is None:
        weight_and_index = _lib.f32c(torch.as_tensor(weight_and_index), dev)
        ori_img = _lib.f32c(torch.as_tensor(ori_img), dev)
    fwd = (lambda s: net(s, weight_and_index, ori_img, view_ids=view_ids)) if view_ids is not None else \
          (lambda s: net(s, weight_and_index, ori_img))
    s = spatial_rgb_0.clone().requires_grad_(True)
    x_out, x_rgba, cla, _, ori_cla = fwd(s)                                             # deepfool.py:33
    C = int(cla.shape[1])
    target = _target_word(target_label, C)
    if cla.shape[0] != 1 or C != int(num_classes) or target is None:
        return mirror()
    ori_cla_max_index = torch.max(ori_cla, 1)[1]
    call = _NativeCall(spatial_rgb_0, C, int(ori_cla_max_index), target, max_iter)     # THE read of the call
    n_rhs, n = len(call.rows), spatial_rgb_0.numel() // 4
    nb = call.lib.nerfail_deepfool_step_scratch_bytes(n_rhs, n)
    scratch = torch.empty((nb // 8,), dtype=torch.float64, device=dev)
    while call.loop_i < max_iter:
        if call.loop_i > 0:
            s = call.out.detach().requires_grad_(True)
            x_out, x_rgba, cla, _, ori_cla = fwd(s)                                     # deepfool.py:51
        if call.gate(cla, m1, m2):
            break
        G = net.logit_gradients(s, None, x_out, x_rgba, cla, call.rows)
        _lib.check(call.lib.nerfail_deepfool_step(_lib.dev(G), n_rhs, n, _lib.dev(call.record), _lib.c_p(scratch.data_ptr()), nb,
                                                  float(overshoot), _lib.dev(spatial_rgb_0), _lib.dev(call.rot), _lib.dev(call.out),
                                                  _lib.dev(call.trace_slot()), _lib.stream()))
        call.loop_i += 1
    return call.result(ori_cla_max_index, cla)


# ---------------------------------------------------------------------------------------------- the 2-D baseline's DeepFool (universal_2d)
def deepfool_2d(net_input, e, net, num_classes=8, max_iter=20, target_label: int = None, overshoot: float = 0.02,
                m1: float = 1, m2: float = 30):
    """deepfool.py:10-111 with universal_2d=True (the inner loop of attack_UAP_2D.py:306-312), in stock torch through
    GaussNet.universal_2D_net: the replacement of `deepfool(universal_2d=True)`, which keeps raising. `net_input` =
    (table [H,W,3] - the ONE plane every view shares -, ori_img [1,H,W,3]); the same 5-tuple return (dr, loop_i,
    ori_cla_max_index, cla_max_index, table after the last step). Any device, the CPU included; the table's dtype is kept.

    The control flow is `deepfool`'s without the alpha restore (deepfool.py:104): the clamp to +-255 acts on all three channels.
    As there, the clean class's gradient is computed once per iteration instead of once per competitor."""
    table, ori_img = net_input
    table = torch.as_tensor(table)
    r_0 = table.clone().detach()
    r = table.detach().clone().requires_grad_(True)
    _, _, cla, _, ori_cla = net(r, ori_img)                                             # deepfool.py:31
    cla_max_index = torch.max(cla, 1)[1]
    ori_cla_max_index = torch.max(ori_cla, 1)[1]
    rot = torch.zeros_like(r_0)
    loop_i = 0
    while loop_i < max_iter:
        r = r.detach().clone().requires_grad_(True)
        _, _, cla, _, ori_cla = net(r, ori_img)                                         # deepfool.py:49
        ori_cla_max_index = torch.max(ori_cla, 1)[1]
        o = int(ori_cla_max_index)
        cla, cla_max_index, done = _bump_and_test(cla, o, target_label, m1)
        if done:
            break
        ks = _competitors(o, num_classes, target_label)
        grad_o = _grad(cla[:, o].sum(), r)
        grad_prime = torch.stack([_grad(cla[:, k].sum(), r) for k in ks]) - grad_o.unsqueeze(0)   # deepfool.py:80 for every k
        nrm = torch.linalg.vector_norm(grad_prime.reshape(len(ks), -1), dim=1)
        best, scale = _choose(cla, o, ks, m2, nrm, target_label)
        rot = (rot + scale * grad_prime[best]).detach()
        r = torch.clamp((r_0 + (overshoot * rot)).detach(), -255, 255)                  # deepfool.py:100-101, all three channels
        loop_i += 1
    r = r.detach()
    return (r - r_0).detach(), loop_i, ori_cla_max_index, cla_max_index, r


def _native_2d_applies(net, num_classes):
    from .GaussNet import universal_2D_net
    return (isinstance(net, universal_2D_net) and 2 <= int(num_classes) <= _lib.DEEPFOOL_MAX_COMPETITORS and torch.cuda.is_available())


def deepfool_2d_native(net_input, e, net, num_classes=8, max_iter=20, target_label: int = None, overshoot: float = 0.02,
                       m1: float = 1, m2: float = 30, images=None, view=None, clean_logits=None):
    """deepfool_2d(...) in product shape: per iteration ops.u2d_fwd on the shared plane (the classifier's planar input and the
    clip's pass mask in one launch), the classifier on the attacked image only, nerfail_deepfool_gate, ONE host read of the
    record's first two words, the class gradients with respect to the classifier input, and nerfail_uap2d_step (norms through
    the pass mask, the choice, rot, the +-255 clamp: three launches). The clean logits do not change during a call: the clean
    argmax `o` is read once.

    Same arguments as deepfool_2d plus `images` / `view`: a resident uint8 store [N,H,W,4|3] and the view's index in it (`view` may
    be left out for a one-view store; an index outside the store is a ValueError) (else
    ori_img, which then must hold whole numbers in 0..255, is taken as a one-view store), and `clean_logits` [1,C] of that view
    (else the classifier runs once on the clean image). Class gradients: with this package's MyCNN under model_name "my_model",
    MyCNN.forward_masks (ops.cnn_fwd with its pool masks, or its bf16x3 form when the victim's precision says so) and ONE
    MyCNN.backward_data (ops.cnn_bwd_data_multi[_x3]) over the one-hot rows [o] + ks; with any other classifier
    one autograd.grad per row with respect to the classifier input, stacked. Record, scratch, rot, the one-hot rows and the
    trace array are allocated once per call.

    Returns SIX values: deepfool_2d's five and the list of the class chosen in each of the loop_i iterations (-1 where nothing
    could be chosen). What the native path does not cover - a net that is not universal_2D_net, classes outside 2..8, a
    classifier row that is not num_classes wide, a batch of more than one view, no GPU - falls through to deepfool_2d and
    returns None as the sixth value."""
    from . import ops
    from .GaussNet import u2d_resize
    from .MyModel import MyCNN
    table, ori_img = net_input
    if images is not None:
        if view is None:
            if images.shape[0] != 1:
                raise ValueError('deepfool_2d_native: `images` holds %d views: `view` must name one' % images.shape[0])
            view = 0
        if not 0 <= int(view) < images.shape[0]:
            raise ValueError('deepfool_2d_native: view %d is outside the store (0..%d)' % (int(view), images.shape[0] - 1))
    elif ori_img is None:
        raise ValueError('deepfool_2d_native: net_input holds no image and no store was given')

    def mirror():
        ori = ori_img
        if ori is None:                                                                 # a resident view: the mirror takes a tensor
            with torch.no_grad():
                r = torch.as_tensor(table).to(images.device)
                ori, _, _ = ops.u2d_fwd(images, torch.full((1,), int(view), dtype=torch.int64, device=images.device),
                                        torch.zeros_like(r, dtype=torch.float32), True, False, False)
        return deepfool_2d((table, ori), e, net, num_classes, max_iter, target_label, overshoot, m1, m2) + (None,)
    if not _native_2d_applies(net, num_classes):
        return mirror()
    dev = torch.device('cuda', torch.cuda.current_device())
    if images is None:
        ori = torch.as_tensor(ori_img).to(dev)
        store = ori.to(torch.uint8).contiguous()
        if ori.dim() != 4 or ori.shape[0] != 1 or ori.shape[-1] != 3 or not bool((store == ori).all()):
            return mirror()
        view = 0
    else:
        store = images
    C = int(num_classes)
    target = _target_word(target_label, C)
    if target is None:
        return mirror()
    model, name = net.model, net.model_name
    cnn = isinstance(model, MyCNN) and name == "my_model"
    r_0 = _lib.f32c(torch.as_tensor(table), dev).clone()
    hw = tuple(r_0.shape[:-1])
    P = r_0.numel() // 3
    idx = torch.full((1,), int(view), dtype=torch.int64, device=dev)
    if clean_logits is None:
        with torch.no_grad():
            _, clean_in, _ = ops.u2d_fwd(store, idx, torch.zeros_like(r_0), False, True, False)
            clean_logits = model(u2d_resize(clean_in, name))
    if clean_logits.dim() != 2 or clean_logits.shape[0] != 1 or clean_logits.shape[1] != C:
        return mirror()
    ori_cla_max_index = torch.max(clean_logits, 1)[1]
    call = _NativeCall(r_0, C, int(ori_cla_max_index), target, max_iter)               # THE read of the call
    rows = call.rows
    scratch, _ = ops.uap2d_step_scratch(len(rows), P, dev)
    onehot = torch.zeros((len(rows), 1, C), dtype=torch.float32, device=dev)
    onehot[torch.arange(len(rows), device=dev), 0, torch.tensor(rows, device=dev)] = 1.
    cur, cla = r_0, None
    while call.loop_i < max_iter:
        with torch.no_grad():
            _, cls_in, mask = ops.u2d_fwd(store, idx, cur, False, True, True)           # deepfool.py:49 up to the classifier
        if cnn:
            cla, ws, pool = model.forward_masks(cls_in)
        else:
            cls_in.requires_grad_()
            cla = model(u2d_resize(cls_in, name))
            if cla.dim() != 2 or cla.shape[0] != 1 or cla.shape[1] != C:
                return mirror()
        if call.gate(cla, m1, m2):
            break
        if cnn:
            G = model.backward_data(ws, pool, onehot, hw[0], hw[1])
        else:
            G = _lib.f32c(torch.stack([torch.autograd.grad(cla[0, k], cls_in, retain_graph=True)[0] for k in rows]))
        ops.uap2d_step(G, mask.view(-1), call.record, scratch, overshoot, r_0, call.rot, call.out, call.trace_slot())
        cur = call.out
        call.loop_i += 1
    if call.arg is None:                                                                # max_iter < 1: deepfool.py:31's forward alone
        with torch.no_grad():
            _, cls_in, _ = ops.u2d_fwd(store, idx, cur, False, True, False)
            cla = model(u2d_resize(cls_in, name))
    return call.result(ori_cla_max_index, cla)
