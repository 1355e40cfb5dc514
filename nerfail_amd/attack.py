"""The attack-step arithmetic of attack_NeRFail_S.py (reference = AS), on the MI355X.

`igsm_step` is AS:352-392 as one kernel. One iteration of the AS:304-392 loop body is written once, as `_rgb_step`: `_share`
takes the batch apart (view ids, size, this rank's views), `_forward_backward` runs gauss_net's forward, the optional epoch
statistics, the CE loss (+ the beta term) and the classifier backward, and the step ends in the fused gather backward + sign
step (one rank) or in the 3 Ns + 1 float buffer - rgb gradient, loss in the tail - that ONE all-reduce sums over the ranks
(RCCL over xGMI on the GPU box, gloo in the CPU tests) before every rank applies the identical step: the only collective on
the whole path. `nerfail_s_step` is that body; `nerfail_s`, the whole AS:278-442 loop as a product
(epoch statistics, best tensor and export epoch, decided on the device, csrc/attack_stats.hip), calls it with its statistics
and beta and adds one all-reduce of a 16-float statistics row per EPOCH. perturbation_grad, the four-channel autograd path,
stays apart: it is what the rgb path is compared against.
"""
import torch

from . import _lib
from . import ops  # noqa: F401  (registers torch.ops.nerfail_mi.*)
from . import sharding
from .run_nerf_helpers import _cuda


def igsm_step(spatial, grad, spatial_init, a=2.0, epsilon=32.0, targeted=False, out=None):
    """AS:352-392: rgb <- rgb -/+ a*sign(grad) where alpha > 0 else 0; clamp to init +- epsilon; alpha kept."""
    dev = _cuda()
    s = _lib.f32c(spatial, dev)
    g = _lib.f32c(grad, dev)
    s0 = _lib.f32c(spatial_init, dev)
    if s.shape[-1] != 4 or g.shape != s.shape or s0.shape != s.shape:
        raise ValueError('spatial, grad and spatial_init must all be [..., 4] of the same shape')
    res = torch.ops.nerfail_mi.igsm_step(s, g, s0, float(a), float(epsilon), bool(targeted))     # K12 as a registered op
    if out is not None:
        out.copy_(res)
        return out
    return res


def perturbation_grad(net, spatial, weight_and_index, ori_img, label, batch_total=None, grad_fn=None, view_ids=None):
    """d(CE(cla, label))/d(spatial) for the views given (AS:317-348). `batch_total` = views in the WHOLE batch
    (CE is a mean over the batch, so a shard holding k of B views contributes with weight k/B). `view_ids`: the views'
    dataset indices - keys of their cached / persisted inverted indices (GaussNet.view_indices, load_view_indices)."""
    s = spatial.detach().clone().requires_grad_(True)
    if view_ids is not None:
        x, r, cla, ori, ori_cla = net(s, weight_and_index, ori_img, view_ids=view_ids)
    else:
        x, r, cla, ori, ori_cla = net(s, weight_and_index, ori_img)
    lab = label.to(cla.device).broadcast_to([cla.shape[0]])
    if grad_fn is not None:
        loss = grad_fn(cla, lab)
    else:
        loss = torch.nn.functional.cross_entropy(cla, lab, reduction='sum') / float(batch_total or cla.shape[0])
    loss.backward()
    return s.grad, loss.detach(), cla.detach()


def igsm_step_rgb(spatial, grad_rgb, spatial_init, a=2.0, epsilon=32.0, targeted=False):
    """AS:352-392 with the gradient as [Ns,3] (rgb only; the alpha channel's gradient is never read by the sign step)."""
    dev = _cuda()
    s, s0 = _lib.f32c(spatial, dev), _lib.f32c(spatial_init, dev)
    n = s.numel() // 4
    g = _lib.f32c(grad_rgb, dev)
    if s.shape[-1] != 4 or s0.shape != s.shape or g.numel() < 3 * n:
        raise ValueError('spatial / spatial_init must be [..., 4] of the same shape and grad_rgb hold 3 floats per row')
    out = torch.empty_like(s)
    _lib.check(_lib.load().nerfail_igsm_step_rgb(_lib.dev(s), _lib.dev(g), _lib.dev(s0), n, float(a), float(epsilon), int(bool(targeted)),
                                                 _lib.dev(out), _lib.stream()))
    return out


def _share(batch, group=None):
    """THE place a batch `(weight_and_index, ori_img[, view_ids])` is taken apart. The ids: the third element, else what travels
    with a MyDataset.collate_views list as `weight_and_index.view_ids`. Returns (this rank's views of the batch as
    (weight_and_index, ori_img, view_ids) - the batch's own objects when the rank owns all of it, None when it owns no view -,
    the size B of the WHOLE batch, sharded: whether the ranks' contributions are summed by a collective)."""
    world, rank = sharding.world_and_rank(group)
    wi, ori = batch[0], batch[1]
    vids = batch[2] if len(batch) > 2 and batch[2] is not None else getattr(wi, 'view_ids', None)
    B = len(vids if vids is not None else wi)
    lo, hi = sharding.shard_range(B, rank, world)
    if hi <= lo:                            # more ranks than views: this rank only takes part in the sum
        parts = None
    elif (lo, hi) == (0, B):
        parts = (wi, ori, vids)
    else:
        parts = (None if wi is None else wi[lo:hi], None if ori is None else ori[lo:hi], None if vids is None else list(vids)[lo:hi])
    return parts, B, world > 1 or sharding.force_collectives()


def _forward_backward(net, spatial, parts, batch_total, label, stats=None, epoch=None, beta=0.):
    """Forward of the views `parts`, their statistics (on the perturbation BEFORE this batch's update, as the reference takes
    them), the objective (1 - |beta|) CE + beta MSE of AS:332-336 as a mean over `batch_total` views (a shard holding k of B
    views contributes with weight k/B), backward down to x_rgba. Returns (x_rgba with its .grad, views, aux, loss, cla)."""
    xr, cla, ori_cla, views, aux = net.attack_forward(spatial, *parts)
    if stats is not None:
        stats.batch(epoch, cla.detach(), ori_cla.detach(), xr, views)
    B = float(batch_total or cla.shape[0])
    loss = torch.nn.functional.cross_entropy(cla, label.to(cla.device).broadcast_to([cla.shape[0]]), reduction='sum') / B
    if beta != 0.:
        loss = (1. - abs(beta)) * loss                                # AS:332-334
    loss.backward()
    if beta != 0.:                                                    # d (beta mean((x_rgba - ori)^2)) / d x_rgba, mean over the WHOLE batch
        _lib.check(_lib.load().nerfail_img_sqerr_grad_add(_lib.dev(xr.detach()), _ori_pointer_table(views), views.B, views.P, int(views.ori_u8),
                                                          2. * float(beta) / (4. * views.P * B), _lib.dev(xr.grad), _lib.stream()))
    return xr, views, aux, loss.detach(), cla.detach()


def _grad_buffer(xr, views, aux, loss, out=None):
    """The rgb gradient as [Ns,3] by the gather backward, then the loss: `out`, 3 Ns + 1 floats."""
    from .GaussNet import hot_backward_rgb
    if out is None:
        out = torch.empty((3 * views.Ns + 1,), dtype=torch.float32, device=xr.device)
    hot_backward_rgb(aux, xr.grad, views, out)
    out[3 * views.Ns] = loss
    return out


def _summed_grad_rgb(net, spatial, share, label, group=None, timing=None, **objective):
    """The 3 Ns + 1 floats of this rank's share (zeros when it owns no view), summed over the ranks by ONE all-reduce (C1: the
    gradient and, in its tail, the loss) when sharded. Identical on every rank."""
    parts, B, sharded = share
    if parts is not None:
        buf = _grad_buffer(*_forward_backward(net, spatial, parts, B, label, **objective)[:4])
    else:
        buf = torch.zeros((3 * (spatial.numel() // 4) + 1,), dtype=torch.float32, device=_cuda())
    if sharded:
        sharding.all_reduce_sum_(buf, group, timing)
    return buf


def _rgb_step(net, spatial, spatial_init, batch, label, a, epsilon, targeted, group=None, timing=None, **objective):
    """THE NeRFail-S step on the rgb-gradient path: (new perturbation, loss). One rank, no collective, net.fused_sign_step: the
    gather backward with the sign step AS:352-392 as its epilogue (the [Ns,3] gradient is never materialised); else the summed
    buffer, then the sign step on every rank. `objective`: stats, epoch and beta of _forward_backward, as nerfail_s passes them."""
    from .GaussNet import hot_backward_rgb_step
    share = parts, B, sharded = _share(batch, group)
    if parts is None or sharded or not getattr(net, 'fused_sign_step', True):
        buf = _summed_grad_rgb(net, spatial, share, label, group, timing, **objective)
        return igsm_step_rgb(spatial, buf, spatial_init, a, epsilon, targeted).view(spatial.shape), buf[-1]
    xr, views, aux, loss, _ = _forward_backward(net, spatial, parts, B, label, **objective)
    return hot_backward_rgb_step(aux, xr.grad, views, spatial, spatial_init, a, epsilon, targeted).view(spatial.shape), loss


def _attack_batch(net, s, s_init, batch, lab, a, epsilon, targeted, beta, stats, epoch, group):
    """One batch of an attack epoch of nerfail_s: _rgb_step with the epoch's statistics and the beta term. Returns the new
    perturbation (the seam at which the tests record every iterate)."""
    return _rgb_step(net, s, s_init, batch, lab, a, epsilon, targeted, group, stats=stats, epoch=epoch, beta=beta)[0]


def perturbation_grad_rgb(net, spatial, weight_and_index, ori_img, label, batch_total=None, view_ids=None, out=None):
    """The NeRFail-S step's gradient in the form the step consumes (AS:357-392 reads grad[..., :3] only): a flat buffer of
    3 Ns + 1 floats - d(CE)/d(spatial rgb) as [Ns,3], then the loss - filled by the rgb-only backward (no `x` tensor, 5 bytes
    per pixel between forward and backward, 23 MB instead of 30.7 MB for the all-reduce, which carries the loss in the same
    collective). The three channels equal perturbation_grad()'s bit for bit."""
    xr, views, aux, loss, cla = _forward_backward(net, spatial, (weight_and_index, ori_img, view_ids), batch_total, label)
    return _grad_buffer(xr, views, aux, loss, out), cla


def sharded_perturbation_grad_rgb(net, spatial, weight_and_index, ori_img, label, group=None, timing=None, view_ids=None):
    """perturbation_grad_rgb of this rank's share of the batch's views, then ONE all-reduce of the 3 Ns + 1 floats (C1: the
    gradient and, in its tail, the loss). Identical on every rank. `timing`: optional dict; gets HIP events around the
    collective ('allreduce_events', sharding.all_reduce_sum_)."""
    return _summed_grad_rgb(net, spatial, _share((weight_and_index, ori_img, view_ids), group), label, group, timing)


def sharded_perturbation_grad(net, spatial, weight_and_index, ori_img, label, group=None, timing=None, view_ids=None):
    """d(mean CE over the WHOLE batch)/d(spatial), identical on every rank: this rank differentiates its contiguous
    share of the batch's views (weight k/B), then ONE all-reduce sums the [P,H,W,4] gradient (C1).
    `timing`: as sharded_perturbation_grad_rgb."""
    parts, B, sharded = _share((weight_and_index, ori_img, view_ids), group)
    if parts is not None:
        g, loss, _ = perturbation_grad(net, spatial, parts[0], parts[1], label, batch_total=B, view_ids=parts[2])
    else:
        g, loss = torch.zeros_like(spatial), torch.zeros((), device=spatial.device)
    if sharded:
        sharding.all_reduce_sum_(g, group, timing)   # C1: the perturbation-gradient all-reduce
        sharding.all_reduce_sum_(loss, group)
    return g, loss


def perturbation_step_rgb(net, spatial, spatial_init, weight_and_index, ori_img, label, a, epsilon, targeted, view_ids=None):
    """One rank, no collective: forward, CE, classifier backward, then the gather backward with the sign step AS:352-392 as its
    epilogue (GaussNet.hot_backward_rgb_step) - the [Ns,3] gradient is never materialised. Returns (new perturbation, loss);
    bit-identical to perturbation_grad_rgb + igsm_step_rgb."""
    from .GaussNet import hot_backward_rgb_step
    xr, views, aux, loss, _ = _forward_backward(net, spatial, (weight_and_index, ori_img, view_ids), None, label)
    return hot_backward_rgb_step(aux, xr.grad, views, spatial, spatial_init, a, epsilon, targeted), loss


def nerfail_s_step(net, spatial, spatial_init, weight_and_index, ori_img, label, a=2.0, epsilon=32.0,
                   targeted=False, group=None, timing=None, view_ids=None):
    """One NeRFail-S iteration (AS:304-392) on one batch of views. Sharded over ranks when torch.distributed is up:
    every rank ends with the identical perturbation tensor."""
    if getattr(net, 'deterministic', True) and getattr(net, 'rgb_grad_only', True):
        return _rgb_step(net, spatial, spatial_init, (weight_and_index, ori_img, view_ids), label, a, epsilon, targeted, group, timing)
    g, loss = sharded_perturbation_grad(net, spatial, weight_and_index, ori_img, label, group, timing, view_ids)
    return igsm_step(spatial, g, spatial_init, a, epsilon, targeted), loss


def nerfail_s_loop(net, spatial, spatial_init, batches, label, iters, a=2.0, epsilon=32.0, targeted=False, group=None,
                   on_iter=None):
    """The AS:278-392 loop shape of BASELINE configs[2]: `iters` passes over `batches` (list of (weight_and_index,
    ori_img[, view_ids]) per batch of views), the perturbation updated after EVERY batch (sequential dependence, AS:306-392).
    Returns the final perturbation; `on_iter(it, b, s, loss)` sees every iterate."""
    s = spatial
    for it in range(iters):
        for b, batch in enumerate(batches):
            s, loss = nerfail_s_step(net, s, spatial_init, batch[0], batch[1], label, a, epsilon, targeted, group,
                                     view_ids=batch[2] if len(batch) > 2 else None)
            if on_iter is not None:
                on_iter(it, b, s, loss)
    return s


# ---------------------------------------------------------------------------------------------- the product loop (AS:278-442)
STAT_FIELDS = ('test_loss', 'test_acc', 'attack_loss', 'attack_acc', 'img_loss', 'views', 'taken', 'best_epoch', 'best_acc',
               'best_loss', 'epoch', 'test_correct', 'attack_correct')


class AttackResult:
    """What nerfail_s returns. `best`: the perturbation the rule of AS:422-431 kept (device tensor) - the attack's result, the
    tensor the export epoch rendered; `last`: the last iterate; `stats`: one dict per epoch (STAT_FIELDS, plus epsilon_3d_min /
    epsilon_3d_max; the last one is the export epoch's); `best_epoch` / `best_acc`: epoch and attack accuracy of `best`
    (-1 / None when no attack epoch ran). The export epoch's record carries the rule of AS:422-431 applied once more, to the
    export pass's accuracy, as the reference applies it after its last epoch: its `taken` / `best_epoch` / `best_acc` /
    `best_loss` fields describe that comparison, not the kept tensor - `best_epoch` / `best_acc` of this object do (they
    are the last ATTACK epoch's record)."""

    def __init__(self, best, last, stats, best_epoch, best_acc):
        self.best, self.last, self.stats, self.best_epoch, self.best_acc = best, last, stats, best_epoch, best_acc


def _read_stats(record, minmax):
    """THE host read of an epoch: its record and the running epsilon_3d [min, max], one device-to-host copy."""
    v = torch.cat([record, minmax]).cpu().tolist()
    d = dict(zip(STAT_FIELDS, v))
    for k in ('views', 'taken', 'best_epoch', 'epoch', 'test_correct', 'attack_correct'):
        d[k] = int(d[k])
    d['epsilon_3d_min'], d['epsilon_3d_max'] = v[-2], v[-1]
    return d


def _ori_pointer_table(views):
    return (_lib.c_p * views.B)(*[o.data_ptr() for o in views.ori])


class _EpochStats:
    """The device side of one run's bookkeeping: a stats row and a record per epoch, the best record, the flag word."""

    def __init__(self, epochs, targeted, label, dev):
        n = _lib.ATTACK_ROW_FLOATS
        self.rows = torch.zeros((epochs, n), dtype=torch.float32, device=dev)
        self.records = torch.zeros((epochs, n), dtype=torch.float32, device=dev)
        self.best = torch.zeros((4,), dtype=torch.float32, device=dev)     # {acc, loss, epoch, -}; filled on the device: no host copy
        self.best[0:1].fill_(0. if targeted else 10000.)                   # AS:270-276
        self.best[2:3].fill_(-1.)
        self.flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.lib = _lib.load()
        self.scratch = torch.empty((self.lib.nerfail_img_sqerr_scratch_bytes() // 8,), dtype=torch.float64, device=dev)
        self.targeted, self.label = int(bool(targeted)), int(label)

    def batch(self, epoch, cla, ori_cla, x_rgba, views):
        """AS:319-344 for one batch (this rank's views of it): five sums into the epoch's row, no host read."""
        row = _lib.dev(self.rows[epoch])
        c, oc = _lib.f32c(cla), _lib.f32c(ori_cla)
        _lib.check(self.lib.nerfail_attack_logit_stats(_lib.dev(c), _lib.dev(oc), c.shape[0], c.shape[1], self.label, row, _lib.stream()))
        _lib.check(self.lib.nerfail_img_sqerr(_lib.dev(x_rgba.detach()), _ori_pointer_table(views), views.B, views.P, int(views.ori_u8),
                                              _lib.c_p(self.scratch.data_ptr()), row, _lib.stream()))

    def close(self, epoch, group):
        sharding.all_reduce_sum_(self.rows[epoch], group)            # the ONE extra collective of an epoch (when sharded): 16 floats
        _lib.check(self.lib.nerfail_attack_epoch_close(_lib.dev(self.rows[epoch]), _lib.dev(self.best), epoch, self.targeted,
                                                       _lib.dev(self.records[epoch]), _lib.dev(self.flag), _lib.stream()))

    def keep_if_taken(self, s, best):
        _lib.check(self.lib.nerfail_copy_if(_lib.dev(self.flag), _lib.dev(s), _lib.dev(best), s.numel(), _lib.stream()))


class _ExportBuffers:
    """Device uint8 [2,B,H,W,4] (adversarial image, mask image) and its pinned host twin, kept per batch shape."""

    def __init__(self):
        self.bufs = {}

    def get(self, shape, dev):
        if shape not in self.bufs:
            self.bufs[shape] = (torch.empty((2,) + shape, dtype=torch.uint8, device=dev),
                                torch.empty((2,) + shape, dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
        return self.bufs[shape]


def _export_batch(net, best, batch, index, stats, epoch, group, bufs, on_export):
    """AS:310-317, 394-403 for one batch (this rank's views of it): the best tensor through the forward without gradient, the
    same statistics, then x_rgba and the unclipped mask image x as uint8 to the host in ONE copy."""
    parts = _share(batch, group)[0]
    if parts is None:
        return
    x, x_rgba, cla, ori_cla, views = net.export_forward(best, *parts)
    stats.batch(epoch, cla, ori_cla, x_rgba, views)
    if on_export is None:
        return
    d_u8, h_u8, ev = bufs.get(tuple(x_rgba.shape), x_rgba.device)         # (free again: every call waits for its own copy below)
    n = x_rgba.numel()
    _lib.check(stats.lib.nerfail_export_u8(_lib.dev(x_rgba), n, _lib.dev(d_u8[0]), _lib.stream()))
    _lib.check(stats.lib.nerfail_export_u8(_lib.dev(x), n, _lib.dev(d_u8[1]), _lib.stream()))
    h_u8.copy_(d_u8, non_blocking=True)
    ev.record()
    ev.synchronize()
    arr = h_u8.numpy()
    on_export(index, parts[2], arr[0].copy(), arr[1].copy())


def nerfail_s(net, spatial, batches, label, epochs, a=2., epsilon=32., targeted=False, beta=0., export_batches=None,
              on_export=None, log=print, group=None):
    """The NeRFail-S attack loop, AS:278-442, as one call: the counterpart of train.train().

    `spatial`: the perturbation table [P,H,W,4] (BGRA rows; also the init the epsilon clamp is centred on, AS:265). `batches`:
    the attack epochs' batch list - or a callable of the epoch that returns it (a reshuffling / subsampling loader, AS:230) -
    each batch `(weight_and_index, ori_img[, view_ids])` as nerfail_s_loop takes them. `label`: the class index (int or a
    tensor). Epochs 0 .. epochs-2 attack: per batch the forward, the batch's statistics (CE and accuracy of the clean and of
    the attacked logits, the image loss MSE(x_rgba, ori_img), all of the perturbation BEFORE this batch's update, AS:319-344),
    then the step - with beta == 0 today's fused path (bit for bit nerfail_s_loop), else the objective
    (1 - |beta|) CE + beta MSE of AS:332-336. At the end of an epoch the sums become the epoch's means (AS:405-413), the
    perturbation is kept as the best one when its attack accuracy is <= the best so far (>= when targeted; a tie goes to the
    later epoch, AS:422-431) and net.epsilon_3d_zero() runs (AS:420). Epoch epochs-1 is the export epoch (AS:299-312,
    394-403): the BEST tensor, no gradient, over `export_batches` (default: the attack batches), the same statistics, and
    `on_export(batch_index, view_ids, adv_u8, mask_u8)` per batch with host uint8 arrays [B,H,W,4] of x_rgba and of the
    unclipped mask image x, converted as cv2.imwrite converts a float image. With epochs == 1 there is no attack epoch and the
    initial tensor is exported (AS:266 sets the best tensor to the init before the loop, so the reference's only epoch would
    render the init as well; nothing of it is tested there).

    Nothing between epoch ends waits for the GPU: the statistics accumulate in a device row, the rule is decided on the
    device (nerfail_attack_epoch_close) and the best tensor kept by a conditional copy (nerfail_copy_if). One host read per
    epoch (the epoch's record, for the four log lines of AS:415-418 and print_epsilon's two; log=None keeps the read and
    drops the lines); the export epoch additionally waits once per batch for its images. Requires the deterministic
    rgb-gradient step path (net.deterministic and net.rgb_grad_only, the defaults).

    More than one rank (torch.distributed; `group`): every batch's views are sharded as nerfail_s_step shards them, each rank
    accumulates the statistics of the views it owns, ONE extra all-reduce per epoch sums the stats row before the close, so
    every rank takes the same decisions and ends with the same `best`. on_export is called on every rank for its own views.

    Returns an AttackResult (best, last, stats, best_epoch, best_acc)."""
    if not (getattr(net, 'deterministic', True) and getattr(net, 'rgb_grad_only', True)):
        raise ValueError('nerfail_s runs the deterministic rgb-gradient step path (net.deterministic and net.rgb_grad_only)')
    epochs = int(epochs)
    if epochs < 1:
        raise ValueError('epochs must be at least 1 (the last epoch is the export epoch)')
    if not -1. <= float(beta) <= 1.:
        raise ValueError('beta must be in [-1, 1] (AS:332-336)')
    dev = _cuda()
    beta = float(beta)
    rank = sharding.world_and_rank(group)[1]
    label_i = int(label)                                              # (a device label is read once, before the first epoch)
    lab = torch.full((), label_i, dtype=torch.int64, device=dev)
    s_init = _lib.f32c(spatial, dev)
    s = s_init
    best = s_init.clone()
    stats = _EpochStats(epochs, targeted, label_i, dev)
    bufs = _ExportBuffers()
    records = []

    def finish(epoch):
        d = _read_stats(stats.records[epoch], net._mm())
        records.append(d)
        if log is not None and rank == 0:
            log('Attack ...... [%d/%d]' % (epoch, epochs))
            log('{} Loss: {:.4f} Acc: {:.4f}'.format('test', d['test_loss'], d['test_acc']))                       # AS:415-418
            log('{} Loss: {:.4f} Acc: {:.4f}'.format('attack', d['attack_loss'], d['attack_acc']))
            b1 = 1. - beta                                                                                        # (AS:340 has no abs)
            log('{} Beta Loss: {:.4f} Beta Img Loss: {:.4f}'.format('attack', b1 * d['attack_loss'], beta * d['img_loss']))
            log('{} Img Loss: {:.4f} Total Loss: {:.4f}'.format('attack', d['img_loss'],
                                                                  (1. - abs(beta)) * d['attack_loss'] + beta * d['img_loss']))
            log('epsilon_3d_min:  %s' % d['epsilon_3d_min'])
            log('epsilon_3d_max:  %s' % d['epsilon_3d_max'])
        net.epsilon_3d_zero()                                         # AS:420

    for epoch in range(epochs - 1):
        for batch in (batches(epoch) if callable(batches) else batches):
            s = _attack_batch(net, s, s_init, batch, lab, float(a), float(epsilon), bool(targeted), beta, stats, epoch, group)
        stats.close(epoch, group)
        stats.keep_if_taken(s, best)
        finish(epoch)
    epoch = epochs - 1
    exp = export_batches if export_batches is not None else batches
    for i, batch in enumerate(exp(epoch) if callable(exp) else exp):
        _export_batch(net, best, batch, i, stats, epoch, group, bufs, on_export)
    stats.close(epoch, group)                                         # (its decision moves no tensor: the epoch ran on `best` itself)
    finish(epoch)
    last_attack = records[-2] if epochs > 1 else None
    return AttackResult(best, s, records, last_attack['best_epoch'] if last_attack else -1,
                        last_attack['best_acc'] if last_attack else None)
