"""The attack-step arithmetic of attack_NeRFail_S.py (reference = AS), on the MI355X.

`igsm_step` is AS:352-392 as one kernel. One iteration of the AS:304-392 loop body is written once, as `_rgb_step`: `_share`
takes the batch apart (view ids, size, this rank's views), `_forward_backward` runs gauss_net's forward, the optional epoch
statistics, the CE loss (+ the beta term) and the classifier backward, and the step ends in the fused gather backward + sign
step (one rank) or in the 3 Ns + 1 float buffer - rgb gradient, loss in the tail - that ONE all-reduce sums over the ranks
(RCCL over xGMI on the GPU box, gloo in the CPU tests) before every rank applies the identical step: the only collective on
the whole path. `nerfail_s_step` is that body; `nerfail_s`, the whole AS:278-442 loop as a product
(epoch statistics, best tensor and export epoch, decided on the device, csrc/attack_stats.hip), calls it with its statistics
and beta and adds one all-reduce of a 16-float statistics row per EPOCH. perturbation_grad, the four-channel autograd path,
stays apart: it is what the rgb path is compared against. `nerfail` is the universal attack (attack_NeRFail.py:269-512), `igsm_2d`
the 2-D baseline of NeRFail-S (attack_IGSM_2D.py:263-416, csrc/u2d.hip) and `uap_2d` the 2-D baseline of NeRFail
(attack_UAP_2D.py:241-358, csrc/uap2d.hip), each as one call.
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
    lo, hi = sharding.batch_share(B, rank, world)    # THE ownership rule (sharding.owned_positions: the same call per batch)
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


def _attack_result(best, last, records, epochs):
    """The AttackResult of nerfail_s and igsm_2d: best_epoch / best_acc are the last ATTACK epoch's record (records[-1] is the
    export epoch's)."""
    d = records[-2] if epochs > 1 else None
    return AttackResult(best, last, records, d['best_epoch'] if d else -1, d['best_acc'] if d else None)


def _read_stats(record, minmax=None):
    """THE host read of an epoch: its record and, where the loop has one (nerfail_s), the running epsilon_3d [min, max], in one
    device-to-host copy."""
    v = (record if minmax is None else torch.cat([record, minmax])).cpu().tolist()
    d = dict(zip(STAT_FIELDS, v))
    for k in ('views', 'taken', 'best_epoch', 'epoch', 'test_correct', 'attack_correct'):
        d[k] = int(d[k])
    if minmax is not None:
        d['epsilon_3d_min'], d['epsilon_3d_max'] = v[-2], v[-1]
    return d


def _log_loss_acc(log, d):
    """The two lines every epoch (AS:415-416, IG:402-403) and every pass (AN:481-482, UA:345-346) print."""
    log('{} Loss: {:.4f} Acc: {:.4f}'.format('test', d['test_loss'], d['test_acc']))
    log('{} Loss: {:.4f} Acc: {:.4f}'.format('attack', d['attack_loss'], d['attack_acc']))


def _log_epsilon(log, d):
    """print_epsilon (AS:419, AN:487)."""
    log('epsilon_3d_min:  %s' % d['epsilon_3d_min'])
    log('epsilon_3d_max:  %s' % d['epsilon_3d_max'])


def _log_epoch(log, epoch, epochs, d, beta):
    """The reference's log block of an epoch (AS:415-418 = IG:402-405, where beta is the constant 0.) and print_epsilon's two
    lines when the record carries them. log=None prints nothing."""
    if log is None:
        return
    log('Attack ...... [%d/%d]' % (epoch, epochs))
    _log_loss_acc(log, d)
    b1 = 1. - beta                                                                                                # (AS:340 has no abs)
    log('{} Beta Loss: {:.4f} Beta Img Loss: {:.4f}'.format('attack', b1 * d['attack_loss'], beta * d['img_loss']))
    log('{} Img Loss: {:.4f} Total Loss: {:.4f}'.format('attack', d['img_loss'], (1. - abs(beta)) * d['attack_loss'] + beta * d['img_loss']))
    if 'epsilon_3d_min' in d:
        _log_epsilon(log, d)


def _check_epochs(epochs):
    epochs = int(epochs)
    if epochs < 1:
        raise ValueError('epochs must be at least 1 (the last epoch is the export epoch)')
    return epochs


def _check_one_rank(what):
    """nerfail and uap_2d update their table view by view: `what` names the loop and its table in the refusal."""
    world = sharding.world_and_rank(None)[0]
    if world > 1:
        raise ValueError('%s view by view: there is nothing to shard over %d ranks' % (what, world))


def _check_export_views(caller, items):
    """An export epoch without views would never end the loop (nothing sets tensor_not_changed). `items`: the views of the export
    epoch where they are known - a callable is checked when its pass begins."""
    if items is not None and not callable(items) and len(items) == 0:
        raise ValueError('%s: the export epoch needs at least one view (export_views is empty)' % caller)


def _ori_pointer_table(views):
    return (_lib.c_p * views.B)(*[o.data_ptr() for o in views.ori])


def _logit_stats(lib, cla, ori_cla, label, row):
    """AS:319-344's four logit sums and two correct counts of one batch into the stats row `row`, no host read."""
    c, oc = _lib.f32c(cla), _lib.f32c(ori_cla)
    _lib.check(lib.nerfail_attack_logit_stats(_lib.dev(c), _lib.dev(oc), c.shape[0], c.shape[1], int(label), _lib.dev(row), _lib.stream()))


class _EpochStats:
    """The device side of one run's bookkeeping: a stats row and a record per epoch, the best record, the flag word. `strict`:
    the rule an epoch is closed with - False AS:422-431 (<= / >=, a tie goes to the later epoch; the stats row all-reduced in
    front of it), True IG:407-416 (< / >, a tie keeps the earlier epoch; one rank)."""

    def __init__(self, epochs, targeted, label, dev, strict=False):
        n = _lib.ATTACK_ROW_FLOATS
        self.rows = torch.zeros((epochs, n), dtype=torch.float32, device=dev)
        self.records = torch.zeros((epochs, n), dtype=torch.float32, device=dev)
        self.best = torch.zeros((4,), dtype=torch.float32, device=dev)     # {acc, loss, epoch, -}; filled on the device: no host copy
        self.best[0:1].fill_(0. if targeted else 10000.)                   # AS:270-276
        self.best[2:3].fill_(-1.)
        self.flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.lib = _lib.load()
        self.scratch = torch.empty((self.lib.nerfail_img_sqerr_scratch_bytes() // 8,), dtype=torch.float64, device=dev)
        self.targeted, self.label, self.strict = int(bool(targeted)), int(label), bool(strict)

    def batch(self, epoch, cla, ori_cla, x_rgba, views):
        """AS:319-344 for one batch (this rank's views of it): five sums into the epoch's row, no host read."""
        _logit_stats(self.lib, cla, ori_cla, self.label, self.rows[epoch])
        _lib.check(self.lib.nerfail_img_sqerr(_lib.dev(x_rgba.detach()), _ori_pointer_table(views), views.B, views.P, int(views.ori_u8),
                                              _lib.c_p(self.scratch.data_ptr()), _lib.dev(self.rows[epoch]), _lib.stream()))

    def close(self, epoch, group=None):
        """The epoch's sums become its record (means, the rule's decision, the best record) and the flag word, on the device."""
        if self.strict:
            ops.u2d_epoch_close(self.rows[epoch], self.best, epoch, bool(self.targeted), self.records[epoch], self.flag)
            return
        sharding.all_reduce_sum_(self.rows[epoch], group)            # the ONE extra collective of an epoch (when sharded): 16 floats
        _lib.check(self.lib.nerfail_attack_epoch_close(_lib.dev(self.rows[epoch]), _lib.dev(self.best), epoch, self.targeted,
                                                       _lib.dev(self.records[epoch]), _lib.dev(self.flag), _lib.stream()))

    def keep_if_taken(self, s, best):
        _lib.check(self.lib.nerfail_copy_if(_lib.dev(self.flag), _lib.dev(s), _lib.dev(best), s.numel(), _lib.stream()))


class _ExportBuffers:
    """The export epoch's way to the host: a device uint8 buffer with one 16-byte aligned slot per image and its pinned host twin,
    kept per tuple of image sizes for the run."""

    def __init__(self):
        self.bufs = {}
        self.lib = _lib.load()

    def to_host(self, *images):
        """float32 device tensors -> one host uint8 array per tensor, shaped like it, converted as cv2.imwrite converts a float
        image (nerfail_export_u8): one launch per image, ONE copy, one event wait. The arrays are copies: they alias neither the
        pinned buffer nor each other. An image whose pointer is not 16-byte aligned (a row range of the best table) is cloned
        first: the kernel reads 128 bits at a time."""
        sizes = tuple(t.numel() for t in images)
        starts = [0]
        for n in sizes:
            starts.append(starts[-1] + -(-n // 16) * 16)
        if sizes not in self.bufs:                                         # (free again: every call waits for its own copy below)
            self.bufs[sizes] = (torch.empty((starts[-1],), dtype=torch.uint8, device=images[0].device),
                                torch.empty((starts[-1],), dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
        d_u8, h_u8, ev = self.bufs[sizes]
        for t, n, at in zip(images, sizes, starts):
            src = t if t.data_ptr() % 16 == 0 else t.clone()
            _lib.check(self.lib.nerfail_export_u8(_lib.dev(src), n, _lib.dev(d_u8[at:at + n]), _lib.stream()))
        h_u8.copy_(d_u8, non_blocking=True)
        ev.record()
        ev.synchronize()
        arr = h_u8.numpy()
        return [arr[at:at + n].reshape(tuple(t.shape)).copy() for t, n, at in zip(images, sizes, starts)]


def _export_batch(net, best, batch, index, stats, epoch, group, bufs, on_export, export_sink=None):
    """AS:310-317, 394-403 for one batch (this rank's views of it): the best tensor through the forward without gradient, the
    same statistics, then x_rgba and the unclipped mask image x as uint8 to the host in ONE copy. `export_sink` takes x_rgba on
    the device first (retrain.PoisonedTrainSet); without on_export nothing is copied to the host."""
    parts = _share(batch, group)[0]
    if parts is None:
        return
    x, x_rgba, cla, ori_cla, views = net.export_forward(best, *parts)
    stats.batch(epoch, cla, ori_cla, x_rgba, views)
    if export_sink is not None:
        export_sink.put(parts[2], x_rgba)
    if on_export is not None:
        on_export(index, parts[2], *bufs.to_host(x_rgba, x))


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
    every rank takes the same decisions and ends with the same `best`. on_export is called on every rank for its own views
    (an export sink likewise receives them: retrain.PoisonedTrainSet.gather() then makes every rank's sink complete). The views
    a rank owns are those of sharding.owned_positions: scene.build_scene_maps(shard_batch=) registers exactly them per rank.

    nerfail_s_into(export_sink, ...) is this call with a device-side sink behind the export epoch.

    Returns an AttackResult (best, last, stats, best_epoch, best_acc)."""
    return _nerfail_s(None, net, spatial, batches, label, epochs, a, epsilon, targeted, beta, export_batches, on_export, log, group)


def nerfail_s_into(export_sink, net, spatial, batches, label, epochs, *args, **kwargs):
    """nerfail_s(net, spatial, batches, label, epochs, ...) with an export sink: an object with put(view_ids, x_rgba) -
    retrain.PoisonedTrainSet - that receives every export batch's x_rgba [B,H,W,4] as a device tensor, before and independently
    of on_export (the export batches then need view ids). With on_export None no image is copied to the host. A function of
    its own because nerfail_s's parameter list is pinned as it is; nerfail, igsm_2d and uap_2d take `export_sink=` directly."""
    return _nerfail_s(export_sink, net, spatial, batches, label, epochs, *args, **kwargs)


def _nerfail_s(export_sink, net, spatial, batches, label, epochs, a=2., epsilon=32., targeted=False, beta=0., export_batches=None,
               on_export=None, log=print, group=None):
    """The body of nerfail_s (its defaults repeated for nerfail_s_into's pass-through)."""
    if not (getattr(net, 'deterministic', True) and getattr(net, 'rgb_grad_only', True)):
        raise ValueError('nerfail_s runs the deterministic rgb-gradient step path (net.deterministic and net.rgb_grad_only)')
    epochs = _check_epochs(epochs)
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
        records.append(_read_stats(stats.records[epoch], net._mm()))
        _log_epoch(log if rank == 0 else None, epoch, epochs, records[-1], beta)
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
        _export_batch(net, best, batch, i, stats, epoch, group, bufs, on_export, export_sink)
    stats.close(epoch, group)                                         # (its decision moves no tensor: the epoch ran on `best` itself)
    finish(epoch)
    return _attack_result(best, s, records, epochs)


# ---------------------------------------------------------------------------------------------- the product loop (AN:269-512)
class NerfailResult:
    """What nerfail returns. `best`: the table the rule of AN:490-503 kept (device tensor) - the attack's result, what the export
    epoch rendered; `last`: the table the loop ended on (after an export epoch the reference's table IS the best tensor,
    AN:345, so `last` then aliases it until the rule replaces `best` by a copy); `m1_best`, `m2_best`, `best_acc`: what the rule
    recorded with `best`; `stats`: one dict per PASS over the views (a pass is one turn of AN:311's while loop; `epoch` is the
    epoch it ran as, `next_epoch` where the loop went); `need_to_log_dict`: the reference's, keyed "m1-<m1> epoch-<epoch>"
    with the values AFTER the pass's m1 / epoch update, as AN:485 forms them."""

    def __init__(self, best, last, m1_best, m2_best, best_acc, stats, need_to_log_dict):
        self.best, self.last, self.m1_best, self.m2_best, self.best_acc = best, last, m1_best, m2_best, best_acc
        self.stats, self.need_to_log_dict = stats, need_to_log_dict


class _PassStats:
    """One pass's running sums of AN:358-376 in a device row (nerfail_attack_logit_stats): what _export_batch calls `stats`."""

    def __init__(self, label, dev):
        self.lib = _lib.load()
        self.label = int(label)
        self.row = torch.zeros((_lib.ATTACK_ROW_FLOATS,), dtype=torch.float32, device=dev)

    def batch(self, epoch, cla, ori_cla, x_rgba=None, views=None):
        _logit_stats(self.lib, cla, ori_cla, self.label, self.row)

    def read(self, n_views, minmax=None):
        """THE host read of a pass, one device-to-host copy: its means as AN:476-480 / UA:340-344 divide the four sums and the
        two correct counts by `n_views` = len(now_dataloader.dataset) (NaN for a pass without views) and, where the loop has one
        (nerfail), epsilon_3d's [min, max]."""
        v = (self.row if minmax is None else torch.cat([self.row, minmax])).cpu().tolist()
        d = dict(views=n_views, test_correct=int(v[4]), attack_correct=int(v[5]))
        for k, total in (('test_loss', v[0] + v[1]), ('test_acc', d['test_correct']), ('attack_loss', v[2] + v[3]),
                         ('attack_acc', d['attack_correct'])):
            d[k] = total / n_views if n_views else float('nan')
        if minmax is not None:
            d['epsilon_3d_min'], d['epsilon_3d_max'] = v[-2], v[-1]
        return d


class _Visits:
    """What a pass of nerfail / uap_2d counts view by view; fields() is its part of the pass's record. `key`: what names the
    visit in `visits` (nerfail: the position in the pass, uap_2d: the view index)."""

    def __init__(self):
        self.visits, self.skipped, self.attacked, self.completed, self.iters = [], 0, 0, 0, 0

    def skip(self, key):
        self.skipped += 1
        self.visits.append((key, True, 0, []))

    def ran(self, key, iter_k, classes):
        """A DeepFool call of iter_k iterations; `classes`: the class chosen in each, None with the mirror."""
        self.attacked += 1
        self.iters += iter_k
        self.visits.append((key, False, iter_k, classes))

    def fields(self):
        return dict(skipped=self.skipped, attacked=self.attacked, completed=int(self.completed), deepfool_iters=self.iters,
                    visits=self.visits)


def _deepfool_kw(num_classes, df_max_iter, label, targeted, overshoot, m1, m2):
    """The keyword arguments a pass hands to deepfool[_2d][_native] (AN:396-402, UA:306-312)."""
    return dict(num_classes=num_classes, max_iter=df_max_iter, target_label=label if targeted else None, overshoot=overshoot, m1=m1, m2=m2)


def _pass_done(index, table):
    """Called at the end of every pass with the table as the pass left it (the seam at which the tests record it)."""


def _same_class(cla, ori_cla):
    """AN:387-392: the raw (unbumped) argmax of the attacked logits equals the clean one. One small host read per visit."""
    return bool(torch.argmax(cla[0]) == torch.argmax(ori_cla[0]))


def nerfail(net, spatial, views, label, epochs, m1=8, m2=100, targeted=False, df_max_iter=1000, overshoot=0.02, num_classes=8,
            m2_max_limit=10000, accumulate_incomplete=False, export_views=None, on_export=None, log=print, native=None,
            export_sink=None):
    """The NeRFail universal attack, attack_NeRFail.py:269-512 (= AN), as one call: the counterpart of nerfail_s.

    `spatial`: the perturbation table [P,H,W,4]. `views`: a list of batch-1 items `(weight_and_index, ori_img[, view_id])`, or a
    callable of the pass number that returns such a list (the reshuffled gauss_dataset_rand_select loader of AN:246-249).
    `label`: the views' class, or the target class when `targeted`. `m1`, `m2`: the two margins (args.m1 / args.m2).

    The loop is the reference's, quirks included. `while epoch < epochs` steps `epoch` itself. A pass before the last epoch
    visits every view: open_update_epsilon_3d, the forward, the four running sums of AN:358-376 (in a device row: no host read
    per view for them), close_update_epsilon_3d, and - only when the raw argmax of the attacked logits still equals the clean
    one (AN:387-394) - DeepFool on the view; its perturbation is added to the table when it finished before df_max_iter (or
    `accumulate_incomplete`), else the m2 * 10 rule of AN:410-418 counts it (m2 is reset at the start of every pass, AN:332).
    A pass that changed nothing at epoch 0 bisects m1 downwards between m1_list = [0, m1] (AN:442-453) and runs epoch 0 again -
    at any other epoch it jumps to the last epoch; the last epoch is the export epoch: the BEST tensor, without gradient, over
    `export_views` (default: the views; `on_export(index, view_ids, adv_u8, mask_u8)` per view as in nerfail_s), after which m1
    is bisected upwards and the loop returns to epoch 0 while m1 < m1_list[1] (AN:456-468) - the table is then NOT reset: it is
    the best tensor itself. Each pass ends with its means (sums / views of the pass), print_epsilon, epsilon_3d_zero and the
    best rule of AN:490-503 with the m1 / m2 the bisection just set.

    Host reads: one per visit for the skip decision, DeepFool's own (deepfool_native: one per iteration), one per pass for the
    record and the log lines. `native=None` runs deepfool.deepfool_native (which itself falls through to the mirror where it
    does not apply), `native=False` the mirror deepfool.deepfool (a resident view given by name alone is handed to it as the tensors
    the visit's forward resolved). An export epoch without views is a ValueError. The update is sequential over the views: there is nothing to
    shard, and more than one rank is a ValueError. `export_sink`: as for nerfail_s - put([view_id], x_rgba) per exported view.

    Returns a NerfailResult. Every dict of `stats` holds m1 / m2 (at the end of the pass), m1_pass (the m1 the pass ran with),
    epoch, next_epoch, test_loss, test_acc, attack_loss, attack_acc, views, skipped, attacked, completed, deepfool_iters,
    m2_raises, taken, epsilon_3d_min, epsilon_3d_max and `visits`: per visit (position in the pass, skipped, iter_k, the chosen
    class of every iteration or None with the mirror)."""
    import time
    from . import deepfool as DF
    epochs = _check_epochs(epochs)
    _check_export_views('nerfail', export_views if export_views is not None else views)
    _check_one_rank('nerfail updates the table')
    dev = _cuda()
    say = log if log is not None else (lambda *_: None)
    label_i = int(label)
    args_m1, args_m2 = m1, m2
    m1_list = [0, m1]
    table = _lib.f32c(spatial, dev).clone()
    best = table.clone()
    best_acc = 0 if targeted else 10000                                   # AN:294-303
    m1_best = m2_best = 0
    bufs = _ExportBuffers()
    records, need_to_log = [], {}
    epoch, n_pass = 0, 0
    while epoch < epochs:
        say('Attack ...... [' + str(epoch) + '/' + str(epochs) + ']')
        since = time.time()
        no_attack = attack_all = 0                                        # AN:329-330
        m2 = args_m2                                                      # AN:332
        not_changed = True
        export = epoch == epochs - 1
        src = (export_views if export_views is not None else views) if export else views
        items = list(src(n_pass) if callable(src) else src)
        if export:
            _check_export_views('nerfail', items)
        stats, seen, raises = _PassStats(label_i, dev), _Visits(), 0
        pass_epoch, pass_m1 = epoch, m1
        for i, item in enumerate(items):
            wi, ori = item[0], item[1]
            vid = item[2] if len(item) > 2 and item[2] is not None else None
            vids = None if vid is None else [vid]
            if export:
                if i == 0:
                    table = best                                          # AN:345: the table IS the best tensor from here on
                    say('best m1=' + str(m1_best))
                    say('best m2=' + str(m2_best))
                    say('best acc=' + str(best_acc))
                net.open_update_epsilon_3d()
                _export_batch(net, table, (wi, ori, vids), i, stats, epoch, None, bufs, on_export, export_sink)
                not_changed = False                                       # AN:432
                continue
            net.open_update_epsilon_3d()
            with torch.no_grad():
                _, _, cla, _, ori_cla = net(table, wi, ori, view_ids=vids) if vids is not None else net(table, wi, ori)
            stats.batch(epoch, cla, ori_cla)
            net.close_update_epsilon_3d()
            if not _same_class(cla, ori_cla):
                seen.skip(i)
                continue
            kw = _deepfool_kw(num_classes, df_max_iter, label_i, targeted, overshoot, m1, m2)
            if native is None or native:
                dr, iter_k, _, _, _, classes = DF.deepfool_native((table, wi, ori), None, net, view_ids=vids, **kw)
            else:
                if wi is None or ori is None:                             # a resident view: the mirror takes tensors, not names
                    wi, ori = net._last_views.wi_batch(), net._last_ori
                dr, iter_k, _, _, _ = DF.deepfool((table, wi, ori), None, net, **kw)
                classes = None
            seen.ran(i, iter_k, classes)
            if iter_k < df_max_iter or accumulate_incomplete:             # AN:405-409
                say('iter_k < df_max_iter')
                table += dr
                not_changed = False
                attack_all += 1
                seen.completed += iter_k < df_max_iter
            elif m2 < m2_max_limit:                                       # AN:410-418
                no_attack += 1
                attack_all += 1
                if attack_all > 10 and (no_attack / attack_all) > 0.5:
                    m2 = m2 * 10
                    raises += 1
                    say('m2 is too small, times 10 to ' + str(m2))
                    no_attack = attack_all = 0
        if not_changed:                                                   # AN:434-472
            if m1_list[0] < m1 - 1 and epoch == 0:
                m1_list[1] = m1
                m1 = int((m1 + m1_list[0]) / 2)
                say('m1 from ' + str(m1_list[0]) + ' to ' + str(m1_list[1]) + ', m1=' + str(m1))
                m2 = args_m2
                epoch = 0
            elif m1_list[0] < m1 and epoch == 0:
                m1_list[1] = m1
                m1 = m1_list[0]
                say('m1 from ' + str(m1_list[0]) + ' to ' + str(m1_list[1]) + ', m1=' + str(m1))
                m2 = args_m2
                epoch = 0
            else:
                epoch = epochs - 1
        elif epoch == epochs - 1:
            if m1 < m1_list[1] - 1:
                m1_list[0] = m1
                m1 = int((m1 + m1_list[1]) / 2)
                say('m1 from ' + str(m1_list[0]) + ' to ' + str(m1_list[1]) + ', m1=' + str(m1))
                m2 = args_m2
                epoch = 0
            elif m1 < m1_list[1]:
                m1_list[0] = m1
                m1 = m1_list[1]
                say('m1 from ' + str(m1_list[0]) + ' to ' + str(m1_list[1]) + ', m1=' + str(m1))
                m2 = args_m2
                epoch = 0
            else:
                epoch += 1
        else:
            epoch += 1
        d = stats.read(len(items), net._mm())                             # THE host read of the pass; AN:476-480
        attack_acc = d['attack_acc']
        _log_loss_acc(say, d)
        need_to_log['m1-' + str(m1) + ' epoch-' + str(epoch)] = 'time: {} Acc: {:.4f}'.format(time.time() - since, attack_acc)
        _log_epsilon(say, d)                                              # AN:487
        net.epsilon_3d_zero()
        if targeted:                                                      # AN:490-503
            take = (attack_acc >= best_acc and m1 == m1_best) or (m1 > m1_best and attack_acc > 0)
        else:
            take = (attack_acc <= best_acc and m1 == m1_best) or (m1 > m1_best and attack_acc < 1)
        if take:
            best_acc, m1_best, m2_best = attack_acc, m1, m2
            best = table.clone().detach()
        records.append(dict(d, m1=m1, m2=m2, m1_pass=pass_m1, epoch=pass_epoch, next_epoch=epoch, m2_raises=raises, taken=int(bool(take)),
                            **seen.fields()))
        _pass_done(n_pass, table)
        n_pass += 1
    return NerfailResult(best, table, m1_best, m2_best, best_acc, records, need_to_log)


# ---------------------------------------------------------------------------------------------- the product loop (IG:263-416)
def _igsm2d_batch_done(epoch, batch_index, table):
    """Called after every attack batch with the table as the step left it (the seam at which the tests record it)."""


def _frozen(model):
    """gauss_net._classifier_is_frozen's rule: every module in eval() mode and no parameter requiring grad."""
    if not isinstance(model, torch.nn.Module):
        return False
    return not any(m.training for m in model.modules()) and not any(p.requires_grad for p in model.parameters())


class _Store2D:
    """What igsm_2d and uap_2d (`caller`) set up alike in front of their loops: the resident uint8 store, the native gate, the
    classifier in eval() mode with frozen parameters (IG:266-272 / UA:244-250) and the clean images' logits, which then never
    change: they are computed at a view range's first use and kept for the run (else computed at every use, as the reference)."""

    def __init__(self, caller, model, model_name, images, native, dev):
        from .GaussNet import u2d_resize
        from .MyModel import MyCNN
        if isinstance(images, (list, tuple)):
            images = torch.stack([torch.as_tensor(v) for v in images])
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] not in (3, 4):
            raise ValueError('images must be a uint8 store [N,H,W,4] (BGRA) or [N,H,W,3]')
        self.images = images.to(dev).contiguous()
        self.N, self.H, self.W = self.images.shape[:3]
        if self.N < 1:
            raise ValueError('images holds no view')
        self.can_native = isinstance(model, MyCNN) and model_name == "my_model"
        if native and not self.can_native:
            raise ValueError('%s: native=True needs this package\'s MyCNN as `model` and model_name == "my_model"' % caller)
        if isinstance(model, torch.nn.Module):
            model.train(False)
            for p in model.parameters():
                p.requires_grad = False
        self.model, self.model_name, self.resize, self.frozen = model, model_name, u2d_resize, _frozen(model)
        self.zero_plane = torch.zeros((self.H, self.W, 3), dtype=torch.float32, device=dev)
        self.idx_all = torch.arange(self.N, dtype=torch.int64, device=dev)
        self.clean = {}

    def classify(self, cls_in):
        return self.model(self.resize(cls_in, self.model_name))

    def clean_logits(self, lo, hi):
        """The classifier's logits of the clean views lo..hi-1, float32 [hi - lo, C]."""
        if (lo, hi) in self.clean:
            return self.clean[lo, hi]
        with torch.no_grad():
            _, clean_in, _ = ops.u2d_fwd(self.images, self.idx_all[lo:hi], self.zero_plane, False, True, False)   # o + 0, clipped: o itself
            oc = _lib.f32c(self.classify(clean_in))
        if self.frozen:
            self.clean[lo, hi] = oc
        return oc

    def ori(self, v):
        """The clean view v on its white background, float32 [1,H,W,3]."""
        with torch.no_grad():
            return ops.u2d_fwd(self.images, self.idx_all[v:v + 1], self.zero_plane, True, False, False)[0]


def igsm_2d(model, model_name, images, label, epochs, a=2., epsilon=32., targeted=False, batch_size=4, on_export=None, log=print,
            native=None, export_sink=None):
    """The IGSM-2D baseline, attack_IGSM_2D.py:263-416 (= IG), as one call: the 2-D counterpart of nerfail_s.

    `model`, `model_name`: the victim classifier and the name that selects the resize in front of it (GaussNet.u2d_resize:
    none for "my_model", 224 for "vit_b_16", else 299). `images`: the views as ONE resident uint8 store [N,H,W,4] (BGRA as cv2
    reads an RGBA PNG; the white background of MD:247-255 is made on the device) or [N,H,W,3]; a list of such views is stacked
    once. `label`: the views' class, or the target class when `targeted`. The perturbation is a per-view table [N,H,W,3] that
    starts at zero (IG:250-252) and is clamped to +-epsilon around zero.

    Epochs 0 .. epochs-2 attack, over batches of `batch_size` views in store order (the last one short; IG:289 iterates the full
    dataloader in every epoch - the rand-select loader of IG:229 is built and never used). Per batch: nerfail_u2d_fwd (the
    attacked image, the classifier's planar input, the clip's pass mask), the classifier, the batch's statistics (CE and
    accuracy of the clean and of the attacked logits, the image loss MSE(x_rgb, ori), all of the table BEFORE this batch's
    update, IG:306-331), the gradient of the mean CE down to the classifier input (beta is the constant 0, IG:69: the image loss
    is a printed statistic only) and nerfail_u2d_step: clip backward, sign step, +-epsilon clamp and the write back into the
    batch's rows in one launch. nerfail_u2d_epoch_close turns the sums into the epoch's means (divided by the number of views,
    IG:392-400) and applies IG's STRICT rule (IG:407-416: a tie keeps the earlier epoch); nerfail_copy_if keeps the best table.
    Epoch epochs-1 is the export epoch (IG:286-301, 381-390): the BEST table, no gradient, the same statistics, and
    `on_export(batch_index, view_indices, adv_u8, mask_u8)` per batch with host uint8 arrays [B,H,W,3] of the attacked image
    and of the perturbation (negative values become 0, as cv2.imwrite saturates), converted by nerfail_export_u8. With
    epochs == 1 the zero table is exported. `export_sink`: an object with put(view_indices, x_rgb) - retrain.PoisonedTrainSet -
    that receives every export batch's attacked image [B,H,W,3] as a device tensor, before and independently of on_export; with
    on_export None no image is copied to the host. None (the default) leaves the loop as it is.

    The classifier. `native=None` (automatic) or True (insist): when `model` is this package's MyCNN and model_name is
    "my_model", a step is MyCNN.forward_masks (ops.cnn_fwd with its pool masks; the bf16x3 ops when the victim's precision is
    'bf16x3'), ops.cls_ce with a constant label vector for d loss / d logits, MyCNN.backward_data (ops.cnn_bwd_data[_x3]) and the
    step kernel - no autograd graph and no torch op between the launches. Any other classifier, or
    native=False: the classifier input requires grad, then the resize, the model and autograd.grad. Both paths take
    d loss / d logits of nn.CrossEntropyLoss() from ONE definition, ops.cls_ce ((softmax - onehot) / B, evaluated in double and
    rounded once): torch's float32 backward of the same loss differs from it in the last bits, which measured flipped the sign
    step of 103 of 5.3 million table elements between the two paths at 766 x 766; with one definition they agree bit for bit.
    Either way the logits are at most NERFAIL_ATTACK_MAX_CLASSES = 32 wide (the statistics' limit).

    As IG:266-272 does, a `model` that is an nn.Module is put in eval() mode and its parameters stop requiring grad. The clean
    images' logits never change then and are computed once per view for the run (else once per batch, as the reference).

    Host reads: one per epoch (the record, for the reference's four log lines, IG:402-405; log=None keeps the read and drops
    the lines), plus one wait per export batch. Returns an AttackResult: `best` and `last` are [N,H,W,3]."""
    epochs = _check_epochs(epochs)
    batch_size = int(batch_size)
    if not 1 <= batch_size <= 65535:
        raise ValueError('batch_size must be in 1..65535')
    dev = _cuda()
    store = _Store2D('igsm_2d', model, model_name, images, native, dev)                # IG:266-272
    images, idx_all, N, H, W = store.images, store.idx_all, store.N, store.H, store.W
    use_native = store.can_native and (native is None or bool(native))
    a, epsilon, targeted = float(a), float(epsilon), bool(targeted)
    label_i = int(label)
    lab32 = torch.full((batch_size,), label_i, dtype=torch.int32, device=dev)
    table = torch.zeros((N, H, W, 3), dtype=torch.float32, device=dev)     # IG:250; its init is the zero table: r_init = NULL
    best = torch.zeros_like(table)
    batches = [(lo, min(lo + batch_size, N)) for lo in range(0, N, batch_size)]
    stats = _EpochStats(epochs, targeted, label_i, dev, strict=True)       # IG:407-416
    ce_row = torch.zeros((_lib.ATTACK_ROW_FLOATS,), dtype=torch.float32, device=dev)   # ops.cls_ce's own sums: not read
    bufs = _ExportBuffers()
    records = []

    def batch_stats(epoch, lo, hi, cla, x_rgb):
        """IG:306-331 for one batch: five sums into the epoch's row, no host read."""
        _logit_stats(stats.lib, cla, store.clean_logits(lo, hi), label_i, stats.rows[epoch])
        ops.u2d_sqerr(x_rgb, images, idx_all[lo:hi], stats.scratch, stats.rows[epoch])

    def finish(epoch):
        records.append(_read_stats(stats.records[epoch]))                 # THE host read of the epoch
        _log_epoch(log, epoch, epochs, records[-1], 0.)                   # IG:402-405; beta is the constant 0, IG:69

    for epoch in range(epochs - 1):
        for bi, (lo, hi) in enumerate(batches):
            ib, B = idx_all[lo:hi], hi - lo
            with torch.no_grad():
                x_rgb, cls_in, mask = ops.u2d_fwd(images, ib, table, True, True, True)
            if use_native:
                with torch.no_grad():
                    cla, ws, pool = model.forward_masks(cls_in)
                    batch_stats(epoch, lo, hi, cla, x_rgb)
                    d_logits = ops.cls_ce(cla, lab32[:B], ce_row, True)                      # (softmax - onehot) / B
                    d_in = model.backward_data(ws, pool, d_logits, H, W)
            else:
                cls_in.requires_grad_()
                cla = store.classify(cls_in)
                batch_stats(epoch, lo, hi, cla.detach(), x_rgb)
                d_logits = ops.cls_ce(_lib.f32c(cla), lab32[:B], ce_row, True)              # CrossEntropyLoss()'s gradient, as above
                d_in = _lib.f32c(torch.autograd.grad(cla, cls_in, grad_outputs=d_logits.to(cla.dtype))[0])
            ops.u2d_step(table, ib, d_in, mask, None, a, epsilon, targeted)
            _igsm2d_batch_done(epoch, bi, table)
        stats.close(epoch)
        stats.keep_if_taken(table, best)
        finish(epoch)
    epoch = epochs - 1
    for bi, (lo, hi) in enumerate(batches):
        with torch.no_grad():
            x_rgb, cls_in, _ = ops.u2d_fwd(images, idx_all[lo:hi], best, True, True, False)
            cla = store.classify(cls_in)
            batch_stats(epoch, lo, hi, cla, x_rgb)
        if export_sink is not None:
            export_sink.put(list(range(lo, hi)), x_rgb)
        if on_export is not None:
            on_export(bi, list(range(lo, hi)), *bufs.to_host(x_rgb, best[lo:hi]))
    stats.close(epoch)                                                    # (its decision moves no tensor: the epoch ran on `best` itself)
    finish(epoch)
    return _attack_result(best, table, records, epochs)


# ---------------------------------------------------------------------------------------------- the product loop (UA:241-358)
class Uap2dResult:
    """What uap_2d returns. `best`: the table [H,W,3] the strict rule of UA:349-358 kept (device tensor) - the attack's result,
    what the export pass rendered; `last`: the table the loop ended on (from the export pass on the reference's table IS the best
    tensor, UA:269, so `last` then aliases it until the rule replaces `best` by a copy); `best_acc`: the attack accuracy recorded
    with `best` (0 / 10000 when the rule never fired); `stats`: one dict per PASS over the views (a pass is one turn of UA:241's
    while loop; `epoch` is the epoch it ran as, `next_epoch` where the loop went)."""

    def __init__(self, best, last, best_acc, stats):
        self.best, self.last, self.best_acc, self.stats = best, last, best_acc, stats


def _uap2d_pass_done(index, table):
    """Called at the end of every pass with the table as the pass left it (the seam at which the tests record it)."""


def uap_2d(model, model_name, images, label, epochs, epsilon=32., m1=8, m2=100, targeted=False, df_max_iter=1000, overshoot=0.02,
           num_classes=8, attack_views=None, export_views=None, on_export=None, log=print, native=None, export_sink=None):
    """The UAP-2D baseline, attack_UAP_2D.py:241-358 (= UA), as one call: the 2-D counterpart of nerfail.

    `model`, `model_name`, `images`, `label`: as for igsm_2d (the resident uint8 store [N,H,W,4|3]; the resize rule of
    GaussNet.u2d_resize). The perturbation is ONE table [H,W,3] that starts at zero (UA:219) and that every view shares
    (GN:359-363). `attack_views` / `export_views`: the view indices of an attack pass / of the export pass, or a callable of the
    pass number that returns them (the rand-select loader of UA:198); default: every view in store order. Batch size 1, as the
    reference fixes it.

    The loop is the reference's, quirks included. `while epoch < epochs` steps `epoch` itself. A pass before the last epoch
    visits every view: nerfail_u2d_fwd on the shared table, the classifier, the four running sums of UA:275-289 (in a device row)
    and - only when the raw argmax of the attacked logits still equals the clean one (UA:297-304) - DeepFool on the view
    (deepfool.deepfool_2d[_native], margins m1 / m2). When it finished before df_max_iter (UA:315-319) nerfail_uap2d_accumulate
    adds its perturbation and clamps the table to +-epsilon; a call that hits the cap changes nothing (there is no m2 rule and
    no m1 bisection here). A pass that changed nothing jumps to the last epoch, else the epoch advances (UA:335-338). The last
    epoch is the export pass (UA:262-270, 322-333): the BEST table, no gradient, over `export_views`, and
    `on_export(index, view_indices, adv_u8, mask_u8, ori_u8)` per view with host uint8 arrays [1,H,W,3] of the attacked image,
    [H,W,3] of the perturbation (negative values become 0, as cv2.imwrite saturates) and [1,H,W,3] of the clean image on its
    white background, converted by nerfail_export_u8. Every pass, the export pass included, ends with its means (sums / views of
    the pass) and the STRICT best rule of UA:349-358 (> targeted, < untargeted, from 0 / 10000). With epochs == 1 the zero table
    is exported. `export_sink`: as for igsm_2d - put([view_index], x_rgb [1,H,W,3]) per exported view, on the device, before and
    independently of on_export.

    The classifier. As UA:244-250 does, a `model` that is an nn.Module is put in eval() mode and its parameters stop requiring
    grad; the clean images' logits then never change and are computed once per view for the run (else at every visit).
    `native=None` (automatic) runs deepfool.deepfool_2d_native - with this package's MyCNN under "my_model" its class gradients
    come from ONE ops.cnn_bwd_data_multi, with any other classifier from autograd with respect to the classifier input;
    `native=True` insists on MyCNN; `native=False` runs the mirror deepfool.deepfool_2d through GaussNet.universal_2D_net.

    Host reads: one per visit for the skip decision, DeepFool's own (one per iteration), one per pass for the record and the
    reference's log lines (log=None keeps the read and drops the lines), one wait per exported view. An export pass without
    views is a ValueError (nothing would end the loop). The update is sequential over the views: there is nothing to shard, and
    more than one rank is a ValueError.

    Returns a Uap2dResult. Every dict of `stats` holds epoch, next_epoch, views, test_loss, test_acc, attack_loss, attack_acc,
    test_correct, attack_correct, skipped, attacked, completed, deepfool_iters, taken and `visits`: per visit (view index,
    skipped, iter_k, the chosen class of every iteration or None with the mirror)."""
    from . import deepfool as DF
    from .GaussNet import universal_2D_net
    epochs = _check_epochs(epochs)
    _check_one_rank('uap_2d updates one table')
    dev = _cuda()
    store = _Store2D('uap_2d', model, model_name, images, native, dev)                 # UA:244-250
    images, idx_all, N, H, W = store.images, store.idx_all, store.N, store.H, store.W
    _check_export_views('uap_2d', export_views)
    use_native = native is None or bool(native)
    net = universal_2D_net(dev, 0.02, model, model_name)
    epsilon, targeted, df_max_iter = float(epsilon), bool(targeted), int(df_max_iter)
    label_i = int(label)
    say = log if log is not None else (lambda *_: None)
    table = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)       # UA:219
    best = table.clone()
    best_acc = 0 if targeted else 10000                                   # UA:234-237
    bufs = _ExportBuffers()

    def views_of(src, n_pass):
        if src is None:
            return list(range(N))
        vs = [int(v) for v in (src(n_pass) if callable(src) else src)]
        if any(not 0 <= v < N for v in vs):
            raise ValueError('uap_2d: a view index is outside the store (0..%d)' % (N - 1))
        return vs

    records = []
    epoch, n_pass = 0, 0
    while epoch < epochs:
        say('Attack ...... [' + str(epoch) + '/' + str(epochs) + ']')
        not_changed = True
        export = epoch == epochs - 1
        items = views_of(export_views if export else attack_views, n_pass)
        if export:
            _check_export_views('uap_2d', items)
        stats, seen = _PassStats(label_i, dev), _Visits()
        pass_epoch = epoch
        for i, v in enumerate(items):
            if export and i == 0:
                table = best                                              # UA:269: the table IS the best tensor from here on
            with torch.no_grad():
                want_x = export and (on_export is not None or export_sink is not None)
                x_rgb, cls_in, _ = ops.u2d_fwd(images, idx_all[v:v + 1], table, want_x, True, False)
                cla = _lib.f32c(store.classify(cls_in))
            ori_cla = store.clean_logits(v, v + 1)
            stats.batch(epoch, cla, ori_cla)                              # UA:275-289
            if export:
                if export_sink is not None:
                    export_sink.put([v], x_rgb)
                if on_export is not None:
                    on_export(i, [v], *bufs.to_host(x_rgb, table, store.ori(v)))
                not_changed = False                                       # UA:333
                continue
            if not _same_class(cla, ori_cla):                             # UA:297-304
                seen.skip(v)
                continue
            kw = _deepfool_kw(num_classes, df_max_iter, label_i, targeted, overshoot, m1, m2)
            if use_native:
                _, iter_k, _, _, r_final, classes = DF.deepfool_2d_native((table, None), epsilon, net, images=images, view=v,
                                                                          clean_logits=ori_cla, **kw)
            else:
                _, iter_k, _, _, r_final = DF.deepfool_2d((table, store.ori(v)), epsilon, net, **kw)
                classes = None
            seen.ran(v, iter_k, classes)
            if iter_k < df_max_iter:                                      # UA:315-319
                say('iter_k < df_max_iter')
                ops.uap2d_accumulate(table, _lib.f32c(r_final), epsilon)
                not_changed = False
                seen.completed += 1
        if not_changed:                                                   # UA:335-338
            epoch = epochs - 1
        else:
            epoch += 1
        d = stats.read(len(items))                                        # THE host read of the pass; UA:340-344
        _log_loss_acc(say, d)
        take = d['attack_acc'] > best_acc if targeted else d['attack_acc'] < best_acc   # UA:349-358: strict
        if take:
            best_acc = d['attack_acc']
            best = table.clone().detach()
        records.append(dict(d, epoch=pass_epoch, next_epoch=epoch, taken=int(bool(take)), **seen.fields()))
        _uap2d_pass_done(n_pass, table)
        n_pass += 1
    return Uap2dResult(best, table, best_acc, records)
