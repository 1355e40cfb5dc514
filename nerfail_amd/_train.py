"""Autograd wiring of the training step (run_nerf.py:776-791): render_rays as ONE torch.autograd.Function whose
forward runs the fused HIP pipeline (saving activations in register-fragment layout) and whose backward runs
nerfail_composite_bwd -> nerfail_mlp_bwd_data -> nerfail_mlp_bwd_weights for the fine and the coarse pass.

Gradients flow to the parameters of network_fn / network_fine only: rays are data and z_samples is detached
(RN:394), exactly the graph the reference's loss.backward() sees."""
import torch

from . import _lib
from .run_nerf_helpers import mlp_forward


# The weight images live in the network's one cache (NeRF._images, rules in _images.py); these are its training-side names.
def ordered_params(net):
    """Parameters in the fixed order used for Function.apply / grads: pts_linears (w, b)*D, views, feature, alpha, rgb."""
    return net.ordered_params()


def _grads_struct(net, tensors):
    """nerfail_mlp_params over `tensors` (ordered_params order), used as they are: the buffers the gradients are written to."""
    return _lib.mlp_params(net.D, net.W, net.input_ch, net.input_ch_views, net._skip(), tensors, None)


def packed_T(net):
    """Transposed weight image for the backward-data pass (nerfail_mlp_pack_T)."""
    return net._images.get('f32_T')


def packed_both(net):
    """Forward and transposed weight images of `net` from ONE launch (nerfail_mlp_pack_train); afterwards NeRF.packed() and
    packed_T() are hits: the training loop re-packs both after every optimizer step."""
    return net.packed_both()


def packed_f16_T(net):
    """fp16 hi/lo image of the transposed weights (split-precision backward-data, nerfail_mlp_pack_f16_T)."""
    return net._images.get('f16_T')


def acts_floats(net, M):
    return _lib.load().nerfail_mlp_train_acts_floats(net.D, net.W, M)


def dz_floats(net, M):
    return _lib.load().nerfail_mlp_train_dz_floats(net.D, net.W, M)


def _train_buffers(net, R, N, acts, device):
    """(raw, acts) of a training forward of R * N samples; `acts` given: checked, else a fresh buffer."""
    if acts is None:
        acts = torch.empty((acts_floats(net, R * N),), dtype=torch.float32, device=device)
    elif acts.numel() != acts_floats(net, R * N):
        raise ValueError('acts buffer has %d floats, the pass needs %d' % (acts.numel(), acts_floats(net, R * N)))
    return torch.empty((R, N, 4), dtype=torch.float32, device=device), acts


def mlp_fwd_train(net, pts, viewdirs, acts=None):
    """Forward that saves the activations; `acts`: where (a slice of a buffer shared by the coarse and the fine pass, so
    that ONE backward launch can walk both), else a fresh buffer. precision 'f16x3': the split-precision forward, same
    saved activations, and no joint f32 pack (its backward-data pass reads the fp16 transposed image)."""
    raw, acts = _train_buffers(net, pts.shape[0], pts.shape[1], acts, pts.device)
    return mlp_forward(net, raw, pts=pts, viewdirs=viewdirs, acts=acts), acts


def mlp_fwd_train_rays(net, rays, z_vals, acts=None):
    """mlp_fwd_train with the sample points formed inside the kernel (nerfail_mlp_fwd_rays): rays [R,11], z_vals [R,N]."""
    raw, acts = _train_buffers(net, z_vals.shape[0], z_vals.shape[1], acts, z_vals.device)
    return mlp_forward(net, raw, rays=rays, z_vals=z_vals, acts=acts), acts


def _same_arch(a, b):
    return (a.D, a.W, a._skip(), getattr(a, 'precision', 'f32')) == (b.D, b.W, b._skip(), getattr(b, 'precision', 'f32'))


def dw_scratch(net, M0, M1, flags, device):
    n = _lib.load().nerfail_mlp_bwd_weights_scratch_bytes(net.D, net.W, net._skip(), M0, M1, flags)
    return torch.empty((max(n, 1),), dtype=torch.uint8, device=device), n


def mlp_backward(net, d_raw, acts, grads, accumulate=True):
    """d loss / d params of ONE network into `grads` (list of tensors in ordered_params order; += when `accumulate`)."""
    mlp_backward2(net, d_raw.reshape(-1, 4), acts, grads, d_raw.shape[0] * d_raw.shape[1], None, None, 0, accumulate)


def mlp_backward2(net0, d_raw, acts, grads0, M0, net1, grads1, M1, accumulate=False):
    """Backward-data + weight gradients of one or TWO networks of the same architecture in ONE launch each: d_raw [M0+M1,4],
    acts hold network 0's tiles then network 1's. The W = 256 weight-gradient kernel is deterministic (no atomics)."""
    lib = _lib.load()
    M = M0 + M1
    split = getattr(net0, 'precision', 'f32') == 'f16x3'
    dz = torch.empty((dz_floats(net0, M0) + (dz_floats(net1, M1) if M1 else 0),), dtype=torch.float32, device=d_raw.device)
    st = _lib.stream()
    if split:
        off_a = off_z = off_r = 0
        for net, Mi in ((net0, M0), (net1, M1)):
            if Mi == 0:
                continue
            _lib.check(lib.nerfail_mlp_bwd_data_f16(_lib.dev(net.packed()), _lib.dev(packed_f16_T(net)), net.D, net.W, net._skip(),
                                                    _lib.dev(d_raw[off_r:off_r + Mi]), _lib.dev(acts[off_a:off_a + acts_floats(net, Mi)]), Mi,
                                                    _lib.dev(dz[off_z:off_z + dz_floats(net, Mi)]), st))
            off_a, off_z, off_r = off_a + acts_floats(net, Mi), off_z + dz_floats(net, Mi), off_r + Mi
    else:
        p0, pT0 = packed_both(net0)
        p1, pT1 = packed_both(net1) if M1 else (None, None)
        _lib.check(lib.nerfail_mlp_bwd_data2(_lib.dev(p0), _lib.dev(pT0), M0, _lib.dev(p1), _lib.dev(pT1), M1, net0.D, net0.W,
                                             net0._skip(), _lib.dev(d_raw), _lib.dev(acts), _lib.dev(dz), st))
    flags = (_lib.DW_BF16X3 if split else 0) | (_lib.DW_ACCUMULATE if accumulate else 0)
    scratch, nbytes = dw_scratch(net0, M0, M1, flags, d_raw.device)
    _lib.check(lib.nerfail_mlp_bwd_weights(net0.D, net0.W, net0._skip(), _lib.dev(acts), _lib.dev(dz), M0, _grads_struct(net0, grads0),
                                           M1, _grads_struct(net1, grads1) if M1 else None, flags, _lib.dev(scratch), nbytes, st))


def composite_backward(raw, z_vals, rays, noise, white_bkgd, g_rgb, g_disp, g_acc, g_depth=None, g_weights=None, out=None):
    R, N = z_vals.shape
    d_raw = torch.empty((R, N, 4), dtype=torch.float32, device=raw.device) if out is None else out.view(R, N, 4)

    def c(t):
        return None if t is None else _lib.f32c(t)
    g_rgb, g_disp, g_acc, g_depth, g_weights = c(g_rgb), c(g_disp), c(g_acc), c(g_depth), c(g_weights)
    _lib.check(_lib.load().nerfail_composite_bwd(_lib.dev(raw), _lib.dev(z_vals), _lib.dev(rays), _lib.dev(noise), R, N,
                                                 int(bool(white_bkgd)), _lib.dev(g_rgb), _lib.dev(g_disp), _lib.dev(g_acc),
                                                 _lib.dev(g_depth), _lib.dev(g_weights), _lib.dev(d_raw), _lib.stream()))
    return d_raw


def _new_grads(net, zero):
    """One flat buffer per network, sliced into per-parameter views (`zero`: one memset; the W = 256 weight-gradient
    kernel OVERWRITES its outputs, so the training step needs none)."""
    ps = ordered_params(net)
    n = sum(p.numel() for p in ps)
    flat = (torch.zeros if zero else torch.empty)((n,), dtype=torch.float32, device=ps[0].device)
    out, off = [], 0
    for p in ps:
        out.append(flat[off:off + p.numel()].view(p.shape))
        off += p.numel()
    return out


def _zero_grads(net):
    return _new_grads(net, True)


def arena_layout(shapes_per_net):
    """Layout of the gradient arena from parameter shapes alone: ([[offset of every parameter] per network], P). The
    parameters of the networks follow each other in ordered_params order, densely; P = their total numel is the index of
    the two tail floats (loss, mse)."""
    offsets, off = [], 0
    for shapes in shapes_per_net:
        offs = []
        for shape in shapes:
            n = 1
            for d in shape:
                n *= int(d)
            offs.append(off)
            off += n
        offsets.append(offs)
    return offsets, off


class GradArena:
    """The one gradient buffer of a data-parallel training run: float32 [coarse params | fine params | loss, mse].
    RenderRaysTrain.backward writes the parameter gradients straight into it (through fresh per-parameter views, which
    autograd adopts as p.grad), the step's loss and fine image loss go into the tail, ONE all-reduce sums all of it over the
    ranks, and optimizer.step() reads the p.grad that still alias it: no gather before the collective, no scatter after."""

    def __init__(self, nets, device=None):
        self.nets = [n for n in nets if n is not None]
        self.shapes = [[tuple(p.shape) for p in ordered_params(n)] for n in self.nets]
        self.offsets, self.P = arena_layout(self.shapes)
        if device is None:
            device = ordered_params(self.nets[0])[0].device
        self.buf = torch.zeros((self.P + 2,), dtype=torch.float32, device=device)
        self.ends = [offs[0] for offs in self.offsets[1:]] + [self.P]

    @property
    def nbytes(self):
        return self.buf.numel() * self.buf.element_size()

    def _index(self, net):
        for k, n in enumerate(self.nets):
            if n is net:
                return k
        raise ValueError('GradArena: the network is not one of the arena\'s')

    def views(self, net, zero=False):
        """Fresh views of `net`'s range, one per parameter in ordered_params order (`zero`: one memset of the range first)."""
        k = self._index(net)
        if zero:
            self.buf[self.offsets[k][0]:self.ends[k]].zero_()
        out = []
        for off, shape in zip(self.offsets[k], self.shapes[k]):
            n = 1
            for d in shape:
                n *= d
            out.append(self.buf[off:off + n].view(shape))
        return out

    def zero_(self):
        self.buf.zero_()

    def holds(self, t):
        """Does tensor `t` lie inside the arena's memory?"""
        lo = self.buf.data_ptr()
        return t is not None and lo <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= lo + 4 * self.P

    def adopt(self):
        """Make every p.grad alias the arena: gradients autograd placed elsewhere (a step of several render chunks, whose
        backward passes it accumulates out of place) are copied in; a parameter without a gradient (an idle rank, which ran
        no backward) gets the view as it is. After a single-chunk backward this finds nothing to do."""
        with torch.no_grad():
            for net in self.nets:
                views = None
                for i, p in enumerate(ordered_params(net)):
                    if self.holds(p.grad):
                        continue
                    views = self.views(net) if views is None else views
                    if p.grad is not None:
                        views[i].copy_(p.grad)
                    p.grad = views[i]

    def put_tail(self, loss, mse):
        torch.stack((loss.detach(), mse.detach()), out=self.buf[self.P:])

    @property
    def loss(self):
        return self.buf[self.P]

    @property
    def mse(self):
        return self.buf[self.P + 1]

    def reduce_(self, group=None, timing=None):
        """THE collective of a step: one all-reduce (sum) of the whole arena, P + 2 floats. `timing`: a dict that gets HIP
        events around it ('allreduce_events': (start, end, bytes), recorded by sharding.all_reduce_sum_)."""
        from . import sharding
        return sharding.all_reduce_sum_(self.buf, group, timing)


class RenderRaysTrain(torch.autograd.Function):
    """forward(rays, cfg, *params) -> (rgb_map, disp_map, acc_map, rgb0, disp0, acc0, z_std, pts_max, raw)."""

    @staticmethod
    def forward(ctx, rays, cfg, *params):
        out = cfg['pipeline'](rays, train=True)
        ctx.cfg = cfg
        ctx.saved = out['_saved']
        ctx.mark_non_differentiable(out['z_std'], out['pts_max'])
        ctx.set_materialize_grads(False)          # unused outputs arrive as None, not as freshly filled zero tensors
        return (out['rgb_map'], out['disp_map'], out['acc_map'], out['rgb0'], out['disp0'], out['acc0'], out['z_std'],
                out['pts_max'], out['raw'])

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_rgb0, g_disp0, g_acc0, g_zstd, g_ptsmax, g_raw):
        cfg, sv = ctx.cfg, ctx.saved
        coarse, fine = cfg['network_fn'], cfg['network_fine']
        arena = cfg.get('grad_arena')

        def _grads(net, zero):                     # where this pass writes d loss / d params of `net`
            return _new_grads(net, zero) if arena is None else arena.views(net, zero)
        nets = [coarse] + ([fine] if fine is not None else [])
        wb = cfg['white_bkgd']
        c, f = sv['coarse'], sv['fine']
        Mc = c['z'].shape[0] * c['z'].shape[1]
        if f is None:
            d_raw = composite_backward(c['raw'], c['z'], sv['rays'], c['noise'], wb, g_rgb, g_disp, g_acc)
            if g_raw is not None and cfg['retraw']:
                d_raw = d_raw + g_raw
            grads = {id(coarse): _grads(coarse, False)}
            mlp_backward2(coarse, d_raw.reshape(-1, 4), c['acts'], grads[id(coarse)], Mc, None, None, 0)
        else:
            run = fine if fine is not None else coarse
            Mf = f['z'].shape[0] * f['z'].shape[1]
            joint = sv.get('acts_all') is not None and Mc % 32 == 0 and _same_arch(coarse, run)
            d_all = torch.empty((Mc + Mf, 4), dtype=torch.float32, device=c['raw'].device)
            composite_backward(c['raw'], c['z'], sv['rays'], c['noise'], wb, g_rgb0, g_disp0, g_acc0, out=d_all[:Mc])
            composite_backward(f['raw'], f['z'], sv['rays'], f['noise'], wb, g_rgb, g_disp, g_acc, out=d_all[Mc:])
            if g_raw is not None and cfg['retraw']:
                d_all[Mc:] += g_raw.reshape(-1, 4)
            grads = {id(n): _grads(n, not joint) for n in nets}
            if joint and run is coarse:            # one network evaluated twice (network_fine=None): one run of Mc + Mf samples
                mlp_backward2(coarse, d_all, sv['acts_all'], grads[id(coarse)], Mc + Mf, None, None, 0)
            elif joint:                            # coarse + fine in ONE launch each (independent: RN:394 detaches z_samples)
                mlp_backward2(coarse, d_all, sv['acts_all'], grads[id(coarse)], Mc, run, grads[id(run)], Mf)
            else:
                mlp_backward2(run, d_all[Mc:], f['acts'], grads[id(run)], Mf, None, None, 0, accumulate=True)
                mlp_backward2(coarse, d_all[:Mc], c['acts'], grads[id(coarse)], Mc, None, None, 0, accumulate=True)
        flat = []
        for n in nets:
            flat += grads[id(n)]
        return (None, None) + tuple(flat)
