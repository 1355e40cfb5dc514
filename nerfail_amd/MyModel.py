"""Native drop-in for the reference's victim classifier, `from model.MyModel import MyCNN` (model/MyModel.py:5-52).

Same submodules and parameter shapes, so a reference checkpoint (model/weights/my_model_<n>_best.pth) loads with
load_state_dict(strict=True): seven stages of 3x3 convolution + ReLU + 2x2 max-pool (3-32-64-128-256-256-128-64
channels), fc1 1024 -> 512 + ReLU, fc2 512 -> num_classes. The forward and the gradient with respect to the input run on
libnerfail_hip's cnn kernels (torch.ops.nerfail_mi.cnn_fwd).

Training is opt-in: MyCNN(num_classes, trainable=True). A default-constructed module is the frozen victim of the attack loops
(AS:281-287): its forward raises if a parameter requires grad under grad mode. With trainable=True such a forward keeps its
pool masks and the backward fills every parameter's .grad (and x.grad when x requires grad) from ONE pass of
torch.ops.nerfail_mi.cnn_bwd_weights: native HIP weight gradients without float atomics, bitwise reproducible; a parameter
with requires_grad=False gets None. model_train.py's loop (cross-entropy, SGD with momentum) runs on it unchanged. The weight
image is rebuilt when a parameter's version moves, so every optimizer.step() is followed by one repack (18 small launches) in
the next forward - unless the module was flattened: MyCNN.flatten_parameters() re-homes the 18 parameters as views of ONE
buffer in the layout the weight gradients arrive in (ops.cnn_grad_layout), and MyCNN.sgd_step() then is torch.optim.SGD's
momentum step and the update of the weight image in one launch (torch.ops.nerfail_mi.cnn_sgd_step): the next forward packs
nothing. nerfail_amd.model_train.train_classifier is the loop built on it. Under torch.no_grad(), with all parameters frozen, in input_gradients() and in DeepFool a trainable module
behaves exactly like a default one.

MyCNN.input_gradients(logits, d_logits) is the backward for several right-hand sides at once: the input gradients of R
rows d_logits [R,B,num_classes] of ONE forward in one launch chain (torch.ops.nerfail_mi.cnn_bwd_data_multi), each slice
bitwise what torch.autograd.grad through forward() gives for that row. DeepFool's inner loop takes the gradients of up to 8
class logits of one view this way (gauss_net.logit_gradients)."""
import ctypes

import torch
from torch import nn

from . import _lib
from . import ops
from ._images import ImageCache


class MyCNN(nn.Module):
    PRECISIONS = ('f32', 'bf16x3')

    def __init__(self, num_classes=24, trainable=False, precision='f32'):
        super().__init__()
        self.trainable = bool(trainable)
        self.precision = precision
        chans = (3, 32, 64, 128, 256, 256, 128, 64)
        for i in range(7):
            setattr(self, 'conv%d' % (i + 1), nn.Conv2d(chans[i], chans[i + 1], 3))
            setattr(self, 'max_pool%d' % (i + 1), nn.MaxPool2d(2))
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, num_classes)
        self.num_classes = num_classes
        self._images = ImageCache(self._params, {'packed': (self._pack, None), 'x3': (self._pack_x3, 'packed')})
        self._flat = None

    @property
    def precision(self):
        """'f32' (the exact kernels) or 'bf16x3' (conv stages 2..7 on bf16 MFMAs, f32-accurate). Assignable."""
        return self._precision

    @precision.setter
    def precision(self, value):
        if value not in self.PRECISIONS:
            raise ValueError('MyCNN: precision must be one of %s (got %r)' % (self.PRECISIONS, value))
        self._precision = value

    def _params(self):
        ps = []
        for i in range(7):
            c = getattr(self, 'conv%d' % (i + 1))
            ps += [c.weight, c.bias]
        return ps + [self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias]

    def _pack(self):
        lib = _lib.load()
        src = [_lib.f32c(p) for p in self._params()]
        for p in src:
            _lib.dev(p, 'MyCNN parameter')
        packed = torch.empty((lib.nerfail_cnn_packed_floats(self.num_classes),), dtype=torch.float32, device=src[0].device)
        ptrs = (ctypes.c_void_p * len(src))(*[p.data_ptr() for p in src])
        _lib.check(lib.nerfail_cnn_pack(ptrs, self.num_classes, _lib.dev(packed), _lib.stream()))
        return packed

    def packed(self):
        """The MFMA weight image (nerfail_cnn_pack), cached like NeRF's (_images.ImageCache): rebuilt when any parameter
        moves or is written in place."""
        return self._images.get('packed')

    def _pack_x3(self, packed):
        return ops.cnn_pack_x3(packed, self.num_classes)

    def packed_x3(self):
        """The bf16x3 image of stages 2..7 (nerfail_cnn_pack_x3), made from packed() and cached beside it: re-made exactly when
        packed() is (a parameter write or move), dropped by sgd_step()."""
        return self._images.get('x3')

    def _family(self, x3, images=None):
        """(forward op, backward op, multi backward op, leading weight-image arguments) of the exact family (x3 False) or the
        bf16x3 family (x3 True): the one place that tells the two apart. images: the ones a forward saved, instead of the
        module's current ones."""
        if x3:
            return ops.cnn_fwd_x3, ops.cnn_bwd_data_x3, ops.cnn_bwd_data_multi_x3, images or (self.packed(), self.packed_x3())
        return ops.cnn_fwd, ops.cnn_bwd_data, ops.cnn_bwd_data_multi, images or (self.packed(),)

    def forward_masks(self, x):
        """(logits, workspace, masks) of a forward that keeps its pool masks, in this module's precision, without an autograd
        graph: what the graph-free attack loops hand to backward_data()."""
        with torch.no_grad():
            fwd, _, _, images = self._family(self._precision == 'bf16x3')
            return fwd(*images, x, self.num_classes, True)

    def backward_data(self, workspace, masks, d_logits, H, W):
        """The input gradient from the buffers of forward_masks(), in this module's precision: d_logits [B,num_classes] ->
        [B,3,H,W] (one backward), d_logits [R,B,num_classes] -> [R,B,3,H,W] (the multi backward, slice r bitwise the single
        backward of row r)."""
        with torch.no_grad():
            _, single, multi, images = self._family(self._precision == 'bf16x3')
            return (multi if d_logits.dim() == 3 else single)(*images, workspace, masks, d_logits, H, W)

    def _is_flat(self):
        """True while every parameter still is the view of self._flat that flatten_parameters() made it (.to(), a deep copy
        or load_state_dict(assign=True) re-home parameters: the module then is an ordinary one again)."""
        flat = self._flat
        if flat is None:
            return False
        layout, _ = ops.cnn_grad_layout(self.num_classes)
        return all(p.data_ptr() == flat.data_ptr() + 4 * o and p.is_contiguous() and p.dtype == torch.float32
                   for (o, _), p in zip(layout, self._params()))

    def flatten_parameters(self):
        """Re-homes the 18 parameters as views of ONE float32 buffer in the layout of ops.cnn_grad_layout (the layout
        cnn_bwd_weights writes d_params in) and returns that buffer; the alignment floats between the regions are 0. The
        Parameter objects stay the same ones, so state_dict(), load_state_dict(), torch.save and an optimizer that already holds
        them keep working; .to() re-homes them as for any module, after which the module is no longer flat (call this again).
        A no-op, returning the same buffer, on a module that is flat. Trainable modules only."""
        if not self.trainable:
            raise RuntimeError('MyCNN.flatten_parameters: construct the module with trainable=True')
        if self._is_flat():
            return self._flat
        ps = self._params()
        layout, total = ops.cnn_grad_layout(self.num_classes)
        flat = torch.zeros((total,), dtype=torch.float32, device=ps[0].device)
        with torch.no_grad():
            for (o, sh), p in zip(layout, ps):
                view = flat[o:o + p.numel()].view(sh)
                view.copy_(p.detach())
                p.data = view
        self._flat = flat
        return flat

    def sgd_step(self, d_params, momentum_buf, lr, momentum, first):
        """One torch.optim.SGD(lr, momentum) step (dampening 0, no weight decay, no Nesterov) on the flat parameters from the
        flat gradient `d_params` of ops.cnn_bwd_weights, with `momentum_buf` (a flat float32 buffer the caller keeps; `first`
        says that it holds nothing yet). The same launch brings the weight image up to date, so the next forward packs
        nothing. No autograd graph, no host read."""
        if not self._is_flat():
            raise RuntimeError('MyCNN.sgd_step: the parameters are not flat (call flatten_parameters(); .to() un-flattens)')
        packed = self.packed()
        ops.cnn_sgd_step(self._flat, d_params, momentum_buf, packed, self.num_classes, float(lr), float(momentum), bool(first))
        for p in self._params():                     # the kernel wrote through the flat buffer: tell autograd and the caches
            torch.autograd.graph.increment_version(p)
        self._images.adopt('packed', packed)

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError('MyCNN: the input is on %s: nerfail_amd runs on the MI355X only (no CPU path)'
                               % (getattr(x, 'device', type(x)),))
        if x.dtype != torch.float32:
            raise TypeError('MyCNN: the input must be float32 (got %s)' % x.dtype)
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1:
            raise ValueError('MyCNN: the input must be [B,3,H,W] (got %s)' % (tuple(x.shape),))
        if not x.is_contiguous():
            raise ValueError('MyCNN: the input must be a contiguous NCHW tensor')
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if self._precision != 'f32':
                raise RuntimeError('MyCNN: the training path is exact f32 only - a forward that needs weight gradients cannot run '
                                   'with precision=%r; set precision=\'f32\', freeze the classifier (requires_grad_(False)) or '
                                   'run under torch.no_grad()' % (self._precision,))
            if self.trainable:
                return ops.CnnTrainFn.apply(self, x, *self._params())
            raise RuntimeError('MyCNN: weight gradients are not enabled on this module - construct it with trainable=True, freeze '
                               'the classifier (requires_grad_(False)) or run under torch.no_grad()')
        keep = torch.is_grad_enabled() and x.requires_grad
        fwd, _, _, images = self._family(self._precision == 'bf16x3')
        return fwd(*images, x, self.num_classes, keep)[0]

    def input_gradients(self, logits, d_logits):
        """d (sum(logits * d_logits[r])) / d x for every row r, [R,B,3,H,W], in ONE backward pass.

        `logits` is the tensor a grad-enabled forward(x) of this module returned (x requiring grad: the forward that keeps its
        pool masks), its graph still alive; `d_logits` is [R,B,num_classes]. The forward's workspace and masks are read off
        that tensor's autograd node: nothing is copied and nothing is kept alive here. Slice r is bitwise
        torch.autograd.grad(logits, x, d_logits[r], retain_graph=True)[0]."""
        saved = ops.cnn_fwd_saved(logits)
        if saved is None:
            raise RuntimeError('MyCNN.input_gradients: `logits` is not the output of a mask-keeping forward of a MyCNN (a '
                               'grad-enabled forward of an input that requires grad, its graph not yet freed)')
        packed, ws, masks, (H, W), packed_x3 = saved
        if not self._images.holds('packed', packed):
            raise RuntimeError('MyCNN.input_gradients: `logits` did not come from the last weight image of this module '
                               '(another module\'s forward, or the parameters were written and repacked since)')
        if not self._images.is_current('packed', packed):
            raise RuntimeError('MyCNN.input_gradients: a parameter was written or moved since the forward that returned '
                               '`logits`; run the forward again')
        if not isinstance(d_logits, torch.Tensor) or d_logits.dim() != 3 or tuple(d_logits.shape[1:]) != tuple(logits.shape):
            raise ValueError('MyCNN.input_gradients: d_logits must be [R,%d,%d] (got %s)'
                             % (logits.shape[0], logits.shape[1], tuple(getattr(d_logits, 'shape', ()))))
        if d_logits.shape[0] < 1:
            raise ValueError('MyCNN.input_gradients: d_logits holds no right-hand side (R = 0)')
        # the family that made `logits` and the images it saved, whatever self.precision is now
        saved_images = (packed,) if packed_x3 is None else (packed, packed_x3)
        _, _, multi, images = self._family(packed_x3 is not None, saved_images)
        return multi(*images, ws, masks, _lib.f32c(d_logits, logits.device), H, W)
