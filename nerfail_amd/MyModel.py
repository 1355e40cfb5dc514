"""Native drop-in for the reference's victim classifier, `from model.MyModel import MyCNN` (model/MyModel.py:5-52).

Same submodules and parameter shapes, so a reference checkpoint (model/weights/my_model_<n>_best.pth) loads with
load_state_dict(strict=True): seven stages of 3x3 convolution + ReLU + 2x2 max-pool (3-32-64-128-256-256-128-64
channels), fc1 1024 -> 512 + ReLU, fc2 512 -> num_classes. The forward and the gradient with respect to the input run on
libnerfail_hip's cnn kernels (torch.ops.nerfail_mi.cnn_fwd). Weight gradients (training the classifier) are not
implemented: the attack loops freeze it (AS:281-287), and forward raises if a parameter requires grad under grad mode."""
import ctypes

import torch
from torch import nn

from . import _lib
from . import ops


class MyCNN(nn.Module):
    def __init__(self, num_classes=24):
        super().__init__()
        chans = (3, 32, 64, 128, 256, 256, 128, 64)
        for i in range(7):
            setattr(self, 'conv%d' % (i + 1), nn.Conv2d(chans[i], chans[i + 1], 3))
            setattr(self, 'max_pool%d' % (i + 1), nn.MaxPool2d(2))
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, num_classes)
        self.num_classes = num_classes
        self._packed = None
        self._packed_key = None

    def _params(self):
        ps = []
        for i in range(7):
            c = getattr(self, 'conv%d' % (i + 1))
            ps += [c.weight, c.bias]
        return ps + [self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias]

    def packed(self):
        """The MFMA weight image (nerfail_cnn_pack), rebuilt when any parameter moves or is written in place."""
        ps = self._params()
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if self._packed is None or key != self._packed_key:
            dev = ps[0].device
            lib = _lib.load()
            src = [_lib.f32c(p) for p in ps]
            for p in src:
                _lib.dev(p, 'MyCNN parameter')
            packed = torch.empty((lib.nerfail_cnn_packed_floats(self.num_classes),), dtype=torch.float32, device=dev)
            ptrs = (ctypes.c_void_p * len(src))(*[p.data_ptr() for p in src])
            _lib.check(lib.nerfail_cnn_pack(ptrs, self.num_classes, _lib.dev(packed), _lib.stream()))
            self._packed, self._packed_key = packed, key
        return self._packed

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
            raise RuntimeError('MyCNN: weight gradients are not implemented - freeze the classifier (requires_grad_(False)) '
                               'or run under torch.no_grad()')
        keep = torch.is_grad_enabled() and x.requires_grad
        logits, _, _ = ops.cnn_fwd(self.packed(), x, self.num_classes, keep)
        return logits
