"""The resize in front of the torchvision classifiers (GN:145-157, MD:110-113, MT:283-290), shared by gauss_net's cold tail and
model_test: torchvision if present (as the reference), else the same bilinear op in torch."""
import torch


def resize(x, size):
    try:
        from torchvision.transforms import Resize
        return Resize([size, size])(x)
    except ImportError:
        return torch.nn.functional.interpolate(x, size=(size, size), mode='bilinear', align_corners=False,
                                               antialias=True)


# ---------------------------------------------------------------------------------- the native stage (csrc/resize.hip, resize revision 1)
# White background, NHWC -> NCHW and the antialiased resize as one kernel with an exact adjoint: fixed-order float32 arithmetic
# (include/nerfail_hip.h "classifier-input resize"; tests/resize_ref.py), no float atomics, the same bits on every run. resize()
# above is unchanged and stays the default everywhere.
_AXIS_TABLES = {}


class AxisTables:
    """One axis' tables on the device and the struct nerfail_resize_axis over them."""

    def __init__(self, n_in, n_out, device):
        import ctypes
        from . import _lib
        lib = _lib.load()
        kmax = max(1, lib.nerfail_resize_aa_kmax(n_in, n_out))
        ints = torch.zeros(2 * max(n_out, 0) + 2 * max(n_in, 0), dtype=torch.int32)
        w = torch.zeros((max(n_out, 0), kmax), dtype=torch.float32)
        p = ints.data_ptr()
        _lib.check(lib.nerfail_resize_aa_table(n_in, n_out, p, p + 4 * n_out, w.data_ptr(), kmax, p + 8 * n_out, p + 8 * n_out + 4 * n_in))
        self.n_in, self.n_out, self.kmax = n_in, n_out, kmax
        self.host_ints, self.host_w = ints, w
        self.ints, self.w = ints.to(device), w.to(device)
        d = self.ints.data_ptr()
        st = _lib.ResizeAxisStruct()
        st.start, st.count, st.w, st.ostart, st.ocount = d, d + 4 * n_out, self.w.data_ptr(), d + 8 * n_out, d + 8 * n_out + 4 * n_in
        st.n_in, st.n_out, st.kmax = n_in, n_out, kmax
        self.struct = st
        self.ref = ctypes.byref(st)


def axis_tables(n_in, n_out, device):
    """The tables of n_in -> n_out on `device`, built once by nerfail_resize_aa_table; raises _lib.NerfailError on its refusals
    (more than 16 taps on either side)."""
    device = torch.device(device)
    key = (int(n_in), int(n_out), device.type, device.index if device.index is not None else torch.cuda.current_device())
    t = _AXIS_TABLES.get(key)
    if t is None:
        t = _AXIS_TABLES[key] = AxisTables(int(n_in), int(n_out), device)
    return t


def _pair(size):
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


def _native_input(x, name, last):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 4 \
            or x.shape[last] != (4 if last == 3 else 3):
        raise ValueError('%s takes a contiguous float32 device tensor %s' % (name, '[B,H,W,4]' if last == 3 else '[B,3,H,W]'))


class ClassifierInputResize(torch.autograd.Function):
    """nerfail_cls_input_resize_fwd / _bwd: torch.ops.nerfail_mi.cls_input_resize with the context and the backward that op
    registers for itself (ops._resize_setup / ops._resize_backward) - one body for both."""

    @staticmethod
    def forward(ctx, src, layout, oh, ow):
        from . import ops
        ops._resize_setup(ctx, (src, layout, oh, ow), None)
        return ops.cls_input_resize(src, layout, oh, ow)

    @staticmethod
    def backward(ctx, g):
        from . import ops
        return ops._resize_backward(ctx, g)


def classifier_input(x_rgba, size):
    """x_rgba float32 [B,H,W,4] -> the classifier input [B,3,size,size]: white where alpha > 0 is false, planar, resized."""
    _native_input(x_rgba, 'classifier_input', 3)
    oh, ow = _pair(size)
    return ClassifierInputResize.apply(x_rgba, 0, oh, ow)


def resize_native(x, size):
    """resize() for a planar float32 [B,3,H,W] device tensor, by the native kernel. Anything else raises."""
    _native_input(x, 'resize_native', 1)
    oh, ow = _pair(size)
    return ClassifierInputResize.apply(x, 1, oh, ow)
