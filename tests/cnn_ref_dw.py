"""Float64 (or `dtype`) reference of the MyCNN WEIGHT gradients (nerfail_cnn_bwd_weights) with the pool routing as an input,
built on the steps of cnn_ref.chain_backward, and the codec of that entry point's d_params and scratch buffers
(include/nerfail_hip.h, ABI 11). tests/test_cnn_dw_ref.py pins it to ATen on the CPU; tests/test_hip_cnn_dw.py judges the
kernels with it. torch / numpy only, no GPU."""
import numpy as np
import torch

import cnn_inputs as CI
import cnn_ref as R


def names(num_classes=24):
    return [n for n, _ in CI.param_shapes(num_classes)]


# ---------------------------------------------------------------------------------------------------------------- buffers
def grad_layout(num_classes):
    """([(name, offset, shape)], total floats) of d_params: state-dict order, every region starting on a multiple of 4."""
    out, o = [], 0
    for name, shape in CI.param_shapes(num_classes):
        out.append((name, o, shape))
        o += (int(np.prod(shape)) + 3) // 4 * 4
    return out, o


def split_grads(d_params, num_classes):
    """({name: array}, defined mask) of a flat d_params buffer."""
    d_params = np.asarray(d_params).reshape(-1)
    lay, total = grad_layout(num_classes)
    assert d_params.size == total, (d_params.size, total)
    defined = np.zeros(total, bool)
    out = {}
    for name, o, shape in lay:
        n = int(np.prod(shape))
        out[name] = d_params[o:o + n].reshape(shape)
        defined[o:o + n] = True
    return out, defined


def split_scratch(scratch, B, H, W):
    """(pooled, d_hidden, floats used) of the entry's scratch: pooled[s] the [B, hp, wp, Cout] (NHWC) gradient with respect
    to stage s's pooled output, d_hidden [B, 512]; the partial slabs behind them are unspecified."""
    scratch = np.asarray(scratch).reshape(-1)
    pooled, o = [], 0
    for s, (_, _, hp, wp) in enumerate(R.stage_dims(H, W)):
        n = B * hp * wp * R.CHANS[s + 1]
        pooled.append(scratch[o:o + n].reshape(B, hp, wp, R.CHANS[s + 1]))
        o += (n + 3) // 4 * 4
    dh = scratch[o:o + B * R.HIDDEN].reshape(B, R.HIDDEN)
    return pooled, dh, o + B * R.HIDDEN


# ---------------------------------------------------------------------------------------------------------------- steps
def unpool(g, act, code, hin, win, dtype):
    """The un-pooled gated gradient on the (hin - 2) x (win - 2) conv grid: g [B, C, hp, wp] goes to window position `code`
    unless act <= 0 (NaN passes); rows and columns the floor pool dropped stay 0. cnn_ref.chain_backward's two steps."""
    g = R._t(g, dtype)
    hp, wp = g.shape[-2:]
    g = torch.where(torch.from_numpy(np.asarray(act) <= 0), torch.zeros((), dtype=dtype), g)
    c = torch.from_numpy(np.asarray(code).astype(np.int64))
    up = torch.zeros((g.shape[0], g.shape[1], hin - 2, win - 2), dtype=dtype)
    for q in range(4):
        up[:, :, (q >> 1):2 * hp:2, (q & 1):2 * wp:2] = torch.where(c == q, g, torch.zeros((), dtype=dtype))
    return up


def conv_dw(up, x):
    """dW[co, ci, ky, kx] = sum over b, y, x of up[b, co, y, x] x[b, ci, y + ky, x + kx], one matrix product per tap."""
    co, ci = up.shape[1], x.shape[1]
    h, w = up.shape[-2:]
    upf = up.permute(1, 0, 2, 3).reshape(co, -1)
    dw = torch.zeros((co, ci, 3, 3), dtype=up.dtype)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = upf @ x[:, :, ky:ky + h, kx:kx + w].permute(1, 0, 2, 3).reshape(ci, -1).T
    return dw


def fc1_columns(x7_nchw):
    """[B, 1024] in PyTorch's flatten order c * 16 + y * 4 + x of the [B, 64, 4, 4] stage-7 output."""
    return x7_nchw.reshape(x7_nchw.shape[0], -1)


def chain_dw(params, x, acts, codes, hidden, d_logits, dtype, hw):
    """All 18 parameter gradients, every stage's pooled gradient and d_x of the network with its routing given (arguments as
    cnn_ref.chain_backward, plus the input x [B, 3, H, W]; acts[s] are the stage outputs in NCHW, whose VALUES are the next
    stage's input here). Returns ({name: numpy}, [pooled gradient s NCHW], d_hidden, d_x) in `dtype`."""
    from torch.nn import functional as F
    dims = R.stage_dims(*hw)
    grads = {}
    dl, hid = R._t(d_logits, dtype), R._t(hidden, dtype)
    grads['fc2.weight'] = dl.T @ hid
    grads['fc2.bias'] = dl.sum(0)
    g = dl @ R._t(params['fc2.weight'], dtype)
    dh = torch.where(torch.from_numpy(np.asarray(hidden) <= 0), torch.zeros((), dtype=dtype), g)
    grads['fc1.weight'] = dh.T @ fc1_columns(R._t(acts[6], dtype))
    grads['fc1.bias'] = dh.sum(0)
    g = (dh @ R._t(params['fc1.weight'], dtype)).reshape(-1, 64, 4, 4)
    pooled = [None] * R.STAGES
    for s in range(R.STAGES - 1, -1, -1):
        hin, win, hp, wp = dims[s]
        pooled[s] = g.numpy()
        up = unpool(g, acts[s], codes[s], hin, win, dtype)
        xin = R._t(x if s == 0 else acts[s - 1], dtype)
        grads['conv%d.weight' % (s + 1)] = conv_dw(up, xin)
        grads['conv%d.bias' % (s + 1)] = up.sum((0, 2, 3))
        g = F.conv_transpose2d(up, R._t(params['conv%d.weight' % (s + 1)], dtype))
    return {k: v.numpy() for k, v in grads.items()}, pooled, dh.numpy(), g.numpy()
