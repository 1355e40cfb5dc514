"""numpy model of the folded bf16x3 weight image (nerfail_mlp_pack_x3f, mlp_x3.hip): the composition rule of the views
layer and the image bytes. Shared by tests/test_x3_fold_ref.py (CPU) and tests/test_hip_mlp_x3_fold.py (-m gpu)."""
import numpy as np

W = 256


def compose64(sd):
    """Wc = Wv[:, :W] Wf and bc = Wv[:, :W] bf + bv in double, BEFORE the one rounding to f32: the sum over m = 0, 1, ..., W-1
    in this order from 0 (a product of two f32 values is exact in double), bv added last."""
    wv = sd['views_linears.0.weight'].astype(np.float32).astype(np.float64)
    wf = sd['feature_linear.weight'].astype(np.float32).astype(np.float64)
    bf = sd['feature_linear.bias'].astype(np.float32).astype(np.float64)
    bv = sd['views_linears.0.bias'].astype(np.float32).astype(np.float64)
    wc = np.zeros((wv.shape[0], W), np.float64)
    bc = np.zeros((wv.shape[0],), np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        for m in range(W):
            wc += wv[:, m:m + 1] * wf[m:m + 1, :]
            bc += wv[:, m] * bf[m]
        bc += bv
    return wc, bc


def compose(sd):
    """The composed block as the image holds it: rounded once to f32."""
    wc, bc = compose64(sd)
    with np.errstate(over='ignore'):
        return wc.astype(np.float32), bc.astype(np.float32)


def folded_f64_forward(sd, D, skips, x, wc, bc):
    """RH:100-123 in float64 on an embedded batch x [M, 90] with feature_linear folded into the views layer (wc, bc)."""
    p = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    x = np.asarray(x, np.float64)
    inp, views = x[:, :63], x[:, 63:]
    h = inp
    for i in range(D):
        h = np.maximum(h @ p['pts_linears.%d.weight' % i].T + p['pts_linears.%d.bias' % i], 0.)
        if i in skips:
            h = np.concatenate([inp, h], -1)
    alpha = h @ p['alpha_linear.weight'].T + p['alpha_linear.bias']
    h2 = np.maximum(h @ np.asarray(wc, np.float64).T + views @ p['views_linears.0.weight'][:, W:].T + np.asarray(bc, np.float64), 0.)
    rgb = h2 @ p['rgb_linear.weight'].T + p['rgb_linear.bias']
    return np.concatenate([rgb, alpha], -1), h


def stream_tile_steps(D, skip):
    """Tile-steps (12 MFMAs each) of the folded and of the unfolded stream: layer 0, the skip re-entry, D-1 hidden layers
    (+ feature_linear when unfolded), the views layer (8 + 1 k32 steps x 8 out tiles)."""
    folded = 32 + (32 if 0 <= skip < D - 1 else 0) + (D - 1) * 128 + 72
    return folded, folded + 128


def bias_index(c):
    """Position of channel c in a bias piece of the f32 image ([32-row tile][lane half][16], mlp_layout.h load_bias)."""
    c = np.asarray(c)
    return 32 * (c >> 5) + 16 * ((c >> 2) & 1) + (c & 3) + 4 * ((c & 31) >> 3)
