"""The classifier-input resize (include/nerfail_hip.h "classifier-input resize (resize revision 1)") in numpy: the one definition the
kernels of nerfail_amd/csrc/resize.hip are compared against, bit for bit.

  axis_table(n_in, n_out)      the tables, in Python floats (float64), weights rounded once to float32; the inverted ranges are
                               asserted contiguous and covering
  matrix64(n_in, n_out)        the axis as a dense float64 matrix [n_out, n_in] (weights NOT rounded): aten's
                               _upsample_bilinear2d_aa, align_corners=False
  forward64 / adjoint64        the two passes with those matrices
  source_values(src, layout)   layout 0: [B,H,W,4] -> [B,3,H,W] with v = a > 0 ? c : 255; layout 1: as it is
  forward32(src, layout, oh, ow)            fixed-order float32: every product and every sum rounded on its own
  adjoint32(g, src, layout, H, W)           the same for g [R,B,3,oh,ow] -> [R,B,H,W,4] (layout 0) or [R,B,3,H,W] (layout 1)
"""
import numpy as np

MAX_TAPS = 16


def _span(scale, support, n_in, i):
    c = scale * (i + 0.5)
    start = max(0, int(c - support + 0.5))
    count = min(n_in, int(c + support + 0.5)) - start
    return c, start, count


def _weights64(n_in, n_out):
    """Per output: (start, [float64 weights])."""
    scale = n_in / n_out
    support = scale if scale >= 1 else 1.0
    inv = 1 / scale if scale >= 1 else 1.0
    rows = []
    for i in range(n_out):
        c, start, count = _span(scale, support, n_in, i)
        w = [max(0.0, 1 - abs((k + start - c + 0.5) * inv)) for k in range(count)]
        total = 0.0
        for v in w:
            total += v
        rows.append((start, [v / total for v in w]))
    return rows


def axis_table(n_in, n_out):
    """dict(start, count int32 [n_out]; w float32 [n_out, kmax]; ostart, ocount int32 [n_in]; kmax; refused). `refused`: a count
    or an inverted count above MAX_TAPS (what nerfail_resize_aa_table answers NERFAIL_EINVAL for)."""
    assert n_in >= 1 and n_out >= 1
    rows = _weights64(n_in, n_out)
    start = np.array([r[0] for r in rows], np.int32)
    count = np.array([len(r[1]) for r in rows], np.int32)
    kmax = int(count.max())
    w = np.zeros((n_out, kmax), np.float32)
    for i, (_, wk) in enumerate(rows):
        w[i, :len(wk)] = np.array(wk, np.float64).astype(np.float32)
    ostart = np.full(n_in, -1, np.int32)
    ocount = np.zeros(n_in, np.int32)
    for i in range(n_out):
        for j in range(start[i], start[i] + count[i]):
            if ocount[j] == 0:
                ostart[j] = i
            assert ostart[j] + ocount[j] == i, 'the outputs that read input %d are not contiguous' % j
            ocount[j] += 1
    assert (ocount >= 1).all(), 'an input is read by no output'
    return dict(start=start, count=count, w=w, ostart=ostart, ocount=ocount, kmax=kmax,
                refused=bool(kmax > MAX_TAPS or ocount.max() > MAX_TAPS))


def matrix64(n_in, n_out):
    m = np.zeros((n_out, n_in), np.float64)
    for i, (start, wk) in enumerate(_weights64(n_in, n_out)):
        m[i, start:start + len(wk)] = wk
    return m


def source_values(src, layout):
    src = np.asarray(src)
    if layout == 1:
        return src
    with np.errstate(invalid='ignore'):
        on = src[..., 3:4] > 0
    return np.ascontiguousarray(np.moveaxis(np.where(on, src[..., :3], src.dtype.type(255)), -1, 1))


def forward64(v, oh, ow):
    """v [B,3,H,W] (any float type) -> float64 [B,3,oh,ow]."""
    v = np.asarray(v, np.float64)
    my, mx = matrix64(v.shape[-2], oh), matrix64(v.shape[-1], ow)
    return np.matmul(np.matmul(my, v), mx.T)


def adjoint64(g, H, W):
    """g [...,3,oh,ow] -> float64 [...,3,H,W]."""
    g = np.asarray(g, np.float64)
    my, mx = matrix64(H, g.shape[-2]), matrix64(W, g.shape[-1])
    return np.matmul(np.matmul(my.T, g), mx)


def _pass32(v, tab):
    """One forward pass along the LAST axis of float32 v: out[..., o] = w[o][0] * v[..., s] (+ w[o][k] * v[..., s + k] in order)."""
    start, count, w = tab['start'].astype(np.int64), tab['count'], tab['w']
    n_in = v.shape[-1]
    with np.errstate(invalid='ignore', over='ignore'):
        acc = w[:, 0] * v[..., start]
        for k in range(1, tab['kmax']):
            live = k < count
            term = w[:, k] * v[..., np.minimum(start + k, n_in - 1)]
            acc = np.where(live, acc + term, acc)
    assert acc.dtype == np.float32
    return acc


def _adjoint_pass32(g, tab):
    """One adjoint pass along the LAST axis of float32 g [..., n_out] -> [..., n_in]: sum over the outputs of the inverted range,
    ascending, the first product starting the sum."""
    start, w, kmax = tab['start'].astype(np.int64), tab['w'], tab['kmax']
    ostart, ocount = tab['ostart'].astype(np.int64), tab['ocount']
    n_in, n_out = len(ostart), len(start)
    j = np.arange(n_in)
    acc = None
    with np.errstate(invalid='ignore', over='ignore'):
        for q in range(int(ocount.max())):
            o = np.minimum(ostart + q, n_out - 1)
            k = j - start[o]
            wq = np.where((k >= 0) & (k < kmax), w[o, np.clip(k, 0, kmax - 1)], np.float32(0))
            term = wq * g[..., o]
            acc = term if q == 0 else np.where(q < ocount, acc + term, acc)
    assert acc.dtype == np.float32
    return acc


def forward32(src, layout, oh, ow):
    """float32 [B,3,oh,ow]: horizontal pass, then vertical pass."""
    v = np.asarray(source_values(np.asarray(src, np.float32), layout), np.float32)
    H, W = v.shape[-2:]
    t = _pass32(v, axis_table(W, ow))                                                   # [B,3,H,ow]
    return np.ascontiguousarray(np.swapaxes(_pass32(np.swapaxes(t, -1, -2), axis_table(H, oh)), -1, -2))


def adjoint32(g, src, layout, H, W):
    """g float32 [R,B,3,oh,ow] -> layout 0: [R,B,H,W,4] (rgb a > 0 ? gx : +0, alpha 0; src [B,H,W,4]), layout 1: [R,B,3,H,W]."""
    g = np.asarray(g, np.float32)
    oh, ow = g.shape[-2:]
    tmp = np.swapaxes(_adjoint_pass32(np.swapaxes(g, -1, -2), axis_table(H, oh)), -1, -2)     # [R,B,3,H,ow]
    gx = _adjoint_pass32(np.ascontiguousarray(tmp), axis_table(W, ow))                        # [R,B,3,H,W]
    if layout == 1:
        return np.ascontiguousarray(gx)
    with np.errstate(invalid='ignore'):
        on = np.asarray(src)[None, ..., 3:4] > 0                                              # [1,B,H,W,1]
    out = np.zeros(g.shape[:2] + (H, W, 4), np.float32)
    out[..., :3] = np.where(on, np.moveaxis(gx, 2, -1), np.float32(0))
    return out
