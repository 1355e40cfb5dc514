"""Float64 references of the MyCNN kernels (nerfail_amd/csrc/cnn.hip) with the pool routing as an INPUT, and the codec of
the buffers the kernels publish (include/nerfail_hip.h, "buffer contract"): tests/test_hip_cnn_stages.py holds every stage
to f32 rounding level with them, tests/test_cnn_ref.py pins them to ATen on the CPU. torch / numpy only, no GPU.

Stage s = 0..6 is the module's conv(s+1): 3x3 valid convolution + bias + ReLU + 2x2 floor max-pool."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

import cnn_inputs as CI

CHANS = CI.CHANS
STAGES = 7
HIDDEN = 512
FLAT = 1024
U = 2.0 ** -24          # f32 unit roundoff
TINY = 2.0 ** -126      # smallest normal f32: what a flushed subnormal product or sum can lose

# (H, W, B) of the stage tests; tests/test_cnn_ref.py asserts size_coverage(SIZES) from stage_dims. The height and width chains are
# independent, so six heights and six widths are paired up; 800 x 800, 766 x 893 and 893 x 766 are the extremes and the
# attack's own size.
SIZES = ((800, 800, 1), (766, 893, 3), (893, 766, 1), (767, 767, 1), (769, 772, 3), (783, 785, 1))


# ---------------------------------------------------------------------------------------------------------------- geometry
def stage_dims(H, W):
    """[(hin, win, hp, wp)] of the seven stages, None when the seventh stage's pooled output is not 4 x 4."""
    out, h, w = [], int(H), int(W)
    for _ in range(STAGES):
        if h < 4 or w < 4:
            return None
        hp, wp = (h - 2) // 2, (w - 2) // 2
        out.append((h, w, hp, wp))
        h, w = hp, wp
    return out if (h, w) == (4, 4) else None


def size_coverage(sizes):
    """{condition: met} over the (H, W, ...) list: every residue at which a tile, a mask byte or the floor pool has an edge
    case (stage numbers in the keys are 1-based, as in cnn.hip's kernel names)."""
    dims = [stage_dims(s[0], s[1]) for s in sizes]
    assert all(d is not None for d in dims), sizes
    cov = {}
    for ax, name in ((0, 'hin'), (1, 'win')):
        for par, pn in ((1, 'odd'), (0, 'even')):               # a conv row / column the floor pool drops, or none
            cov['%s-2 %s at stage 1' % (name, pn)] = any((d[0][ax] - 2) % 2 == par for d in dims)
            cov['%s-2 %s at a stage >= 2' % (name, pn)] = any((st[ax] - 2) % 2 == par for d in dims for st in d[1:])
    for ax, name in ((2, 'hp'), (3, 'wp')):                     # forward tiles: 8 x 8 pooled cells
        for r in (0, 1, 7):
            cov['%s mod 8 == %d' % (name, r)] = any(st[ax] % 8 == r for d in dims for st in d)
    for r in (0, 1, 7):                                         # backward tiles: 8 rows x 32 columns of stage input
        cov['hin mod 8 == %d at a stage >= 2' % r] = any(st[0] % 8 == r for d in dims for st in d[1:])
    for r in (0, 1, 31):
        cov['win mod 32 == %d at a stage >= 2' % r] = any(st[1] % 32 == r for d in dims for st in d[1:])
    for r in (0, 1, 15):                                        # stage-1 backward tiles: 16 x 16
        cov['H mod 16 == %d' % r] = any(d[0][0] % 16 == r for d in dims)
        cov['W mod 16 == %d' % r] = any(d[0][1] % 16 == r for d in dims)
    for r in (1, 2):                                            # a mask byte whose cells are partly padding
        cov['wp mod 8 == %d (mask rows)' % r] = any(st[3] % 8 == r for d in dims for st in d)
    return cov


# ---------------------------------------------------------------------------------------------------------------- buffers
def workspace_floats(B, H, W):
    return sum(B * hp * wp * CHANS[s + 1] for s, (_, _, hp, wp) in enumerate(stage_dims(H, W))) + B * HIDDEN


def mask_bytes(B, H, W):
    return sum(B * hp * ((wp + 7) // 8) * 2 * CHANS[s + 1] for s, (_, _, hp, wp) in enumerate(stage_dims(H, W)))


def split_workspace(ws, B, H, W):
    """(acts, hidden) of the flat workspace: acts[s] the [B, hp, wp, Cout] (NHWC) view of stage s, hidden [B, 512]."""
    ws = np.asarray(ws).reshape(-1)
    assert ws.size == workspace_floats(B, H, W), (ws.size, workspace_floats(B, H, W))
    acts, o = [], 0
    for s, (_, _, hp, wp) in enumerate(stage_dims(H, W)):
        n = B * hp * wp * CHANS[s + 1]
        acts.append(ws[o:o + n].reshape(B, hp, wp, CHANS[s + 1]))
        o += n
    return acts, ws[o:].reshape(B, HIDDEN)


def nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


def decode_masks(masks, B, H, W):
    """Per stage the [B, Cout, hp, wp] window positions 2 dy + dx (0..3) of the mask image."""
    masks = np.asarray(masks, np.uint8).reshape(-1)
    assert masks.size == mask_bytes(B, H, W), (masks.size, mask_bytes(B, H, W))
    out, o = [], 0
    for s, (_, _, hp, wp) in enumerate(stage_dims(H, W)):
        C, n8 = CHANS[s + 1], (wp + 7) // 8
        m = masks[o:o + B * hp * n8 * 2 * C].reshape(B, hp, n8, 2, C)
        o += m.size
        pc = np.arange(wp)
        by = m[:, :, pc >> 3, pc & 1, :]                                     # [B, hp, wp, C]
        sh = (2 * ((pc & 7) >> 1)).astype(np.uint8)
        out.append(np.ascontiguousarray(np.transpose((by >> sh[None, None, :, None]) & 3, (0, 3, 1, 2))))
    return out


def encode_masks(codes):
    """The mask image of per-stage [B, Cout, hp, wp] codes; the cells of a byte beyond wp are 0."""
    parts = []
    for c in codes:
        c = np.asarray(c)
        assert c.min() >= 0 and c.max() <= 3
        B, C, hp, wp = c.shape
        n8 = (wp + 7) // 8
        pad = np.zeros((B, hp, n8 * 8, C), np.uint8)
        pad[:, :, :wp, :] = np.transpose(c, (0, 2, 3, 1))
        cell = pad.reshape(B, hp, n8, 4, 2, C)                               # column pc = 8 byte-pair + 2 g + h
        by = np.zeros((B, hp, n8, 2, C), np.uint8)
        for g in range(4):
            by |= cell[:, :, :, g] << np.uint8(2 * g)
        parts.append(by.reshape(-1))
    return np.concatenate(parts)


def codes_from_indices(idx, conv_w):
    """Window positions from F.max_pool2d(..., 2, return_indices=True) on a conv grid conv_w columns wide."""
    idx = np.asarray(idx)
    hp, wp = idx.shape[-2:]
    y, x = idx // conv_w, idx % conv_w
    dy = y - 2 * np.arange(hp)[:, None]
    dx = x - 2 * np.arange(wp)[None, :]
    assert dy.min() >= 0 and dy.max() <= 1 and dx.min() >= 0 and dx.max() <= 1
    return (2 * dy + dx).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- weight image
def pack_image(sd, C):
    """(image, defined): the packed weight image of nerfail_cnn_pack rebuilt from a state dict, and which of its floats the
    contract defines (the round-up of a region to 4 floats is not)."""
    regions = []
    for s in range(STAGES):
        w, b = np.asarray(sd['conv%d.weight' % (s + 1)], np.float32), np.asarray(sd['conv%d.bias' % (s + 1)], np.float32)
        co, ci = w.shape[:2]
        w9 = w.reshape(co, ci, 9)
        if s == 0:                                              # [Cout][10 taps][4 channels], the padding exactly 0
            f = np.zeros((co, 10, 4), np.float32)
            f[:, :9, :3] = np.transpose(w9, (0, 2, 1))
        else:                                                   # [Cout][tap][Cin]
            f = np.transpose(w9, (0, 2, 1))
        regions += [f, b]
        if s > 0:
            regions.append(np.transpose(w9, (1, 2, 0)))         # backward: [Cin][tap][Cout]
    regions.append(np.asarray(sd['conv1.weight'], np.float32))  # raw stage-1 copy [32][3][9]
    w1 = np.asarray(sd['fc1.weight'], np.float32).reshape(HIDDEN, 64, 16)      # columns c * 16 + yx
    fc1P = np.transpose(w1, (0, 2, 1)).reshape(HIDDEN, FLAT)    # columns yx * 64 + c (NHWC)
    regions += [fc1P.T, fc1P, np.asarray(sd['fc1.bias'], np.float32), np.asarray(sd['fc2.weight'], np.float32),
                np.asarray(sd['fc2.bias'], np.float32)]
    assert regions[-2].shape == (C, HIDDEN)
    img, defined = [], []
    for r in regions:
        r = np.ascontiguousarray(r, np.float32).reshape(-1)
        padn = (-r.size) % 4
        img += [r, np.zeros(padn, np.float32)]
        defined += [np.ones(r.size, bool), np.zeros(padn, bool)]
    return np.concatenate(img), np.concatenate(defined)


# ---------------------------------------------------------------------------------------------------------------- forward
StageRef = collections.namedtuple('StageRef', 'pre pooled mag conv')


def _t(a, dtype=torch.float64):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def stage_forward64(x_nchw, w, b):
    """One stage in float64 on its f32 input: pre = relu(conv + bias) before the pool, pooled = its 2x2 floor max-pool
    (NaN wins), mag = conv(|x|, |w|) + |b|, what the rounding bounds scale with; conv = pre before the ReLU."""
    x, w, b = _t(x_nchw), _t(w), _t(b)
    conv = F.conv2d(x, w, b)
    pre = F.relu(conv)
    return StageRef(pre, F.max_pool2d(pre, 2), F.conv2d(x.abs(), w.abs()) + b.abs()[None, :, None, None], conv)


def linear64(x, w, b):
    """(x w^T + b, |x| |w|^T + |b|) in float64."""
    x, w, b = _t(x), _t(w), _t(b)
    return x @ w.T + b, x.abs() @ w.abs().T + b.abs()


def elem_bound(K, mag):
    """Worst-case rounding error of a length-K f32 dot product plus bias, in any summation order."""
    return (K + 2) * U * mag + K * TINY


def l2_bound(K, mag):
    """Probabilistic (Higham & Mary) bound on the L2 norm of those errors over a whole tensor."""
    return float(np.sqrt(K + 2) * U * np.linalg.norm(np.asarray(mag, np.float64).reshape(-1)))


def forward64(sd, x):
    """The whole network in float64 with the routing ATen chooses: (logits, acts NCHW, codes, hidden), as numpy."""
    h = _t(x)
    acts, codes = [], []
    for s in range(STAGES):
        pre = F.relu(F.conv2d(h, _t(sd['conv%d.weight' % (s + 1)]), _t(sd['conv%d.bias' % (s + 1)])))
        h, idx = F.max_pool2d(pre, 2, return_indices=True)
        acts.append(h.numpy())
        codes.append(codes_from_indices(idx.numpy(), pre.shape[-1]))
    hidden = F.relu(F.linear(h.reshape(h.shape[0], -1), _t(sd['fc1.weight']), _t(sd['fc1.bias'])))
    return F.linear(hidden, _t(sd['fc2.weight']), _t(sd['fc2.bias'])).numpy(), acts, codes, hidden.numpy()


# ---------------------------------------------------------------------------------------------------------------- backward
def chain_backward(params, acts, codes, hidden, d_logits, dtype, hw):
    """d loss / d x [B, 3, H, W] (numpy, `dtype`) of the network with its routing given: acts[s] [B, C, hp, wp] the pooled
    outputs (only their sign and NaN-ness are used), codes[s] the window positions, hidden [B, 512]. fc2^T, the gate
    hidden <= 0 -> 0, fc1^T, then for s = 6..0: the gate acts[s] <= 0 -> 0 (NaN passes), the scatter to position codes[s] on
    the (hin - 2) x (win - 2) conv grid (rows / columns the floor pool dropped stay 0), conv_transpose2d with the stage's
    weights. Every step is linear in d_logits; in float32 this is the stock-fp32 yardstick of the same routing."""
    dims = stage_dims(*hw)
    g = _t(d_logits, dtype) @ _t(params['fc2.weight'], dtype)
    g = torch.where(torch.from_numpy(np.asarray(hidden) <= 0), torch.zeros((), dtype=dtype), g)
    g = (g @ _t(params['fc1.weight'], dtype)).reshape(-1, 64, 4, 4)
    for s in range(STAGES - 1, -1, -1):
        hin, win, hp, wp = dims[s]
        a, c = np.asarray(acts[s]), torch.from_numpy(np.asarray(codes[s]).astype(np.int64))
        assert a.shape == tuple(g.shape) == tuple(c.shape) == (g.shape[0], CHANS[s + 1], hp, wp)
        g = torch.where(torch.from_numpy(a <= 0), torch.zeros((), dtype=dtype), g)
        up = torch.zeros((g.shape[0], CHANS[s + 1], hin - 2, win - 2), dtype=dtype)
        for q in range(4):
            up[:, :, (q >> 1):2 * hp:2, (q & 1):2 * wp:2] = torch.where(c == q, g, torch.zeros((), dtype=dtype))
        g = F.conv_transpose2d(up, _t(params['conv%d.weight' % (s + 1)], dtype))
    return g.numpy()


# ---------------------------------------------------------------------------------------------------------------- inputs
def noise_image(seed, H, W, amp=255.0):
    """[3, H, W] float32 uniform in [-amp, amp): no two conv pixels of a pool window see related operands (no ties)."""
    return np.random.RandomState(seed).uniform(-amp, amp, size=(3, H, W)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- argmax rules
def _windows(a, hp, wp):
    """[4, ...] the four positions 2 dy + dx of every pool window of a [B, C, h, w] conv-grid array."""
    a = np.asarray(a)
    return np.stack([a[:, :, (q >> 1):2 * hp:2, (q & 1):2 * wp:2] for q in range(4)])


def judge_codes(codes, ref, t):
    """Counts of windows that break a rule a correct f32 forward cannot break, given the float64 stage `ref` (StageRef of the
    same input) and t = twice the per-element rounding bound: 'not_max' the coded value is more than t below the window's
    maximum (or not NaN where the window has one); 'wrong_clear' the runner-up is more than t below the maximum and the
    code is not float64's argmax; 'wrong_zero' all four values before the ReLU are below -t (an exact four-way tie at 0 in
    any precision: the first position wins) and the code is not 0. 'undecided': windows neither clearly ordered nor clearly
    all zero, where the rules only ask for a maximum up to rounding."""
    codes = np.asarray(codes).astype(np.int64)
    hp, wp = codes.shape[-2:]
    v, c = _windows(ref.pre.numpy(), hp, wp), _windows(ref.conv.numpy(), hp, wp)
    t = np.asarray(t, np.float64)
    has_nan = np.isnan(v).any(0)
    vj = np.take_along_axis(v, codes[None], 0)[0]
    with np.errstate(invalid='ignore'):
        vs = np.sort(v, 0)
        vmax = vs[3]
        clear = ~has_nan & (vs[2] < vmax - t)
        allneg = ~has_nan & (c < -t).all(0)
        not_max = np.where(has_nan, ~np.isnan(vj), vj < vmax - t)
    return {'windows': int(codes.size), 'not_max': int(not_max.sum()),
            'wrong_clear': int((clear & (codes != np.argmax(np.where(np.isnan(v), -np.inf, v), 0))).sum()),
            'wrong_zero': int((allneg & (codes != 0)).sum()), 'undecided': int((~clear & ~allneg & ~has_nan).sum())}
