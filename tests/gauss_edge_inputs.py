"""Inputs that put the pixel <-> 3-D-point map's per-pixel decisions ON their boundaries (numpy only; shared by
tests/test_gauss_edge_inputs.py, which checks on the oracle that every class of decision is really reached, and by
tests/test_hip_gauss_edges.py, which compares every kernel copy of the chain with the oracle).

The exact map: every pixel has ONE neighbour slot with weight 1.0 (its position varies over 0..7) that points at a
perturbation row of its own; the other seven slots have weight 0 and random in-range indices. The sum over the slots is
sequential, nothing is contracted into an FMA and 0 * finite = 0, so x == s[row] and - one contribution with weight 1 per
row - grad_s[row] == the pixel's effective gradient: the clip / where / clip chain (GN:85-119) of every kernel copy shows up
undiluted and can be compared with the oracle for equality.
"""
import numpy as np

from oracle import gauss as OG

F32 = np.float32
EPS = 32.0
TINY = F32(2.0 ** -149)                    # the smallest positive float32: one float step above 0
STEP255 = F32(2.0 ** -16)                  # one float step below 255 (and, 255 + STEP255 being representable, above it)
UP, DOWN = F32(np.inf), F32(-np.inf)


def _na(v, to):
    return F32(np.nextafter(F32(v), F32(to)))


# x_3 of a pixel: alpha = x_3 / 255 = 1, 0.5, 0, -0, -1, a denormal
X3 = (255.0, 127.5, 0.0, -0.0, -255.0, 1e-40)
ALPHA_OF = {255.0: 1.0, 127.5: 0.5, -255.0: -1.0}        # the alphas that a delta can be divided by exactly
ORI_ALPHA_U8 = (0, 1, 254, 255)
ORI_ALPHA_FLOAT_ONLY = (-3.0, 300.0)

# (ori_c, delta): one colour channel of one pixel. delta = x_c * alpha against epsilon = 32 ...
DELTAS = (F32(32), _na(32, UP), _na(32, 0), F32(-32), _na(-32, DOWN), _na(-32, 0), F32(0), F32(31), F32(-31))
CHANNEL_CASES = [(F32(100), d) for d in DELTAS] + [
    # ... and pre = ori_c + delta against 0 and 255: exactly on, one unit beyond, one float step inside / beyond
    (F32(223), F32(32)), (F32(32), F32(-32)),            # pre == 255, pre == 0 (with delta ON +-epsilon)
    (F32(224), F32(32)), (F32(31), F32(-32)),            # 256, -1
    (F32(255), -STEP255), (F32(0), TINY),                # one float step inside
    (F32(255), STEP255), (F32(0), -TINY),                # one float step beyond
    (F32(255), F32(0)), (F32(0), F32(0)),                # on the bound with delta 0
    (F32(223), _na(32, UP)), (F32(32), _na(-32, DOWN)),  # epsilon None: rounds onto the bound; epsilon 32: blocked by the clip
    (F32(250), F32(31)), (F32(5), F32(-31)),             # far beyond, inside the epsilon clip
]
NCASE = len(CHANNEL_CASES)


def table_pixels(float_only_alpha=False):
    """One pixel per (x_3, channel case, ori alpha); channel c of the pixel takes case (i + 8 c) mod NCASE, so every channel
    meets every case. Returns x [n,4] (what the gather must produce) and ori [n,4] float32 (integers in 0..255 unless
    float_only_alpha, which uses the ori alphas a uint8 image cannot hold)."""
    xs, oris = [], []
    for x3 in X3:
        for oa in (ORI_ALPHA_FLOAT_ONLY if float_only_alpha else ORI_ALPHA_U8):
            for i in range(NCASE):
                x, o = np.zeros(4, F32), np.zeros(4, F32)
                for c in range(3):
                    oc, d = CHANNEL_CASES[(i + 8 * c) % NCASE]
                    a = ALPHA_OF.get(x3)
                    x[c] = d if a is None else F32(d / F32(a))    # exact: a is +-1 or 0.5
                    if a is not None:
                        assert F32(x[c] * F32(a)) == d
                    o[c] = oc
                x[3], o[3] = F32(x3), F32(oa)
                xs.append(x)
                oris.append(o)
    return np.array(xs, F32), np.array(oris, F32)


def exact_map(x_pixels, shape, seed=0, spare_rows=5, index_of_row=None):
    """The exact map for pixels whose gathered value must be x_pixels [n,4] (n = B*H*W of `shape`): returns
    (s [Ns,4], wi [B,2,H,W,8], row [n] int, slot [n] int). s[row[p]] = x_pixels[p]; the spare rows hold random finite values.
    index_of_row (optional): float32 index to WRITE into the live slot of each pixel instead of float(row) (for probing the
    float -> row conversion; `row` then says which row the rule resolves it to and s is laid out accordingly)."""
    B, H, W = shape
    n = B * H * W
    x_pixels = np.asarray(x_pixels, F32)
    assert x_pixels.shape == (n, 4)
    rs = np.random.RandomState(seed)
    Ns = n + spare_rows
    row = rs.permutation(Ns)[:n]
    s = rs.uniform(-40, 40, (Ns, 4)).astype(F32)
    s[row] = x_pixels
    slot = (np.arange(n) + rs.randint(0, 8)) % 8                  # varies over 0..7
    idx = rs.randint(0, Ns, (n, 8)).astype(F32)
    w = np.zeros((n, 8), F32)
    w[np.arange(n), slot] = 1.0
    idx[np.arange(n), slot] = row.astype(F32) if index_of_row is None else np.asarray(index_of_row, F32)
    wi = np.stack([w.reshape(B, H, W, 8), idx.reshape(B, H, W, 8)], 1)
    return s, wi, row, slot


def table_inputs(float_only_alpha=False, seed=0):
    """The table of cases on the exact map: dict with s, wi, ori (float32 [B,H,W,4]), ori_u8 (or None), row, shape, and
    seeded grad_x / grad_x_rgba."""
    x, ori = table_pixels(float_only_alpha)
    n = x.shape[0]
    shape = (2, n // (2 * NCASE), NCASE)                          # two views; P = n / 2 (no multiple of 256)
    assert shape[0] * shape[1] * shape[2] == n
    s, wi, row, slot = exact_map(x, shape, seed)
    rs = np.random.RandomState(seed + 1)
    ori = ori.reshape(shape + (4,))
    return dict(s=s, wi=wi, ori=ori, ori_u8=None if float_only_alpha else ori.astype(np.uint8), row=row, slot=slot, shape=shape,
                x=x.reshape(shape + (4,)),
                grad_x=rs.normal(size=shape + (4,)).astype(F32), grad_x_rgba=rs.normal(size=shape + (4,)).astype(F32))


# ---- the classes of decision a channel of a pixel can fall into (judged on the oracle's own float32 values)
CLASSES = ('ori_alpha', 'eps_low', 'eps_high', 'range_low', 'range_high', 'on_eps_low', 'on_eps_high', 'on_zero', 'on_255', 'interior')


def classify(x, ori, epsilon):
    """Class of every (pixel, channel): which gate blocks it (the first of ori alpha, epsilon clip, range clip), else on which
    bound it passes, else 'interior'. x, ori [..., 4] -> array of indices into CLASSES, [..., 3]."""
    x, ori = np.asarray(x, F32), np.asarray(ori, F32)
    alpha = x[..., 3:4] / F32(255)
    delta = x[..., :3] * alpha
    out = np.full(delta.shape, CLASSES.index('interior'))
    d = delta
    if epsilon is not None:
        e = F32(epsilon)
        d = np.clip(delta, -e, e)
    pre = ori[..., :3] + d
    # later assignments win: the order below is the reverse of the gates' priority
    out[pre == 0] = CLASSES.index('on_zero')
    out[pre == F32(255)] = CLASSES.index('on_255')
    if epsilon is not None:
        out[(delta == -e) & (pre >= 0) & (pre <= F32(255))] = CLASSES.index('on_eps_low')
        out[(delta == e) & (pre >= 0) & (pre <= F32(255))] = CLASSES.index('on_eps_high')
    out[pre < 0] = CLASSES.index('range_low')
    out[pre > F32(255)] = CLASSES.index('range_high')
    if epsilon is not None:
        out[delta < -e] = CLASSES.index('eps_low')
        out[delta > e] = CLASSES.index('eps_high')
    out[np.broadcast_to(~(ori[..., 3:4] > 0), out.shape)] = CLASSES.index('ori_alpha')
    return out


def passes(cls):
    return cls >= CLASSES.index('on_eps_low')


# ---- epsilon bookkeeping (GN:89-103): inputs with known extrema of where(alpha > 0, x_rgb, 0) * alpha
def bookkeeping_inputs(kind, B, seed=0, H=5, W=7):
    """Exact-map inputs whose bookkeeping extrema are attained at ONE known pixel each. kind: 'mixed' (min at -lo, max at +hi),
    'positive' (all deltas >= 0: the minimum stays 0), 'negative', 'small' (|delta| < 4), 'large' (extrema +-57.5 / 61.25).
    Pixels with alpha <= 0 carry huge rgb values that must NOT count. Returns dict(s, wi, ori, shape, emin, emax, at_min, at_max)."""
    rs = np.random.RandomState(seed)
    n = B * H * W
    lim = 3.0 if kind == 'small' else 20.0
    x = np.zeros((n, 4), F32)
    x[:, :3] = rs.uniform(-lim, lim, (n, 3)).astype(F32)
    x[:, 3] = rs.choice(np.array([255.0, 127.5, 63.75], F32), n)
    if kind == 'positive':
        x[:, :3] = np.abs(x[:, :3])
    if kind == 'negative':
        x[:, :3] = -np.abs(x[:, :3])
    dead = rs.uniform(size=n) < 0.25                              # alpha 0, -0, negative: rgb values do not count
    x[dead, :3] = rs.choice(np.array([-1e6, 1e6], F32), (int(dead.sum()), 3))
    x[dead, 3] = rs.choice(np.array([0.0, -0.0, -255.0, -1e-40], F32), int(dead.sum()))
    live = np.flatnonzero(~dead)
    at_max, at_min = int(live[len(live) // 3]), int(live[-2])             # (the maximum early, the minimum in the last view)
    hi, lo = (61.25, 57.5) if kind == 'large' else ((3.5, 3.25) if kind == 'small' else (30.5, 27.25))
    emax = emin = 0.0
    if kind != 'negative':
        x[at_max] = (1.0, 2 * hi, -1.0 if kind != 'positive' else 1.0, 127.5)    # delta = hi exactly, through alpha = 0.5
        emax = hi
    if kind != 'positive':
        x[at_min] = (-lo, 1.0 if kind != 'negative' else -1.0, 0.0, 255.0)
        emin = -lo
    s, wi, row, slot = exact_map(x, (B, H, W), seed + 7)
    ori = np.zeros((B, H, W, 4), F32)
    ori[..., :3] = rs.randint(0, 256, (B, H, W, 3))
    ori[..., 3] = rs.choice(np.array([0.0, 255.0], F32), (B, H, W))
    return dict(s=s, wi=wi, ori=ori, shape=(B, H, W), x=x.reshape(B, H, W, 4), emin=emin, emax=emax, at_min=at_min, at_max=at_max)


# ---- sign step (AS:352-392) at its boundaries
SIGN_GRADS = (0.0, -0.0, 1e-40, -1e-40, 1e-30, -1e-30, 3.0, -3.0)
SIGN_ROW_ALPHA = (255.0, 0.0, -1.0)
A, SIGN_EPS = 2.0, 32.0


def sign_step_rows(with_nan=False):
    """Rows (s, grad rgb, s_init) for the sign step with a = 2, epsilon = 32, s_init rgb = 0: every gradient of SIGN_GRADS
    (the denormals must step: sign is +-1 there) x row alpha x s such that s +- a lands exactly on s_init +- epsilon, one float
    step inside it and one beyond, on either side, plus an interior s. Channel c takes gradient (i + 3 c) mod 8.
    Returns s [n,4], grad [n,3], s_init [n,4]; with_nan appends rows whose gradient holds a NaN."""
    s_vals = [F32(30), _na(30, 0), _na(30, UP), F32(-30), _na(-30, 0), _na(-30, DOWN), F32(5), F32(-0.0), F32(34), F32(-34)]
    rows_s, rows_g = [], []
    for ra in SIGN_ROW_ALPHA:
        for sv in s_vals:
            for i in range(len(SIGN_GRADS)):
                rows_s.append([sv, sv, -sv, ra])
                rows_g.append([SIGN_GRADS[(i + 3 * c) % len(SIGN_GRADS)] for c in range(3)])
    if with_nan:
        for ra in SIGN_ROW_ALPHA:
            rows_s.append([30.0, -7.0, 5.0, ra])
            rows_g.append([np.nan, 3.0, np.nan])
    s = np.array(rows_s, F32)
    s_init = np.zeros_like(s)
    s_init[:, 3] = s[:, 3]
    return s, np.array(rows_g, F32), s_init


# ---- float -> row conversion: one rule everywhere (clamp as a float to [0, Ns-1], NaN -> 0, then truncate)
def probe_indices(Ns):
    return np.array([-1.0, -0.5, -0.0, 0.5, Ns - 1, Ns - 0.5, Ns, Ns + 0.5, 3e9, 1e20, np.inf, -np.inf, np.nan], F32)


def expected_row(fi, Ns):
    """The documented rule, in float64 on the float32 value: NaN -> 0; clamp to [0, Ns-1]; truncate."""
    fi = np.asarray(fi, F32).astype(np.float64)
    fi = np.where(np.isnan(fi), 0.0, fi)
    return np.trunc(np.clip(fi, 0.0, float(Ns - 1))).astype(np.int64)
