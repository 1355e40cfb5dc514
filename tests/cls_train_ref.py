"""Numpy restatement of the victim-training entry points (include/nerfail_hip.h, section "victim training"): what
nerfail_cls_batch, nerfail_cls_ce, nerfail_cnn_sgd_step and nerfail_cls_epoch_close compute, and the bookkeeping of
nerfail_amd.model_train.train_classifier around them - written from the header's definitions and model_train.py:89-193
(MTR), MyDataset.py:93-105 (MD), not from the kernels. tests/test_cls_train_ref.py holds it to torch's CPU kernels and to
fixture g26 (the reference's own run); tests/test_hip_cls_*.py hold the kernels to it."""
import math

import numpy as np

ROW = 16                                      # NERFAIL_ATTACK_ROW_FLOATS
MAX_CLASSES = 32
F32 = np.float32


# ---------------------------------------------------------------------------------------------- 1a: nerfail_cls_batch
def batch(images, labels_all, idx):
    """(x float32 [B,3,P], labels int32 [B]) of a uint8 store [N,P,4|3]: rgb where alpha > 0, else 255 (MD:98-105), planar,
    channel order as stored; an index outside 0..N-1 gives a view of NaN and the label -1."""
    images = np.asarray(images)
    N, P, ch = images.shape
    x = np.empty((len(idx), 3, P), F32)
    labels = np.empty(len(idx), np.int32)
    for b, i in enumerate(np.asarray(idx, np.int64)):
        if i < 0 or i >= N:
            x[b], labels[b] = np.nan, -1
            continue
        v = images[i].astype(F32)
        if ch == 4:
            v = np.where(v[:, 3:4] > 0, v[:, :3], F32(255))
        x[b], labels[b] = v.T, labels_all[i]
    return x, labels


# ---------------------------------------------------------------------------------------------- (hi, lo) pairs of a stats row
def pair_get(row, k):
    return float(row[k]) + float(row[k + 1])


def pair_put(row, k, v):
    with np.errstate(over='ignore', invalid='ignore'):
        hi = F32(v)
        row[k], row[k + 1] = hi, (F32(v - float(hi)) if np.isfinite(hi) else F32(0))


# ---------------------------------------------------------------------------------------------- 1b: nerfail_cls_ce
def row_stats(z, label):
    """(first-maximum argmax or -1, CE float64, softmax float64 [C]) of one float32 row, in double."""
    z = np.asarray(z, F32)
    C = z.size
    if np.isnan(z).any():
        return -1, math.nan, np.full(C, np.nan)
    arg = 0
    for c in range(1, C):
        if z[c] > z[arg]:
            arg = c
    r = z.astype(np.float64)
    e = np.array([math.exp(v - r[arg]) for v in r])
    s = 0.0
    for v in e:                               # summed in class order
        s += v
    p = e / s
    if not 0 <= label < C:
        return arg, math.nan, np.full(C, np.nan)
    return arg, r[arg] + math.log(s) - r[label], p


def ce(logits, labels, row, want_grad=True):
    """Adds the batch into the float32 stats row ([0,1] CE sum as (hi, lo), [2] correct, [3] views), views in order; returns
    (softmax - onehot) / B rounded once to float32, or None."""
    logits = np.asarray(logits, F32)
    B, C = logits.shape
    assert 1 <= C <= MAX_CLASSES
    d = np.empty((B, C), F32)
    total, correct = pair_get(row, 0), 0
    for b in range(B):
        label = int(labels[b])
        arg, c, p = row_stats(logits[b], label)
        total += c
        correct += int(0 <= label < C and arg == label)
        g = p.copy()
        if 0 <= label < C:
            g[label] -= 1.0
        with np.errstate(invalid='ignore'):
            d[b] = (g / float(B)).astype(F32)
    pair_put(row, 0, total)
    row[2] = F32(row[2] + F32(correct))
    row[3] = F32(row[3] + F32(B))
    return d if want_grad else None


# ---------------------------------------------------------------------------------------------- 1c: nerfail_cnn_sgd_step
def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise on float32 arrays. a * b is exact in double (24 + 24 bits); the double sum
    is rounded to odd (Boldo-Melquiond: TwoSum's error says on which side the exact value lies; of the two doubles around it the
    one with an odd last bit is kept), after which the rounding to float32 - 29 bits shorter - is the correct one."""
    prod = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
    c = np.asarray(c, F32).astype(np.float64)
    s = prod + c
    bb = s - prod
    err = (prod - (s - bb)) + (c - bb)        # TwoSum: prod + c = s + err exactly
    bits = s.view(np.int64).copy()
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(F32)


def sgd_step(p, g, buf, lr, mu, first):
    """torch.optim.SGD(lr, momentum=mu), dampening 0, no weight decay, no Nesterov, on float32 arrays (in place):
    buf <- g on the first step, else fl(fl(mu * buf) + g); p <- fma(-lr, buf, p). lr and mu are rounded to float32."""
    lr, mu = F32(lr), F32(mu)
    if first:
        buf[...] = g
    else:
        buf[...] = (mu * buf).astype(F32) + g
    p[...] = fma32(np.full(buf.shape, -lr, F32), buf, p)


def grad_layout(num_classes):
    """[(offset, shape)] and the total of nerfail_cnn_grad_floats: state-dict order, every region on a multiple of 4 floats."""
    chans = (3, 32, 64, 128, 256, 256, 128, 64)
    shapes = []
    for i in range(7):
        shapes += [(chans[i + 1], chans[i], 3, 3), (chans[i + 1],)]
    shapes += [(512, 1024), (512,), (num_classes, 512), (num_classes,)]
    out, o = [], 0
    for sh in shapes:
        out.append((o, sh))
        o += (int(np.prod(sh)) + 3) // 4 * 4
    return out, o


def layout_mask(num_classes):
    """bool [total]: True at the floats of a parameter, False at the alignment padding."""
    layout, total = grad_layout(num_classes)
    m = np.zeros(total, bool)
    for o, sh in layout:
        m[o:o + int(np.prod(sh))] = True
    return m


# ---------------------------------------------------------------------------------------------- 1d: nerfail_cls_epoch_close
def epoch_close(train_row, val_row, n_train, n_val, best, epoch):
    """(record float32 [16], flag): MTR:170-186. best = [best val acc, its epoch] (float32, updated in place). Division by the
    dataset lengths; strict >; NaN never taken."""
    rec = np.zeros(ROW, F32)
    rec[0] = F32(pair_get(train_row, 0) / n_train)
    rec[1] = F32(float(train_row[2]) / n_train)
    rec[2] = F32(pair_get(val_row, 0) / n_val)
    rec[3] = F32(float(val_row[2]) / n_val)
    take = bool(rec[3] > best[0])
    if take:
        best[0], best[1] = rec[3], F32(epoch)
    rec[4], rec[5], rec[6], rec[7] = F32(take), best[1], best[0], F32(epoch)
    rec[8], rec[9], rec[10], rec[11] = train_row[2], train_row[3], val_row[2], val_row[3]
    return rec, int(take)


# ---------------------------------------------------------------------------------------------- the loop's bookkeeping
def batches(order, batch_size):
    """drop_last=True: the whole batches of an epoch's index order."""
    order = np.asarray(order, np.int64)
    return [order[i:i + batch_size] for i in range(0, len(order) - batch_size + 1, batch_size)]


def save_epochs(epochs, save_model_epochs):
    """The 1-based epochs after whose validation phase a checkpoint is written (MTR:177)."""
    return [e + 1 for e in range(epochs) if (e + 1) % save_model_epochs == 0]


def bookkeeping(logits_train, labels_train, logits_val, labels_val, n_train, n_val):
    """The records of a run from every batch's logits: logits_* [epochs, batches, B, C], labels_* [epochs, batches, B].
    Returns (records [epochs,16], best = [acc, epoch])."""
    best = np.array([0, -1], F32)
    records = []
    for e in range(len(logits_train)):
        rows = []
        for lg, lb in ((logits_train[e], labels_train[e]), (logits_val[e], labels_val[e])):
            row = np.zeros(ROW, F32)
            for z, y in zip(lg, lb):
                ce(z, y, row, want_grad=False)
            rows.append(row)
        rec, _ = epoch_close(rows[0], rows[1], n_train, n_val, best, e)
        records.append(rec)
    return np.stack(records), best


def log_lines(rec):
    """The two lines MTR:173 prints for an epoch."""
    return ['{} Loss: {:.4f} Acc: {:.4f}'.format('train', float(rec[0]), float(rec[1])),
            '{} Loss: {:.4f} Acc: {:.4f}'.format('val', float(rec[2]), float(rec[3]))]
