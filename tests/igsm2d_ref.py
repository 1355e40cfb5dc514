"""Numpy restatement of the IGSM-2D baseline: universal_2D_net's forward (model/GaussNet.py:356-385 = GN, with the white
background of MyDataset.py:247-255 = MD) and the loop of attack_IGSM_2D.py:263-416 (= IG), written from those lines and from
include/nerfail_hip.h, section "2-D baseline" - not from the kernels. tests/test_igsm2d_ref.py holds it to fixture g28 (the
reference's own run, tests/golden/make_golden_igsm2d.py); tests/test_hip_u2d_kernels.py holds the kernels to it.

Also the fixture's scene (seeded images, the stand-in classifier's function and its analytic input gradient), shared by the
generator and the tests so that the 800 KB of images need not be stored."""
import numpy as np

import attack_loop_ref as R

F32 = np.float32


# ------------------------------------------------------------------------------------------------ GN:356-370, MD:247-255
def white(images):
    """MD:250-255: float32 [...,3] of a uint8 store [...,4] (rgb where alpha > 0, else 255) or [...,3] (as is)."""
    images = np.asarray(images)
    if images.shape[-1] == 3:
        return images.astype(F32)
    return np.where(images[..., 3:4] > 0, images[..., :3], np.uint8(255)).astype(F32)


def u2d_fwd(images, idx, r, shared=False):
    """(x_rgb float32 [B,...,3], cls_in float32 [B,3,...], pass_mask uint8 [B,...]) of the views idx. An index outside the store
    gives NaN views and a zero mask."""
    images, r = np.asarray(images), np.asarray(r, F32)
    N, hw = images.shape[0], images.shape[1:-1]
    B = len(idx)
    x = np.full((B,) + hw + (3,), np.nan, F32)
    mask = np.zeros((B,) + hw, np.uint8)
    for b, i in enumerate(idx):
        if not 0 <= i < N:
            continue
        with np.errstate(invalid='ignore'):
            v = white(images[i]) + (r if shared else r[i])                 # GN:363 / 365: one rounded float32 add
            x[b] = np.where(v < 0, F32(0), np.where(v > 255, F32(255), v))    # GN:367: torch.clip, a NaN stays
            ok = (v >= 0) & (v <= 255)                                      # where torch.clip's backward passes
        mask[b] = ok[..., 0] * 1 + ok[..., 1] * 2 + ok[..., 2] * 4
    cls_in = np.ascontiguousarray(np.moveaxis(x, -1, 1))                    # GN:369
    return x, cls_in, mask


# ------------------------------------------------------------------------------------------------ IG:335-379
def nan_max(a, b):
    """torch.max over a stacked pair: a NaN on either side is the result, a tie keeps the first."""
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(b > a, b, a))).astype(F32)


def nan_min(a, b):
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(b < a, b, a))).astype(F32)


def u2d_step(r, idx, d_cls_in, pass_mask, r_init, a, epsilon, targeted):
    """The table after IG:335-379 on rows idx (a copy; rows outside 0..N-1 are skipped)."""
    out = np.array(r, F32, copy=True)
    a, epsilon = F32(a), F32(epsilon)
    for b, i in enumerate(idx):
        if not 0 <= i < out.shape[0]:
            continue
        d = np.moveaxis(np.asarray(d_cls_in[b], F32), 0, -1)               # [...,3]
        bits = (np.asarray(pass_mask[b])[..., None] >> np.arange(3)) & 1
        with np.errstate(invalid='ignore'):
            g = np.where(bits == 1, d, F32(0))                              # torch.clip's backward: where(pass, grad, 0)
            sg = np.where(g > 0, F32(1), np.where(g < 0, F32(-1), F32(0)))  # torch.sign: 0 for +-0 and for NaN
        st = (a * sg).astype(F32)
        q = (out[i] - st if targeted else out[i] + st).astype(F32)          # IG:344 / 352
        init = np.zeros_like(q) if r_init is None else np.asarray(r_init[i], F32)
        q = nan_max(q, (init - epsilon).astype(F32))                        # IG:371-374
        q = nan_min(q, (init + epsilon).astype(F32))                        # IG:370, 376-377
        out[i] = q
    return out


def epoch_close_strict(row, best, epoch, targeted):
    """IG:392-416: attack_loop_ref.epoch_close with the strict comparison (a tie keeps the earlier epoch)."""
    rec, lax_best, _ = R.epoch_close(row, best, epoch, targeted)
    best = np.asarray(best, F32).copy()
    acc = rec[3]
    take = bool(acc > best[0]) if targeted else bool(acc < best[0])
    if take:
        best[0:3] = (acc, rec[2], epoch)
    rec[6:10] = (float(take), best[2], best[0], best[1])
    return rec, best, take


def u2d_sqerr(x_rgb, images, idx):
    """(sum (x_rgb - o)^2 in float64, number of elements) of IG:316."""
    images = np.asarray(images)
    o = np.stack([white(images[i]) for i in idx])
    return R.img_sqerr(x_rgb, o)


# ------------------------------------------------------------------------------------------------ fixture g28's scene
G28_N, G28_HW, G28_C, G28_EPOCHS, G28_BATCH = 4, 224, 8, 4, 3


def g28_images(seed, tints):
    """uint8 BGRA [4,224,224,4] from a seeded legacy RandomState (stable across numpy versions): views 0 and 2 are transparent
    outside a centred disc (their pixels there reach the classifier as white), views 1 and 3 opaque everywhere. Each view has
    its own brightness `tints[v]`, so the views sit at different distances from the decision boundary."""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, size=(G28_N, G28_HW, G28_HW, 4)).astype(np.float64)
    img[..., :3] = np.floor(img[..., :3] * np.asarray(tints, np.float64).reshape(G28_N, 1, 1, 1))
    yy, xx = np.mgrid[0:G28_HW, 0:G28_HW]
    inside = ((yy - G28_HW / 2 + .5) ** 2 + (xx - G28_HW / 2 + .5) ** 2) <= (0.375 * G28_HW) ** 2
    img[..., 3] = 255.
    img[0, ..., 3] = np.where(inside, 255., 0.)
    img[2, ..., 3] = np.where(inside, 255., 0.)
    return img.astype(np.uint8)


def pool_logits(cls_in, w):
    """The stand-in classifier (g15's, evaluated in float64 and rounded once as g24's PoolCls64): 4 x 4 average pooling of the
    NCHW input, then a [C,48] matrix."""
    x = np.asarray(cls_in).astype(np.float64)
    B, ch, H, W = x.shape
    p = x.reshape(B, ch, 4, H // 4, 4, W // 4).mean((3, 5)).reshape(B, -1)
    return (p @ np.asarray(w).astype(np.float64).T).astype(F32)


def pool_ce_grad(logits, label, w, H, W):
    """d mean-CE / d cls_in of pool_logits, float64: (softmax - onehot) / B through the matrix and the pooling."""
    z = np.asarray(logits).astype(np.float64)
    B = z.shape[0]
    e = np.exp(z - z.max(1, keepdims=True))
    d = e / e.sum(1, keepdims=True)
    d[:, label] -= 1.
    d /= B
    gp = (d @ np.asarray(w).astype(np.float64)).reshape(B, 3, 4, 1, 4, 1) / ((H // 4) * (W // 4))
    return np.broadcast_to(gp, (B, 3, 4, H // 4, 4, W // 4)).reshape(B, 3, H, W)


def checksums(table):
    """Two float64 checksums per view of a table [N,H,W,3]: the plain sum, and the sum weighted by 1 + (element index mod 251)
    (exact in float64 for small-integer tables: a transposition or a moved element changes it)."""
    t = np.asarray(table).astype(np.float64).reshape(table.shape[0], -1)
    wgt = 1. + (np.arange(t.shape[1]) % 251)
    return np.stack([t.sum(1), (t * wgt).sum(1)], 1)


def run_loop(images, w, label, epochs, a, epsilon, targeted, batch_size):
    """IG:263-416 with the stand-in classifier. Returns a dict: iterates (the table after every attack batch), best, last,
    best_epoch, taken, records (float32 [epochs, 16]), stats_f64 (test CE, attack CE, image loss means), logits (ori_cla, cla
    per epoch) and the export pass's uint8 images."""
    images = np.asarray(images)
    N, H, W = images.shape[:3]
    table = np.zeros((N, H, W, 3), F32)                                     # IG:250-253
    best_table = table.copy()
    best = R.best_init(targeted)                                            # IG:255-261
    batches = [list(range(lo, min(lo + batch_size, N))) for lo in range(0, N, batch_size)]
    zero = np.zeros((H, W, 3), F32)
    ori_cla = np.concatenate([pool_logits(u2d_fwd(images, ib, zero, True)[1], w) for ib in batches])
    out = dict(iterates=[], taken=[], records=[], stats_f64=[], cla=[], adv_u8=[], mask_u8=[])
    for epoch in range(epochs):
        export = epoch == epochs - 1
        src = best_table if export else table                               # IG:294-301
        row = np.zeros(R.ROW, F32)
        ce64, sq64, ep_cla = np.zeros(2), 0., []
        for ib in batches:                                                  # IG:289: the full loader, every epoch
            x_rgb, cls_in, mask = u2d_fwd(images, ib, table if not export else src)
            cla = pool_logits(cls_in, w)
            st = R.logit_stats(cla, ori_cla[ib], label)                     # IG:306-317, 326-331
            sq = u2d_sqerr(x_rgb, images, ib)
            row = R.add_to_row(row, stats=st, sqerr=sq)
            ce64 += st[:2]
            sq64 += sq[0] / sq[1] * len(ib)                                 # IG:328: the batch MEAN times len(ori_img)
            ep_cla.append(cla)
            if not export:
                d = pool_ce_grad(cla, label, w, H, W).astype(F32)            # IG:335 (beta = 0, IG:69: CE alone)
                table = u2d_step(table, ib, d, mask, None, a, epsilon, targeted)
                out['iterates'].append(table.copy())
            else:                                                           # IG:381-390
                out['adv_u8'].append(R.export_u8(x_rgb))
                out['mask_u8'].append(R.export_u8(src[ib]))
        rec, best, take = epoch_close_strict(row, best, epoch, targeted)    # IG:392-416
        if take and not export:
            best_table = table.copy()
        out['records'].append(rec)
        out['taken'].append(int(take))
        out['stats_f64'].append([ce64[0] / N, ce64[1] / N, sq64 / N])
        out['cla'].append(np.concatenate(ep_cla))
        if epoch == epochs - 2:
            out['best_epoch'] = int(best[2])
    if epochs == 1:
        out['best_epoch'] = -1
    out.update(best=best_table, last=table, ori_cla=ori_cla, records=np.stack(out['records']), taken=np.array(out['taken']),
               stats_f64=np.array(out['stats_f64']), cla=np.stack(out['cla']), adv_u8=np.concatenate(out['adv_u8']),
               mask_u8=np.concatenate(out['mask_u8']))
    return out
