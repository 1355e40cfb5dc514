"""Numpy restatement of the NeRFail-S epoch bookkeeping (include/nerfail_hip.h, section "NeRFail-S epoch statistics"):
what nerfail_attack_logit_stats, nerfail_img_sqerr, nerfail_attack_epoch_close and nerfail_export_u8 compute, written
from the header's definitions and attack_NeRFail_S.py:319-344, 405-431 (AS) - not from the kernels. tests/test_attack_loop_ref.py
holds it to fixture g24 (the reference's own run); tests/test_hip_attack_stats.py holds the kernels to it."""
import numpy as np

ROW = 16          # NERFAIL_ATTACK_ROW_FLOATS


def ce_rows(logits, label):
    """Per-row cross entropy: log-sum-exp with the maximum subtracted, minus the label's logit; float64 from the given values."""
    z = np.asarray(logits).astype(np.float64)
    with np.errstate(invalid='ignore'):
        m = np.where(np.isnan(z).any(1), np.nan, np.nanmax(z, 1))
        return m + np.log(np.exp(z - m[:, None]).sum(1)) - z[:, label]


def correct_rows(logits, label):
    """argmax == label with the FIRST maximum as argmax; a row holding a NaN is never correct."""
    z = np.asarray(logits)
    out = np.zeros(z.shape[0], bool)
    for b, row in enumerate(z):
        if np.isnan(row).any():
            continue
        arg = 0
        for c in range(1, row.size):
            if row[c] > row[arg]:
                arg = c
        out[b] = arg == label
    return out


def logit_stats(cla, ori_cla, label):
    """(sum CE(ori_cla), sum CE(cla), correct(ori_cla), correct(cla), B): what one launch adds into the row, in this order."""
    return (float(ce_rows(ori_cla, label).sum()), float(ce_rows(cla, label).sum()),
            int(correct_rows(ori_cla, label).sum()), int(correct_rows(cla, label).sum()), int(np.asarray(cla).shape[0]))


def img_sqerr(x_rgba, ori):
    """(sum (x_rgba - ori)^2 in float64, number of elements)."""
    d = np.asarray(x_rgba).astype(np.float64) - np.asarray(ori).astype(np.float64)
    return float((d * d).sum()), int(d.size)


def pair(v):
    """(hi, lo) float32 of a float64: hi the value rounded to float32, lo the rest."""
    hi = np.float32(v)
    return hi, (np.float32(np.float64(v) - np.float64(hi)) if np.isfinite(hi) else np.float32(0))


def unpair(row, i):
    return np.float64(row[i]) + np.float64(row[i + 1])


def add_to_row(row, stats=None, sqerr=None):
    """Accumulates logit_stats() / img_sqerr() results into a float32 row of ROW floats the way the kernels do."""
    row = np.asarray(row, np.float32).copy()
    if stats is not None:
        row[0:2] = pair(unpair(row, 0) + stats[0])
        row[2:4] = pair(unpair(row, 2) + stats[1])
        row[4] += np.float32(stats[2])
        row[5] += np.float32(stats[3])
        row[6] += np.float32(stats[4])
    if sqerr is not None:
        row[7:9] = pair(unpair(row, 7) + sqerr[0])
        row[9:11] = pair(unpair(row, 9) + sqerr[1])
    return row


def best_init(targeted):
    return np.array([0. if targeted else 10000., 0., -1., 0.], np.float32)       # AS:270-276


def epoch_close(row, best, epoch, targeted):
    """AS:405-431: (record float32 [ROW], new best [4], taken). Means in float64, rounded to float32 once."""
    row = np.asarray(row, np.float32)
    views = np.float64(row[6])
    with np.errstate(invalid='ignore', divide='ignore'):
        test_loss, attack_loss = np.float32(unpair(row, 0) / views), np.float32(unpair(row, 2) / views)
        test_acc, attack_acc = np.float32(np.float64(row[4]) / views), np.float32(np.float64(row[5]) / views)
        img_loss = np.float32(unpair(row, 7) / unpair(row, 9))
    best = np.asarray(best, np.float32).copy()
    take = bool(attack_acc >= best[0]) if targeted else bool(attack_acc <= best[0])
    if take:
        best[0:3] = (attack_acc, attack_loss, epoch)
    rec = np.zeros(ROW, np.float32)
    rec[:13] = (test_loss, test_acc, attack_loss, attack_acc, img_loss, row[6], float(take), best[2], best[0], best[1], epoch, row[4], row[5])
    return rec, best, take


def export_u8(x):
    """cv2.imwrite's float -> uint8: clamp to [0, 255], round half to even; NaN -> 0."""
    v = np.asarray(x, np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.rint(np.clip(v, 0., 255.)).astype(np.uint8)
