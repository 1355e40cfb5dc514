"""Numpy float64 restatement of the attack evaluation (include/nerfail_hip.h, section "Attack evaluation"): what
nerfail_eval_view_metrics, nerfail_eval_logit_stats, nerfail_eval_fold and nerfail_amd.model_test.report compute, written from
the header's definitions and model_test.py:26-39, 237-278, 292-299, 341-399 (MT), MyDataset.py:93-113 (MD) - not from the
kernels. tests/test_eval_ref.py holds it to fixture g25 (the reference's own run); tests/test_hip_eval.py holds the kernels to it."""
import math

import numpy as np

import eval_inputs as EI

U8C4, U8C3, F32C4, FLAT = 0, 1, 2, 3          # NERFAIL_EVAL_*
VIEW, RECORD, MAX_CLASSES = 6, 48, 32         # NERFAIL_EVAL_VIEW_DOUBLES, NERFAIL_EVAL_RECORD_DOUBLES, NERFAIL_ATTACK_MAX_CLASSES
PSNR_IDENTICAL = 20 * math.log10(255.0 / float(np.finfo(np.float64).eps))


def white(img, fmt):
    """One view as float32 elements after the white background (MT:237-254, MD:98-105): [P,3] for the image formats (rgb where
    alpha > 0, else 255 - a NaN alpha fails the comparison), the elements themselves for FLAT."""
    a = np.asarray(img)
    if fmt == FLAT:
        return a.astype(np.float32).reshape(-1)
    if fmt == U8C3:
        return a.reshape(-1, 3).astype(np.float32)
    a = a.reshape(-1, 4).astype(np.float32)
    with np.errstate(invalid='ignore'):
        return np.where(a[:, 3:4] > 0, a[:, :3], np.float32(255))


def cla_in(img, fmt):
    """[3,P] float32: the planar classifier input of one view."""
    return np.ascontiguousarray(white(img, fmt).T)


def view_row(a, a_fmt, o, o_fmt):
    """{max d, min d, sum d, sum d^2, count(d != 0), n} of d = |a - o| (one float32 subtraction), sums in float64. A NaN element
    makes max, min and both sums NaN and counts as non-zero."""
    with np.errstate(invalid='ignore'):
        d = np.abs(white(a, a_fmt) - white(o, o_fmt)).reshape(-1)
    assert d.dtype == np.float32
    dd = d.astype(np.float64)
    nan = bool(np.isnan(d).any())
    with np.errstate(invalid='ignore', over='ignore'):
        return np.array([np.nan if nan else dd.max(), np.nan if nan else dd.min(), dd.sum(), (dd * dd).sum(), np.count_nonzero(d), d.size],
                        np.float64)


def view_rows(attacked, a_fmt, originals, o_fmt):
    return np.stack([view_row(a, a_fmt, o, o_fmt) for a, o in zip(attacked, originals)])


def logit_stats(logits, label):
    """(pred int32 [B], ce float64 [B]): the FIRST maximum; max-subtracted log-sum-exp minus the label's logit; a row holding a
    NaN predicts -1 and has CE NaN."""
    z = np.asarray(logits, np.float32)
    pred, ce = np.zeros(z.shape[0], np.int32), np.zeros(z.shape[0], np.float64)
    for b, row in enumerate(z):
        if np.isnan(row).any():
            pred[b], ce[b] = -1, np.nan
            continue
        arg = 0
        for c in range(1, row.size):
            if row[c] > row[arg]:
                arg = c
        r = row.astype(np.float64)
        pred[b], ce[b] = arg, r[arg] + math.log(np.exp(r - r[arg]).sum()) - r[label]
    return pred, ce


def psnr_of(sum_sq, n):
    """get_psnr (MT:26-39) from sum d^2 and the element count."""
    rmse = math.sqrt(sum_sq / n) if not math.isnan(sum_sq) else math.nan
    if rmse == 0:
        rmse = float(np.finfo(np.float64).eps)
    return 20 * math.log10(255.0 / rmse) if not math.isnan(rmse) else math.nan


def _nmax(m, v):
    return math.nan if (math.isnan(m) or math.isnan(v)) else max(m, v)


def _nmin(m, v):
    return math.nan if (math.isnan(m) or math.isnan(v)) else min(m, v)


def fold(record, rows, pred, ce, C):
    """One batch into the set record (the header's field list); record[0] == 0 marks the first view."""
    rec = np.asarray(record, np.float64).copy()
    assert rec.size == RECORD
    for r, k, c in zip(np.asarray(rows, np.float64), pred, ce):
        n = r[5]
        psnr = psnr_of(r[3], n)
        first = rec[0] == 0
        rec[1] = r[0] if first else _nmax(rec[1], r[0])
        rec[2] = r[1] if first else _nmin(rec[2], r[1])
        rec[7] = psnr if first else _nmax(rec[7], psnr)
        rec[6] = psnr if first else _nmin(rec[6], psnr)
        rec[3] += r[2] / n
        rec[4] += math.sqrt(r[3]) if not math.isnan(r[3]) else math.nan
        rec[5] += r[4]
        rec[8] += psnr
        rec[9] += c
        rec[11] += n
        if 0 <= k < C:
            rec[16 + int(k)] += 1
        else:
            rec[10] += 1
        rec[0] += 1
    return rec


def report(record, label, num_classes):
    """msg_dict of MT:355-399 from a record: the reference's keys and string forms, plus 'loss' and 'acc' as floats. Views
    without a prediction are counted under the key '<label> to -1'."""
    rec = np.asarray(record, np.float64)
    number = int(rec[0])
    hist = {k: int(rec[16 + k]) for k in range(num_classes) if rec[16 + k] > 0}
    if rec[10] > 0:
        hist[-1] = int(rec[10])
    msg = {'attack acc': '100.0 %' if label not in hist else str((1 - hist[label] / number) * 100) + ' %'}
    for k, cnt in hist.items():
        msg['%d to %d' % (label, k)] = str((cnt / number) * 100) + ' %'
    msg.update({'e min': float(rec[2]), 'e avg': float(rec[3] / number), 'e max': float(rec[1]), 'd l2 norm': float(rec[4] / number),
                'd l0 norm': float(rec[5] / number), 'psnr min': float(rec[6]), 'psnr max': float(rec[7]), 'psnr avg': float(rec[8] / number),
                'loss': float(rec[9] / number), 'acc': hist.get(label, 0) / number})
    return msg


def evaluate(attacked, a_fmt, originals, o_fmt, logits, label, num_classes, batch=8):
    """The whole chain on the host: rows, predictions, fold in batches, report."""
    rec = np.zeros(RECORD)
    rows = view_rows(attacked, a_fmt, originals, o_fmt)
    pred, ce = logit_stats(logits, label)
    for b0 in range(0, len(rows), batch):
        rec = fold(rec, rows[b0:b0 + batch], pred[b0:b0 + batch], ce[b0:b0 + batch], num_classes)
    return rec, report(rec, label, num_classes)


# ---------------------------------------------------------------------------------------------------------- fixture g25
def stored_msg(g):
    return {str(k): (float(v) if f else str(v)) for k, v, f in zip(g['msg_keys'], g['msg_values'], g['msg_is_float'])}


def g25_pairs(g):
    return EI.view_pairs([int(s) for s in g['image_seeds']], int(g['pert_seed']), int(g['side']), int(g['bound']), int(g['identical']),
                         int(g['hidden']))


def check_msg(msg, g, who, logit_slack=0.0):
    """The rules every implementation is held to against g25's msg_dict: strings (percentages) and integer-valued entries exact;
    float entries within twice the reference's own float32-vs-float64 gap. 'loss' (not in the reference's dict; judged against
    the mean CE of the reference's logits) gets 2 * logit_slack on top when the logits are the implementation's own: a CE moves
    by at most twice the largest change of a logit."""
    want = stored_msg(g)
    gap = {str(k): abs(want[str(k)] - float(v)) for k, v in zip(g['msg_f64_keys'], g['msg_f64_values'])}
    assert set(want) <= set(msg) and set(msg) - set(want) == {'loss', 'acc'}, (who, sorted(msg), sorted(want))
    for k, v in want.items():
        if isinstance(v, str) or k in ('e min', 'e max'):
            assert msg[k] == v, (who, k, msg[k], v)
        else:
            print('%s %-10s got %.17g reference %.17g |diff| %.2e bound %.2e' % (who, k, msg[k], v, abs(msg[k] - v), 2 * gap[k]))
            assert abs(msg[k] - v) <= 2 * gap[k], (who, k, msg[k], v, gap[k])
    ce_gap = abs(float(g['ce_f32']) - float(g['ce_f64']))
    print('%s loss got %.17g reference %.9g bound %.2e' % (who, msg['loss'], float(g['ce_f32']), 2 * ce_gap))
    assert abs(msg['loss'] - float(g['ce_f32'])) <= 2 * ce_gap + 2 * logit_slack
    assert msg['acc'] == float((g['logits'].argmax(1) == int(g['label'])).mean())
