"""Pins tests/cls_train_ref.py, the restatement the victim-training kernels are tested against: the SGD arithmetic to torch's CPU
kernels (bitwise), the cross-entropy gradient to float64 F.cross_entropy, the epoch bookkeeping to fixture g26 (the reference's
own run, tests/golden/make_golden_cls_train.py), and the new C-ABI section to its revision word and signatures."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cls_train_ref as R
from conftest import ROOT

LR, MU = 0.001, 0.9


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------ (i) SGD
def _sgd_case(p0, grads, foreach):
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([p], lr=LR, momentum=MU, foreach=foreach)
    mine_p, mine_buf = p0.copy(), np.zeros_like(p0)
    for t, g in enumerate(grads):
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        R.sgd_step(mine_p, g, mine_buf, LR, MU, first=(t == 0))
        bad_p = int((_bits(p.detach().numpy()) != _bits(mine_p)).sum())
        bad_b = int((_bits(opt.state[p]['momentum_buffer'].numpy()) != _bits(mine_buf)).sum())
        print('step %d foreach=%s: %d parameter and %d momentum mismatches of %d' % (t + 1, foreach, bad_p, bad_b, p0.size))
        assert bad_p == 0 and bad_b == 0


@pytest.mark.parametrize('foreach', [False, True])
def test_sgd_equals_torch_cpu_bitwise_over_three_steps(foreach):
    rs = np.random.RandomState(7)
    n = 1 << 20
    p0 = (rs.standard_normal(n) * np.exp(rs.uniform(-8, 2, n))).astype(np.float32)
    grads = [(rs.standard_normal(n) * np.exp(rs.uniform(-8, 4, n))).astype(np.float32) for _ in range(3)]
    _sgd_case(p0, grads, foreach)


def test_sgd_on_the_real_layout():
    """The flat buffer of 8 classes, weights of the module's scale, three steps; the padding floats stay what they were."""
    import cnn_inputs as CI
    layout, total = R.grad_layout(8)
    mask = R.layout_mask(8)
    sd = CI.state_dict(5, 8)
    p0 = np.full(total, 7.0, np.float32)
    for (o, sh), (_, v) in zip(layout, sd.items()):
        assert tuple(v.shape) == tuple(sh)
        p0[o:o + v.size] = v.reshape(-1)
    rs = np.random.RandomState(8)
    grads = [np.where(mask, rs.standard_normal(total) * 10.0, 0.0).astype(np.float32) for _ in range(3)]
    _sgd_case(p0, grads, None)
    assert [o for o, _ in layout][:4] == [0, 864, 896, 896 + 18432]


def test_fma32_is_one_rounding():
    """Cases where fl(fl(a b) + c) and fl64-then-fl32 differ from the fused result."""
    a = np.array([1 + 2.0 ** -12, 3.0, 1 + 2.0 ** -23], np.float32)
    b = np.array([1 + 2.0 ** -12, 2.0 ** -30, 1 + 2.0 ** -23], np.float32)
    c = np.array([-1.0, 1.0, 2.0 ** 30], np.float32)
    from fractions import Fraction
    got = R.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(exact - Fraction(float(got[i]))) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi))))


# ------------------------------------------------------------------------------------------------------------ (ii) cross entropy
def _ce_inputs(C, B=5, seed=0):
    rs = np.random.RandomState(seed + C)
    z = (rs.standard_normal((B, C)) * 4).astype(np.float32)
    y = rs.randint(0, C, size=B).astype(np.int32)
    return z, y


@pytest.mark.parametrize('C', [1, 8, 32])
def test_ce_gradient_is_one_rounding_of_float64(C):
    z, y = _ce_inputs(C)
    row = np.zeros(R.ROW, np.float32)
    d = R.ce(z, y, row)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    loss = F.cross_entropy(zt, torch.from_numpy(y).long())
    loss.backward()
    want = zt.grad.numpy()
    err = np.abs(d.astype(np.float64) - want)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print('C=%d: worst error %.2e of an ulp' % (C, float((err / ulp).max())))
    assert (err <= ulp).all()                                   # one float32 rounding (half an ulp, plus float64 noise)
    per_view = F.cross_entropy(zt.detach(), torch.from_numpy(y).long(), reduction='sum').item()
    assert abs(R.pair_get(row, 0) - per_view) <= 1e-12 * max(1.0, abs(per_view))
    assert row[2] == float((z.argmax(1) == y).sum()) and row[3] == z.shape[0]


def test_ce_nan_row_equal_maxima_and_bad_label():
    z = np.array([[1, 5, 5, 0], [np.nan, 1, 2, 3], [0, 1, 2, 3], [4, 4, 4, 4]], np.float32)
    y = np.array([2, 3, 7, 0], np.int32)                         # row 0: the FIRST maximum is class 1, so label 2 is wrong
    row = np.zeros(R.ROW, np.float32)
    d = R.ce(z, y, row)
    assert R.row_stats(z[0], 2)[0] == 1 and R.row_stats(z[3], 0)[0] == 0
    assert np.isnan(d[1]).all() and np.isnan(d[2]).all() and np.isfinite(d[0]).all() and np.isfinite(d[3]).all()
    assert row[2] == 1 and row[3] == 4                           # only row 3 is correct
    assert math.isnan(R.pair_get(row, 0)) and row[1] == 0        # a NaN CE makes the sum NaN; lo stays finite
    row2 = np.zeros(R.ROW, np.float32)
    R.ce(z[[0, 3]], y[[0, 3]], row2)
    R.ce(z[[3]], y[[3]], row2)                                   # two batches accumulate
    want = 2 * math.log(4.0) + (5 + math.log(2 + math.exp(-4) + math.exp(-5)) - 5)
    assert abs(R.pair_get(row2, 0) - want) < 1e-12 and row2[2] == 2 and row2[3] == 3


# ------------------------------------------------------------------------------------------------------------ (iii) bookkeeping
def test_bookkeeping_matches_the_reference_run(golden):
    g = golden('g26_cls_train')
    E, bs = int(g['epochs']), int(g['batch'])
    n_train, n_val = len(g['train_labels']), len(g['val_labels'])
    assert (n_train, n_val, bs) == (5, 3, 2)                     # each phase drops one view
    for tag in ('f32', 'f64'):
        lt, lv = g['logits_train_' + tag], g['logits_val_' + tag]
        yt = [[g['train_labels'][b] for b in R.batches(g['order_train'][e], bs)] for e in range(E)]
        yv = [[g['val_labels'][b] for b in R.batches(g['order_val'][e], bs)] for e in range(E)]
        assert lt.shape[:3] == (E, n_train // bs, bs) and lv.shape[:3] == (E, n_val // bs, bs)
        rec, best = R.bookkeeping(lt, yt, lv, yv, n_train, n_val)
        # prediction-derived numbers: equal
        assert np.array_equal(rec[:, 1], g['acc_' + tag][:, 0].astype(np.float32))
        assert np.array_equal(rec[:, 3], g['acc_' + tag][:, 1].astype(np.float32))
        assert rec[:, 4].astype(int).tolist() == g['taken_' + tag].tolist()
        assert int(best[1]) == int(g['best_epoch_' + tag]) and best[0] == np.float32(g['best_acc_' + tag])
        assert rec[:, 9].tolist() == [4.0] * E and rec[:, 11].tolist() == [2.0] * E          # views seen < the divisors 5 and 3
        # losses: the reference forms each batch's mean CE in the run's precision (log_softmax, nll, mean: a handful of
        # roundings at the size of the largest logit and of the loss) and multiplies it back by B (MTR:168); the sum of per-view
        # CE here is exact. Allowed per batch: 8 roundings of (max |logit| + loss); plus the record's own float32 rounding.
        eps = 2.0 ** -24 if tag == 'f32' else 2.0 ** -53
        for k, ph, lg, n in ((0, 'train', lt, n_train), (2, 'val', lv, n_val)):
            want = g['loss_' + tag][:, k // 2]
            size = np.abs(lg).max((2, 3)) + np.abs(g['batch_loss_%s_%s' % (ph, tag)])
            slack = 8 * eps * size.sum(1) * bs / n + 2.0 ** -24 * np.abs(want)
            err = np.abs(rec[:, k].astype(np.float64) - want)
            print(tag, ph, 'loss error', err, 'allowed', slack)
            assert (err <= slack).all()
    assert 0 < int(g['best_epoch_f32']) and int((g['acc_f32'][:, 1] == g['best_acc_f32']).sum()) == 1
    assert R.save_epochs(E, int(g['save_model_epochs'])) == g['saved_f32'].tolist() == [2]


def test_epoch_close_rule():
    def rows(correct, views, ce_sum):
        r = np.zeros(R.ROW, np.float32)
        R.pair_put(r, 0, ce_sum)
        r[2], r[3] = correct, views
        return r
    best = np.array([0, -1], np.float32)
    rec, flag = R.epoch_close(rows(2, 4, 6.0), rows(0, 2, 3.0), 5, 3, best, 0)
    assert flag == 0 and best.tolist() == [0, -1]                # 0 > 0 is false: the initial best stays
    assert rec[0] == np.float32(6.0 / 5) and rec[1] == np.float32(2 / 5) and rec[2] == np.float32(1.0) and rec[3] == 0
    rec, flag = R.epoch_close(rows(2, 4, 6.0), rows(1, 2, 3.0), 5, 3, best, 1)
    assert flag == 1 and best.tolist() == [np.float32(1 / 3), 1] and rec[4:8].tolist() == [1, 1, np.float32(1 / 3), 1]
    rec, flag = R.epoch_close(rows(2, 4, 6.0), rows(1, 2, 3.0), 5, 3, best, 2)
    assert flag == 0 and best[1] == 1 and rec[4:8].tolist() == [0, 1, np.float32(1 / 3), 2]     # a tie keeps the earlier epoch
    rec, flag = R.epoch_close(rows(2, 4, 6.0), rows(np.nan, 2, 3.0), 5, 3, best, 3)
    assert flag == 0 and best[1] == 1                             # NaN is never taken
    assert R.log_lines(rec)[0] == 'train Loss: 1.2000 Acc: 0.4000'


def test_batch_restatement():
    img = np.array([[[10, 20, 30, 0], [40, 50, 60, 7]], [[1, 2, 3, 255], [4, 5, 6, 0]]], np.uint8)
    x, lb = R.batch(img, np.array([3, 5], np.int32), [1, 0, 2, 1])
    assert lb.tolist() == [5, 3, -1, 5] and np.isnan(x[2]).all()
    assert x[0].tolist() == [[1, 255], [2, 255], [3, 255]] and x[1].tolist() == [[255, 40], [255, 50], [255, 60]]
    x3, _ = R.batch(img[..., :3], np.array([3, 5], np.int32), [0])
    assert x3[0].tolist() == [[10, 40], [20, 50], [30, 60]]


# ------------------------------------------------------------------------------------------------------------ (iv) revisions
NEW = ('nerfail_cls_revision', 'nerfail_cls_batch', 'nerfail_cls_ce', 'nerfail_cnn_sgd_step', 'nerfail_cls_epoch_close')


def test_revisions_and_signatures():
    import ctypes
    from nerfail_amd import _lib
    lib = _lib.load()
    assert lib.nerfail_cls_revision() == 1 == _lib.CLS_REVISION
    assert (lib.nerfail_abi_version(), lib.nerfail_abi_revision(), lib.nerfail_eval_revision()) == (14, 15, 1)
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nerfail_hip.h')).read(), flags=re.S)
    ctype = {'int': ctypes.c_int, 'float': ctypes.c_float, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t}
    for name in NEW:
        m = re.search(r'\b(\w+)\s+%s\s*\(([^)]*)\)\s*;' % name, text)
        assert m, name
        args = [a.strip() for a in m.group(2).split(',') if a.strip() != 'void']
        want = [ctypes.c_void_p if '*' in a else ctype[a.split()[-2]] for a in args]
        res, got = _lib.SIGNATURES[name]
        assert res is ctype[m.group(1)] and got == want, (name, got, want)


def test_new_entries_reject_bad_arguments_before_any_launch():
    from nerfail_amd import _lib
    lib = _lib.load()
    assert lib.nerfail_cls_batch(None, 2, None, 4, 16, None, 1, None, None, None) == 1 and b'format' in lib.nerfail_last_error()
    assert lib.nerfail_cls_batch(None, 0, None, 4, 16, None, 0, None, None, None) == 0          # B == 0: a no-op
    assert lib.nerfail_cls_batch(None, 0, None, 4, 16, None, 2, None, None, None) == 1 and b'NULL' in lib.nerfail_last_error()
    assert lib.nerfail_cls_batch(None, 0, None, 4, 16, None, 70000, None, None, None) == 1
    assert lib.nerfail_cls_ce(None, None, 4, 33, None, None, None) == 1 and b'1..32' in lib.nerfail_last_error()
    assert lib.nerfail_cls_ce(None, None, 4, 0, None, None, None) == 1
    assert lib.nerfail_cls_ce(None, None, 4, 8, None, None, None) == 1 and b'NULL' in lib.nerfail_last_error()
    assert lib.nerfail_cls_ce(None, None, 0, 8, None, None, None) == 0
    assert lib.nerfail_cnn_sgd_step(None, None, None, None, 8, 0.001, 0.9, 1, None) == 1 and b'NULL' in lib.nerfail_last_error()
    assert lib.nerfail_cnn_sgd_step(16, 16, 16, 20, 8, 0.001, 0.9, 1, None) == 1 and b'aligned' in lib.nerfail_last_error()
    assert lib.nerfail_cnn_sgd_step(16, 16, 16, 16, 0, 0.001, 0.9, 1, None) == 1
    assert lib.nerfail_cls_epoch_close(None, None, 5, 3, None, 0, None, None, None) == 1
    assert lib.nerfail_cls_epoch_close(16, 16, 0, 3, 16, 0, 16, 16, None) == 1 and b'lengths' in lib.nerfail_last_error()
