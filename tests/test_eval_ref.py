"""The numpy restatement of the attack evaluation (tests/eval_ref.py) against fixture g25 = the REFERENCE's test_for_inception
run on six 800 x 800 view pairs (tests/golden/make_golden_eval.py), and the host-side contract of the new entry points.

Measured when g25 was generated (reference float32 vs the same lines in float64; the bound of a float entry is twice this gap,
because the restatement's float64 sits on one side of it and the reference's float32 on the other):
    e avg 4.5e-08   d l2 norm 8.2e-04   d l0 norm 5.2e-03 (an int64 sum divided as float32)   psnr min 2.3e-07   psnr avg 5.8e-09
    e min, e max, psnr max (the identical pair: 20 log10(255 / eps)): gap 0, held exactly.   mean CE: 7.1e-08."""
import ctypes
import inspect

import numpy as np
import pytest

import eval_ref as R
from eval_ref import check_msg, g25_pairs


@pytest.fixture(scope='module')
def g25_run(golden):
    g = golden('g25_eval')
    originals, attacked = g25_pairs(g)
    rec, msg = R.evaluate(attacked, R.U8C4, originals, R.U8C4, g['logits'], int(g['label']), int(g['num_classes']), batch=4)
    return g, originals, attacked, rec, msg


def test_restatement_matches_reference_report(g25_run):
    g, originals, attacked, rec, msg = g25_run
    check_msg(msg, g, 'restatement')
    assert rec[0] == 6 and rec[10] == 0
    hist = np.bincount(g['logits'].argmax(1), minlength=R.MAX_CLASSES)
    assert rec[16:].tolist() == hist.tolist() and 0 < hist[int(g['label'])] < 6                     # histogram: exact
    assert rec[5] == g['view_metrics_f64'][:, 4].sum() == g['view_metrics_f32'][:, 4].sum()         # d l0: exact
    assert rec[5] < rec[11] == 6 * 3 * int(g['side']) ** 2


def test_restatement_matches_reference_per_view(g25_run):
    g, originals, attacked, rec, msg = g25_run
    rows = R.view_rows(attacked, R.U8C4, originals, R.U8C4)
    m32, m64 = g['view_metrics_f32'], g['view_metrics_f64']                                         # e max, e avg, e min, d l2, d l0, psnr
    mine = np.stack([rows[:, 0], rows[:, 2] / rows[:, 5], rows[:, 1], np.sqrt(rows[:, 3]), rows[:, 4],
                     [R.psnr_of(r[3], r[5]) for r in rows]], 1)
    assert np.array_equal(mine[:, [0, 2, 4]], m32[:, [0, 2, 4]])                                    # integers: exact
    assert (np.abs(mine - m32) <= 2 * np.abs(m32 - m64)).all(), np.abs(mine - m32) / np.maximum(np.abs(m32 - m64), 1e-300)
    i = int(g['identical'])
    assert rows[i, 3] == 0 and mine[i, 5] == R.PSNR_IDENTICAL == m32[i, 5]                          # the rmse == 0 branch
    h = int(g['hidden'])
    assert (attacked[h][..., 3] == 0).any() and (attacked[h][attacked[h][..., 3] == 0][:, :3] != 0).any()
    pred, ce = R.logit_stats(g['logits'], int(g['label']))
    assert pred.tolist() == g['logits'].argmax(1).tolist()
    assert abs(ce.mean() - float(g['ce_f64'])) <= 1e-12


def test_white_background_and_nan_rules():
    px = np.array([[10, 20, 30, 0], [10, 20, 30, 1], [1, 2, 3, 255]], np.uint8)
    assert R.white(px, R.U8C4).tolist() == [[255, 255, 255], [10, 20, 30], [1, 2, 3]]
    f = px.astype(np.float32)
    f[1, 3] = np.nan                                                                                # a NaN alpha: white
    assert R.white(f, R.F32C4).tolist() == [[255, 255, 255], [255, 255, 255], [1, 2, 3]]
    o = px.astype(np.float32)
    f2 = o.copy()
    f2[2, 1] = np.nan
    row = R.view_row(f2, R.F32C4, o, R.F32C4)
    assert np.isnan(row[:4]).all() and row[4] == 1 and row[5] == 9
    pred, ce = R.logit_stats(np.array([[1., 7., 7.], [np.nan, 1., 2.]], np.float32), 2)
    assert pred.tolist() == [1, -1] and np.isnan(ce[1]) and abs(ce[0] - np.log(2 + np.exp(-6.))) < 1e-15
    rec = R.fold(np.zeros(R.RECORD), np.array([[3., 0., 6., 18., 2., 9.]]), pred[:1], ce[:1], 3)
    assert rec[1] == 3 and rec[2] == 0 and rec[6] == rec[7] == R.psnr_of(18., 9.) and rec[17] == 1
    msg = R.report(R.fold(rec, np.array([[1., 1., 9., 9., 9., 9.]]), pred[1:], ce[1:], 3), 2, 3)
    assert msg['attack acc'] == '100.0 %' and msg['2 to 1'] == '50.0 %' and msg['2 to -1'] == '50.0 %' and msg['e min'] == 0 and msg['e max'] == 3


def test_product_report_is_the_restatements(g25_run):
    from nerfail_amd import model_test as MT
    g, originals, attacked, rec, msg = g25_run
    assert MT.report(rec, int(g['label']), int(g['num_classes'])) == msg
    check_msg(MT.report(rec, int(g['label']), int(g['num_classes'])), g, 'report')


def test_signature_and_get_psnr(golden):
    import torch
    from nerfail_amd import model_test as MT
    g = golden('g25_eval')
    assert str(inspect.signature(MT.test_for_inception)) == str(g['signature'])
    a = torch.arange(12.).reshape(3, 4)
    assert MT.get_psnr(a, a) == R.PSNR_IDENTICAL
    assert abs(MT.get_psnr(a, a + 2) - 20 * np.log10(255. / 2.)) < 1e-12


def test_revisions():
    from nerfail_amd import _lib
    lib = _lib.load()
    assert lib.nerfail_eval_revision() == 1 == _lib.EVAL_REVISION
    assert lib.nerfail_abi_version() == 14 and lib.nerfail_abi_revision() == 15
    assert _lib.EVAL_RECORD_DOUBLES == R.RECORD == 16 + 32 and _lib.EVAL_VIEW_DOUBLES == R.VIEW
    assert (_lib.EVAL_U8C4, _lib.EVAL_U8C3, _lib.EVAL_F32C4, _lib.EVAL_FLAT) == (R.U8C4, R.U8C3, R.F32C4, R.FLAT)
    assert lib.nerfail_eval_scratch_bytes() == 16 * 128 * 5 * 8


def test_validation_without_gpu():
    """Every rule of the header is NERFAIL_EINVAL before any launch; the pointers below are never dereferenced."""
    from nerfail_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p

    def table(addr):
        return (p * 1)(addr)

    def vm(a=0x1000, fa=R.U8C4, o=0x2000, fo=R.U8C4, n=1, P=4, scratch=0x3000, rows=0x4000, cla=None, a_tab=True, o_tab=True):
        return lib.nerfail_eval_view_metrics(table(a) if a_tab else None, fa, table(o) if o_tab else None, fo, n, P, p(scratch), p(rows),
                                             p(cla) if cla else None, None)

    def err():
        return lib.nerfail_last_error()

    assert vm(n=-1) == 1 and b'negative' in err()
    assert vm(P=-1) == 1 and b'negative' in err()
    assert vm(fa=4) == 1 and b'format' in err()
    assert vm(fo=-1) == 1 and b'format' in err()
    assert vm(fa=R.FLAT) == 1 and b'FLAT' in err()
    assert vm(fo=R.FLAT) == 1 and b'FLAT pairs' in err()
    assert vm(fa=R.FLAT, fo=R.FLAT, cla=0x5000) == 1 and b'cla_in' in err()
    assert vm(n=0) == 0 and vm(P=0) == 0 and vm(n=0, a_tab=False, o_tab=False, scratch=None, rows=None) == 0      # no-ops
    assert vm(a_tab=False) == 1 and b'NULL' in err()
    assert vm(o_tab=False) == 1 and b'NULL' in err()
    assert vm(scratch=None) == 1 and b'NULL' in err()
    assert vm(rows=None) == 1 and b'NULL' in err()
    assert vm(a=0) == 1 and b'NULL' in err()
    assert vm(o=0) == 1 and b'NULL' in err()
    for fmt, bad, ok in ((R.U8C4, 0x1002, 0x1004), (R.U8C3, 0x1001, 0x1004), (R.F32C4, 0x1008, None), (R.F32C4, 0x1004, None)):
        assert vm(a=bad, fa=fmt) == 1 and b'attacked view is not aligned' in err(), fmt
        assert vm(o=bad, fo=fmt) == 1 and b'original view is not aligned' in err(), fmt
    assert vm(a=0x1002, fa=R.FLAT, fo=R.FLAT) == 1 and b'aligned' in err()
    assert vm(cla=0x5002) == 1 and b'cla_in' in err()
    assert vm(rows=0x4004) == 1 and b'8-byte' in err()
    ls = lib.nerfail_eval_logit_stats
    assert ls(None, -1, 8, 0, None, None, None) == 1 and b'negative' in err()
    assert ls(None, 2, 0, 0, None, None, None) == 1 and b'1..32' in err()
    assert ls(None, 2, 33, 0, None, None, None) == 1 and b'1..32' in err()
    assert ls(None, 2, 8, 8, None, None, None) == 1 and b'label' in err()
    assert ls(None, 2, 8, -1, None, None, None) == 1 and b'label' in err()
    assert ls(None, 2, 8, 0, None, None, None) == 1 and b'NULL' in err()
    assert ls(None, 0, 8, 0, None, None, None) == 0
    fold = lib.nerfail_eval_fold
    assert fold(None, None, None, -1, 8, None, None) == 1 and b'negative' in err()
    assert fold(None, None, None, 2, 0, None, None) == 1 and fold(None, None, None, 2, 33, None, None) == 1 and b'1..32' in err()
    assert fold(None, None, None, 2, 8, None, None) == 1 and b'NULL' in err()
    assert fold(None, None, None, 0, 8, None, None) == 0
