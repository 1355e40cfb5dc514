"""-m gpu: the victim-training kernels (nerfail_amd/csrc/cls_train.hip, include/nerfail_hip.h "victim training") against their
restatement tests/cls_train_ref.py: the batch assembly bitwise, with canaries and one run under guard pages; the cross entropy,
its gradient and the stats row; the SGD step bitwise and the weight image against nerfail_cnn_pack; opcheck of the four ops."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import cls_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
CANARY = 64


def _dev():
    return torch.device('cuda:0')


def _ops():
    import nerfail_amd.ops as O
    return O


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ 1. batch assembly
def store(N, H, W, ch, seed):
    """uint8 [N,H*W,ch]; four-channel: about half the pixels alpha 0, all with non-white garbage rgb."""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 255, size=(N, H * W, ch)).astype(np.uint8)
    if ch == 4:
        img[..., 3] = rs.randint(0, 3, size=(N, H * W)) * 127            # 0, 127, 254
    return img, rs.randint(0, 8, size=N).astype(np.int32)


def cls_batch_with_canaries(img, labels_all, idx):
    """nerfail_cls_batch through the C ABI into the middle of larger buffers: (x, labels, canaries intact?)."""
    from nerfail_amd import _lib
    lib, dev = _lib.load(), _dev()
    N, P, ch = img.shape
    B = len(idx)
    st, la = torch.from_numpy(img).to(dev), torch.from_numpy(labels_all).to(dev)
    ix = torch.tensor(idx, dtype=torch.int64, device=dev)
    xbuf = torch.full((B * 3 * P + 2 * CANARY,), -7.5, dtype=torch.float32, device=dev)
    lbuf = torch.full((B + 2 * CANARY,), -77, dtype=torch.int32, device=dev)
    x, lb = xbuf[CANARY:CANARY + B * 3 * P], lbuf[CANARY:CANARY + B]
    _lib.check(lib.nerfail_cls_batch(_lib.dev(st), _lib.EVAL_U8C4 if ch == 4 else _lib.EVAL_U8C3, _lib.dev(la), N, P, _lib.dev(ix), B,
                                     ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(lb.data_ptr()), _lib.stream()))
    torch.cuda.synchronize()
    intact = bool((xbuf[:CANARY] == -7.5).all() and (xbuf[-CANARY:] == -7.5).all() and (lbuf[:CANARY] == -77).all()
                  and (lbuf[-CANARY:] == -77).all())
    return x.view(B, 3, P).cpu().numpy(), lb.cpu().numpy(), intact


N_STORE = 4
BATCHES = {'B1_last': [N_STORE - 1], 'B3_repeat_oob': [2, 2, N_STORE], 'B3_neg_first_last': [-1, 0, N_STORE - 1]}


@pytest.mark.parametrize('hw', [(766, 766), (767, 767), (769, 772)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('ch', [4, 3], ids=['U8C4', 'U8C3'])
def test_batch_is_bitwise_the_restatement(hw, ch):
    img, labels_all = store(N_STORE, hw[0], hw[1], ch, seed=hw[0] + ch)
    for name, idx in BATCHES.items():
        want_x, want_l = R.batch(img, labels_all, idx)
        x, lb, intact = cls_batch_with_canaries(img, labels_all, idx)
        assert intact, name
        assert np.array_equal(lb, want_l), (name, lb, want_l)
        assert np.array_equal(x.view(np.int32), want_x.view(np.int32)), name     # bitwise, NaN views included
        assert np.isnan(x[[i for i, v in enumerate(idx) if not 0 <= v < N_STORE]]).all()


def test_batch_op_shapes_and_tiny_views():
    """The op keeps the store's spatial dims; views smaller than a wide load (P = 1, 2, 5) take the scalar paths only."""
    O, dev = _ops(), _dev()
    for P, ch in ((1, 3), (2, 3), (5, 3), (1, 4), (3, 4), (5, 4)):
        img, la = store(3, 1, P, ch, seed=P * ch)
        x, lb = O.cls_batch(torch.from_numpy(img).to(dev).view(3, 1, P, ch), torch.from_numpy(la).to(dev),
                            torch.tensor([2, 1, 0, 2], device=dev))
        assert tuple(x.shape) == (4, 3, 1, P)
        want_x, want_l = R.batch(img, la, [2, 1, 0, 2])
        assert np.array_equal(x.cpu().numpy().reshape(4, 3, P), want_x) and np.array_equal(lb.cpu().numpy(), want_l)


def test_batch_under_guard_pages(rank_launcher):
    """The (767, 767) U8C3 case - every view but view 0 misaligned - with unmapped pages behind the store."""
    rep = rank_launcher(os.path.abspath(__file__), 1, [], timeout=300, env={'NERFAIL_GUARD_ALLOC': '1'})
    log = '\n'.join(rep['logs'])
    assert rep['rc'] == [0], log
    assert 'Memory access fault' not in log and '[guard_alloc] active' in log and 'CLS BATCH GUARD OK' in log, log


def _guard_child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import guard
    assert guard.install_if_wanted()
    O, dev = _ops(), _dev()
    img, la = store(N_STORE, 767, 767, 3, seed=9)
    st, lt = torch.from_numpy(img).to(dev), torch.from_numpy(la).to(dev)
    for idx in BATCHES.values():
        x, lb = O.cls_batch(st, lt, torch.tensor(idx, device=dev))
        want_x, want_l = R.batch(img, la, idx)
        assert np.array_equal(x.cpu().numpy().view(np.int32), want_x.view(np.int32)) and np.array_equal(lb.cpu().numpy(), want_l)
    torch.cuda.synchronize()
    print('CLS BATCH GUARD OK', flush=True)


# ------------------------------------------------------------------------------------------------------------ 2. cross entropy
def ce_inputs(B, C, seed):
    rs = np.random.RandomState(seed)
    z = (rs.standard_normal((B, C)) * 4).astype(np.float32)
    return z, rs.randint(0, C, size=B).astype(np.int32)


def f64_definition(z, y):
    zt = torch.from_numpy(z).double().requires_grad_(True)
    torch.nn.functional.cross_entropy(zt, torch.from_numpy(y).long()).backward()
    return zt.grad.numpy(), torch.nn.functional.cross_entropy(zt.detach(), torch.from_numpy(y).long(), reduction='sum').item()


@pytest.mark.parametrize('B,C', [(5, 1), (16, 8), (70, 32)])
def test_ce_gradient_and_row(B, C):
    O, dev = _ops(), _dev()
    z, y = ce_inputs(B, C, seed=B + C)
    z2, y2 = ce_inputs(3, C, seed=B)
    rows = []
    for _ in range(2):                                           # two runs: the same bits
        row = torch.zeros(16, device=dev)
        row[4:] = 3.25                                           # [4..15] are left alone
        d = O.cls_ce(torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev), row, True)
        mid = row.clone()
        e = O.cls_ce(torch.from_numpy(z2).to(dev), torch.from_numpy(y2).to(dev), row, False)     # NULL d_logits
        assert e.numel() == 0
        rows.append((bits(d), bits(mid), bits(row)))
    assert all(torch.equal(a, b) for a, b in zip(*rows))
    want, ce_sum = f64_definition(z, y)
    got = d.cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print('B=%d C=%d: worst gradient error %.2f ulp' % (B, C, float((np.abs(got - want) / ulp).max())))
    assert (np.abs(got - want) <= ulp).all()                     # one float32 rounding of the float64 definition
    ref_row = np.zeros(16, np.float32)
    ref_d = R.ce(z, y, ref_row)
    assert (np.abs(got - ref_d.astype(np.float64)) <= ulp).all()
    m = mid.cpu().numpy()
    assert abs(float(m[0]) + float(m[1]) - ce_sum) <= 1e-12 * max(1.0, abs(ce_sum)) and m[0] == ref_row[0]
    assert m[2] == ref_row[2] == float((z.argmax(1) == y).sum()) and m[3] == B and (m[4:] == 3.25).all()
    R.ce(z2, y2, ref_row, want_grad=False)                       # the second batch accumulated in stream order
    r = row.cpu().numpy()
    assert abs(float(r[0]) + float(r[1]) - R.pair_get(ref_row, 0)) <= 1e-12 * max(1.0, abs(ce_sum))
    assert r[2] == ref_row[2] and r[3] == B + 3 and (r[4:] == 3.25).all()


def test_ce_special_rows():
    O, dev = _ops(), _dev()
    z = np.array([[1, 5, 5, 0], [np.nan, 1, 2, 3], [0, 1, 2, 3], [4, 4, 4, 4]], np.float32)
    y = np.array([2, 3, 7, 0], np.int32)                         # equal maxima (first wins: wrong), NaN row, bad label, all equal
    row = torch.zeros(16, device=dev)
    d = O.cls_ce(torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev), row, True).cpu().numpy()
    r = row.cpu().numpy()
    assert np.isnan(d[1]).all() and np.isnan(d[2]).all() and np.isfinite(d[[0, 3]]).all()
    assert np.isnan(r[0]) and r[1] == 0 and r[2] == 1 and r[3] == 4
    ref_row = np.zeros(16, np.float32)
    ref_d = R.ce(z, y, ref_row)
    assert np.allclose(d[[0, 3]], ref_d[[0, 3]], rtol=2e-7, atol=0)


# ------------------------------------------------------------------------------------------------------------ 3. SGD + image
def pack_of(flat, C):
    """nerfail_cnn_pack of the parameters in a flat buffer, into an image pre-filled with a sentinel."""
    from nerfail_amd import _lib
    lib = _lib.load()
    layout, _ = R.grad_layout(C)
    ptrs = (ctypes.c_void_p * 18)(*[flat.data_ptr() + 4 * o for o, _ in layout])
    img = torch.full((lib.nerfail_cnn_packed_floats(C),), -123.0, dtype=torch.float32, device=flat.device)
    _lib.check(lib.nerfail_cnn_pack(ptrs, C, _lib.dev(img), _lib.stream()))
    return img


@pytest.mark.parametrize('C', [8, 24])
def test_sgd_step_and_image(C):
    import cnn_inputs as CI
    O, dev = _ops(), _dev()
    layout, total = R.grad_layout(C)
    mask = R.layout_mask(C)
    p = np.full(total, 7.0, np.float32)                          # 7: the padding floats, which must stay
    for (o, _), v in zip(layout, CI.state_dict(31 + C, C).values()):
        p[o:o + v.size] = v.reshape(-1)
    rs = np.random.RandomState(C)
    buf = np.full(total, 9.0, np.float32)                        # garbage: `first` must overwrite, not read, it
    tp, tbuf = torch.from_numpy(p.copy()).to(dev), torch.from_numpy(buf.copy()).to(dev)
    image = pack_of(tp, C)
    written = (image != -123.0).cpu().numpy()                    # the non-padding floats of the image: what pack writes
    assert written.sum() > mask.sum()
    for t in range(3):
        g = (rs.standard_normal(total) * np.exp(rs.uniform(-6, 3, total))).astype(np.float32)
        g[~mask] = np.nan                                        # the gradient's padding is never read
        pm, bm = p[mask], buf[mask]
        R.sgd_step(pm, g[mask], bm, 0.001, 0.9, first=(t == 0))
        p[mask], buf[mask] = pm, bm
        O.cnn_sgd_step(tp, torch.from_numpy(g).to(dev), tbuf, image, C, 0.001, 0.9, t == 0)
        assert np.array_equal(tp.cpu().numpy().view(np.int32), p.view(np.int32)), 'parameters, step %d' % (t + 1)
        assert np.array_equal(tbuf.cpu().numpy().view(np.int32), buf.view(np.int32)), 'momentum, step %d' % (t + 1)
        fresh = pack_of(tp, C)
        same = (bits(image) == bits(fresh)).numpy()
        assert same[written].all(), 'image, step %d: %d floats differ' % (t + 1, int((~same[written]).sum()))
        assert (image.cpu().numpy()[~written] == -123.0).all(), 'image padding written'
    assert (p[~mask] == 7.0).all() and (buf[~mask] == 9.0).all()


def test_sgd_step_refuses_bad_buffers():
    from nerfail_amd import _lib
    lib, dev = _lib.load(), _dev()
    n, k = lib.nerfail_cnn_grad_floats(8), lib.nerfail_cnn_packed_floats(8)
    a, b, c = (torch.zeros(n + 4, device=dev) for _ in range(3))
    img = torch.zeros(k + 4, device=dev)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)      # noqa: E731
    for args in ((ptr(a, 4), ptr(b), ptr(c), ptr(img)), (ptr(a), ptr(b, 4), ptr(c), ptr(img)), (ptr(a), ptr(b), ptr(c, 8), ptr(img)),
                 (ptr(a), ptr(b), ptr(c), ptr(img, 4)), (None, ptr(b), ptr(c), ptr(img)), (ptr(a), ptr(b), ptr(c), None)):
        assert lib.nerfail_cnn_sgd_step(*args, 8, 0.001, 0.9, 1, _lib.stream()) == 1
    torch.cuda.synchronize()
    assert float(a.abs().sum() + c.abs().sum() + img.abs().sum()) == 0.0          # nothing was launched


# ------------------------------------------------------------------------------------------------------------ 1d. epoch close
def test_epoch_close_matches_the_restatement():
    O, dev = _ops(), _dev()
    best, ref_best = torch.tensor([0., -1.]).to(dev), np.array([0, -1], np.float32)
    flag, rec = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(16, device=dev)
    cases = [(0, 2, 3.7), (1, 2, 2.9), (1, 2, 2.5), (float('nan'), 2, 2.0), (2, 2, 1.0)]       # none, take, tie, NaN, take
    for epoch, (correct, views, ce_sum) in enumerate(cases):
        rows = []
        for cs, c in ((6.123456789, 2), (ce_sum, correct)):
            r = np.zeros(16, np.float32)
            R.pair_put(r, 0, cs)
            r[2], r[3] = c, views
            rows.append(r)
        want, want_flag = R.epoch_close(rows[0], rows[1], 5, 3, ref_best, epoch)
        O.cls_epoch_close(torch.from_numpy(rows[0]).to(dev), torch.from_numpy(rows[1]).to(dev), 5, 3, best, epoch, rec, flag)
        assert int(flag.item()) == want_flag == [0, 1, 0, 0, 1][epoch]
        assert np.array_equal(rec.cpu().numpy().view(np.int32), want.view(np.int32)), (epoch, rec.cpu().numpy(), want)
        assert np.array_equal(best.cpu().numpy(), ref_best)


# ------------------------------------------------------------------------------------------------------------ 8. opcheck
def test_cls_ops_pass_opcheck():
    O, dev = _ops(), _dev()
    assert set(O.CLS_OPS) == {'cls_batch', 'cls_ce', 'cnn_bwd_weights_into', 'cnn_sgd_step', 'cls_epoch_close'}
    ops = torch.ops.nerfail_mi
    tests = ('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_static')
    img, la = store(2, 1, 5, 3, seed=1)
    z, y = ce_inputs(2, 8, seed=2)
    from nerfail_amd import _lib
    lib = _lib.load()
    n, k = lib.nerfail_cnn_grad_floats(1), lib.nerfail_cnn_packed_floats(1)
    cases = {
        'cls_batch': (torch.from_numpy(img).to(dev), torch.from_numpy(la).to(dev), torch.tensor([1, 0], device=dev)),
        'cls_ce': (torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev), torch.zeros(16, device=dev), True),
        'cnn_sgd_step': (torch.zeros(n, device=dev), torch.ones(n, device=dev), torch.zeros(n, device=dev), torch.zeros(k, device=dev),
                         1, 0.001, 0.9, True),
        'cls_epoch_close': (torch.ones(16, device=dev), torch.ones(16, device=dev), 5, 3, torch.tensor([0., -1.]).to(dev), 0,
                            torch.zeros(16, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)),
    }
    import cnn_inputs as CI
    import cls_inputs as XI
    from nerfail_amd.MyModel import MyCNN
    m = MyCNN(8, trainable=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CI.state_dict(3, 8).items()})
    m = m.to(dev)
    x = torch.from_numpy(XI.white_nchw(XI.views(77, (2,))[0])).to(dev)
    logits, ws, masks = O.cnn_fwd(m.packed(), x, 8, True)
    d = O.cls_ce(logits, torch.tensor([2], dtype=torch.int32, device=dev), torch.zeros(16, device=dev), True)
    into = torch.zeros(lib.nerfail_cnn_grad_floats(8), device=dev)
    scratch = torch.empty(O.cnn_bwd_weights_scratch_floats(1, XI.H, XI.W, 8) + 5, device=dev)       # larger is fine
    O.cnn_bwd_weights_into(m.packed(), x, ws, masks, d, scratch, into)
    assert torch.equal(into, O.cnn_bwd_weights(m.packed(), x, ws, masks, d, False)[0])               # bitwise the allocating op
    cases['cnn_bwd_weights_into'] = (m.packed(), x, ws, masks, d, scratch, into)
    for name in O.CLS_OPS:
        res = torch.library.opcheck(getattr(ops, name).default, cases[name], test_utils=tests)
        assert all(v == 'SUCCESS' for v in res.values()), (name, res)


if __name__ == '__main__':
    _guard_child()
