"""-m gpu: the 2-D baseline kernels (nerfail_amd/csrc/u2d.hip, include/nerfail_hip.h "2-D baseline") against their numpy
restatement tests/igsm2d_ref.py, bit for bit: the forward at every size at which a view is cut differently (scalar head and
tail, whole quads, more than one workgroup), for both store formats, per-view and shared r, every combination of outputs,
elements sitting on and one ulp outside the clip's bounds, NaN, out-of-range indices, the store at the end of its allocation
and canaries around every output; the step with every kind of gradient, rows on the epsilon bounds, r_init NULL / zero /
non-zero, both directions, untouched rows; the image-loss statistic and the strict epoch close."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import attack_loop_ref as R
import igsm2d_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
CANARY = 64
N_STORE = 7
SIZES = (1, 3, 63, 64, 65, 29 * 37, 257, 258, 259, 4 * 512 * 3 + 5)     # from 29 * 37 on a lane takes a second quad; the last: 4 workgroups per view
BATCHES = ([6], [6, 2, 0, 5, 3])
NAN = np.float32(np.nan)


def _dev():
    return torch.device('cuda:0')


def same(a, b):
    """Bitwise equal, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


def store(P, ch, seed):
    """uint8 [7,P,ch]; four-channel: about a third of the pixels alpha 0, all with non-white garbage rgb. The first pixels of
    view 2 and of view 6 (when there are that many) are pinned for the boundary elements of boundary_r()."""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 255, size=(N_STORE, P, ch)).astype(np.uint8)
    if ch == 4:
        img[..., 3] = rs.randint(0, 3, size=(N_STORE, P)) * 127
    for v in (2, 6):
        for p, rgb in enumerate(((0, 10, 255), (200, 255, 0), (10, 200, 255))[:P]):
            img[v, p, :3] = rgb
            if ch == 4:
                img[v, p, 3] = 255
    return img


def boundary_r(P, seed, shared=False):
    """r in [-300, 300] (both clip bounds are crossed often), a few NaN, and on the pinned pixels of views 2 and 6: sums exactly
    0 and exactly 255, one ulp outside either, a sum that only rounding brings back to 255, and NaN."""
    rs = np.random.RandomState(seed)
    r = rs.uniform(-300, 300, size=(P, 3) if shared else (N_STORE, P, 3)).astype(np.float32)
    r.reshape(-1)[rs.randint(0, r.size, size=max(1, r.size // 50))] = NAN
    pins = (((0, 10, 255), (0., -10., 0.)),                                # 0 + 0 = 0, 10 - 10 = 0, 255 + 0 = 255: all inside
            ((200, 255, 0), (55., np.float32(1.5258789e-05), -1e-30)),      # exactly 255; one ulp above 255; just below 0
            ((10, 200, 255), (np.nextafter(np.float32(-10), np.float32(-20)), np.nextafter(np.float32(55), np.float32(60)), NAN)))
    for p, (_, vals) in enumerate(pins[:P]):
        if shared:
            r[p] = vals
        else:
            r[2, p] = r[6, p] = vals
    return r


def fwd(img, idx, r, shared, want):
    """nerfail_u2d_fwd through the C ABI: the store in the LAST bytes of its allocation, every output in the middle of a
    canary-padded buffer. want = (x_rgb, cls_in, mask) booleans. Returns the outputs (None where not wanted) and whether every
    canary is intact."""
    from nerfail_amd import _lib
    lib, dev = _lib.load(), _dev()
    N, P, ch = img.shape
    B = len(idx)
    nbytes = img.size
    pad = 4096                                                             # the store starts 16-byte aligned and ends the allocation
    sbuf = torch.zeros((pad + nbytes,), dtype=torch.uint8, device=dev)
    sbuf[pad:] = torch.from_numpy(img.reshape(-1)).to(dev)
    st = sbuf[pad:]
    assert st.data_ptr() % 16 == 0
    ix = torch.tensor(idx, dtype=torch.int64, device=dev)
    rt = torch.from_numpy(r).to(dev)
    xbuf = torch.full((B * 3 * P + 2 * CANARY,), -7.5, dtype=torch.float32, device=dev)
    cbuf = torch.full((B * 3 * P + 2 * CANARY,), -7.5, dtype=torch.float32, device=dev)
    mbuf = torch.full((B * P + 2 * CANARY,), 99, dtype=torch.uint8, device=dev)
    x, c, m = xbuf[CANARY:CANARY + B * 3 * P], cbuf[CANARY:CANARY + B * 3 * P], mbuf[CANARY:CANARY + B * P]
    ptr = lambda t, on: ctypes.c_void_p(t.data_ptr()) if on else None     # noqa: E731
    _lib.check(lib.nerfail_u2d_fwd(ctypes.c_void_p(st.data_ptr()), _lib.EVAL_U8C4 if ch == 4 else _lib.EVAL_U8C3, N, P, _lib.dev(ix), B,
                                   _lib.dev(rt), int(shared), ptr(x, want[0]), ptr(c, want[1]), ptr(m, want[2]), _lib.stream()))
    torch.cuda.synchronize()
    intact = all(bool((buf[:CANARY] == v).all() and (buf[-CANARY:] == v).all()) for buf, v in ((xbuf, -7.5), (cbuf, -7.5), (mbuf, 99)))
    for buf, v, on in ((x, -7.5, want[0]), (c, -7.5, want[1]), (m, 99, want[2])):
        if not on:
            intact = intact and bool((buf == v).all())                     # an output that was not asked for is not written
    return (x.view(B, P, 3).cpu().numpy() if want[0] else None, c.view(B, 3, P).cpu().numpy() if want[1] else None,
            m.view(B, P).cpu().numpy() if want[2] else None, intact)


@pytest.mark.parametrize('ch', (4, 3))
@pytest.mark.parametrize('P', SIZES)
def test_forward_bitwise(P, ch):
    img = store(P, ch, seed=P + ch)
    for shared in (False, True):
        r = boundary_r(P, seed=3 * P + shared, shared=shared)
        for idx in BATCHES:
            want_x, want_c, want_m = IR.u2d_fwd(img, idx, r, shared)
            for want in ((True, False, False), (False, True, False), (False, True, True), (True, True, True)):
                x, c, m, intact = fwd(img, idx, r, shared, want)
                assert intact, (P, ch, shared, idx, want)
                assert x is None or same(x, want_x), (P, ch, shared, idx, want)
                assert c is None or same(c, want_c), (P, ch, shared, idx, want)
                assert m is None or np.array_equal(m, want_m), (P, ch, shared, idx, want)


def test_forward_boundary_elements_are_what_the_header_says():
    """The pinned pixels of view 2, spelled out: inside on 0 and on 255, outside one ulp beyond, NaN never passes and stays."""
    img = store(65, 4, seed=1)
    x, c, m, _ = fwd(img, [2], boundary_r(65, seed=1), False, (True, True, True))
    assert x[0, 0].tolist() == [0., 0., 255.] and m[0, 0] == 7
    assert x[0, 1].tolist() == [255., 255., 0.] and m[0, 1] == 1           # 200 + 55 inside; 255 + ulp and 0 - 1e-30 outside
    assert x[0, 2, 0] == 0. and x[0, 2, 1] == 255. and np.isnan(x[0, 2, 2]) and m[0, 2] == 2   # -10.000001 + 10 < 0; 200 + 55.000004 rounds to 255
    assert same(c[0].T, x[0])


@pytest.mark.parametrize('ch', (4, 3))
def test_forward_out_of_range_index(ch):
    P = 259
    img, r = store(P, ch, seed=5), boundary_r(P, seed=6)
    idx = [3, -1, 7, 0]
    want_x, want_c, want_m = IR.u2d_fwd(img, idx, r)
    x, c, m, intact = fwd(img, idx, r, False, (True, True, True))
    assert intact and same(x, want_x) and same(c, want_c) and np.array_equal(m, want_m)
    assert np.isnan(x[1]).all() and np.isnan(c[2]).all() and not m[1:3].any()


def test_under_guard_pages(rank_launcher):
    """Forward, statistic and step at 767 x 767 on a U8C3 store - every view but view 0 misaligned - and on a U8C4 one, each
    tensor ending its own mapping with unmapped pages behind it (tests/guard)."""
    rep = rank_launcher(os.path.abspath(__file__), 1, [], timeout=300, env={'NERFAIL_GUARD_ALLOC': '1'})
    log = '\n'.join(rep['logs'])
    assert rep['rc'] == [0], log
    assert 'Memory access fault' not in log and '[guard_alloc] active' in log and 'U2D GUARD OK' in log, log


def _guard_child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import guard
    assert guard.install_if_wanted()
    import nerfail_amd.ops as O
    from nerfail_amd import _lib
    dev = _dev()
    P = 767 * 767
    for ch in (3, 4):
        img, r = store(P, ch, seed=9), boundary_r(P, seed=10)
        st, rt = torch.from_numpy(img.reshape(N_STORE, 767, 767, ch)).to(dev), torch.from_numpy(r.reshape(N_STORE, 767, 767, 3)).to(dev)
        scratch = torch.empty((_lib.load().nerfail_img_sqerr_scratch_bytes() // 8,), dtype=torch.float64, device=dev)
        for idx in BATCHES:
            ix = torch.tensor(idx, dtype=torch.int64, device=dev)
            x, c, m = O.u2d_fwd(st, ix, rt, True, True, True)
            wx, wc, wm = IR.u2d_fwd(img, idx, r)
            assert same(x.cpu().numpy().reshape(wx.shape), wx) and same(c.cpu().numpy().reshape(wc.shape), wc)
            assert np.array_equal(m.cpu().numpy().reshape(wm.shape), wm)
            O.u2d_sqerr(torch.nan_to_num(x), st, ix, scratch, torch.zeros((16,), dtype=torch.float32, device=dev))
            d = torch.randn_like(c)
            table = rt.clone()
            O.u2d_step(table, ix, d, m, None, 8., 24., False)
            want = IR.u2d_step(r, idx, d.cpu().numpy().reshape(len(idx), 3, P), wm, None, 8., 24., False)
            assert same(table.cpu().numpy().reshape(want.shape), want)
    torch.cuda.synchronize()
    print('U2D GUARD OK', flush=True)


# ------------------------------------------------------------------------------------------------------------ the step
def step_inputs(P, B_idx, seed, eps, init):
    """Table, init, gradient and mask. Gradient elements cycle through +x, -x, +0, -0, NaN; every mask pattern occurs; the
    first rows of every view sit exactly on init - eps / init + eps."""
    rs = np.random.RandomState(seed)
    B = len(B_idx)
    r0 = (rs.randint(-3, 4, size=(N_STORE, P, 3)) * 8).astype(np.float32)
    r_init = None if init is None else (np.zeros_like(r0) if init == 'zero' else (rs.randint(-2, 3, size=r0.shape) * 4).astype(np.float32))
    base = np.zeros_like(r0) if r_init is None else r_init
    r = np.clip(r0 + base, base - eps, base + eps).astype(np.float32)
    flat = r.reshape(N_STORE, -1)
    k = min(flat.shape[1], 10)
    flat[:, :k:2] = (base.reshape(N_STORE, -1)[:, :k:2] - np.float32(eps))
    flat[:, 1:k:2] = (base.reshape(N_STORE, -1)[:, 1:k:2] + np.float32(eps))
    mag = rs.uniform(1e-8, 5, size=(B, 3, P)).astype(np.float32)
    kind = (np.arange(B * 3 * P).reshape(B, 3, P) + seed) % 5
    d = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [mag, -mag, np.float32(0.), np.float32(-0.)], NAN).astype(np.float32)
    mask = rs.randint(0, 8, size=(B, P)).astype(np.uint8)
    return r, r_init, d, mask


def step(r, r_init, idx, d, mask, a, eps, targeted):
    from nerfail_amd import _lib
    lib, dev = _lib.load(), _dev()
    N, P = r.shape[:2]
    rbuf = torch.full((r.size + 2 * CANARY,), -7.5, dtype=torch.float32, device=dev)
    rt = rbuf[CANARY:CANARY + r.size]
    rt.copy_(torch.from_numpy(r.reshape(-1)).to(dev))
    it = None if r_init is None else torch.from_numpy(r_init).to(dev)
    ix = torch.tensor(idx, dtype=torch.int64, device=dev)
    dt, mt = torch.from_numpy(d).to(dev), torch.from_numpy(mask).to(dev)
    _lib.check(lib.nerfail_u2d_step(ctypes.c_void_p(rt.data_ptr()), N, P, _lib.dev(ix), len(idx), _lib.dev(dt), _lib.dev(mt),
                                    _lib.dev(it), a, eps, int(targeted), _lib.stream()))
    torch.cuda.synchronize()
    intact = bool((rbuf[:CANARY] == -7.5).all() and (rbuf[-CANARY:] == -7.5).all())
    return rt.view(N, P, 3).cpu().numpy(), intact


@pytest.mark.parametrize('targeted', (False, True))
@pytest.mark.parametrize('P', SIZES)
def test_step_bitwise(P, targeted):
    a, eps = 8., 24.
    for init in (None, 'zero', 'random'):
        for idx in BATCHES:
            r, r_init, d, mask = step_inputs(P, idx, seed=P + len(idx), eps=eps, init=init)
            got, intact = step(r, r_init, idx, d, mask, a, eps, targeted)
            want = IR.u2d_step(r, idx, d, mask, r_init, a, eps, targeted)
            assert intact and same(got, want), (P, targeted, init, idx)
            others = [v for v in range(N_STORE) if v not in idx]
            assert same(got[others], r[others])                            # every non-indexed row unchanged, bitwise
            if init is None:                                               # r_init NULL: the bits of a zero tensor
                got0, _ = step(r, np.zeros_like(r), idx, d, mask, a, eps, targeted)
                assert same(got, got0)


def test_step_rows_on_the_bounds_and_bad_indices():
    """A row on init + eps pushed outward stays, pushed inward moves by a; NaN gradients and masked gradients do not move it;
    a NaN in the table stays; indices outside the table are skipped."""
    P, a, eps = 5, 8., 24.
    r = np.zeros((N_STORE, P, 3), np.float32)
    r[1, :, 0], r[1, :, 1], r[1, 0, 2] = eps, -eps, NAN
    d = np.zeros((3, 3, P), np.float32)
    d[1, 0], d[1, 1] = [1., -1., NAN, 0., 2.], [-1., 1., 1., -0., -2.]
    mask = np.full((3, P), 7, np.uint8)
    mask[1, 4] = 0
    got, intact = step(r, None, [-5, 1, 7], d, mask, a, eps, False)
    assert intact and same(got, IR.u2d_step(r, [-5, 1, 7], d, mask, None, a, eps, False))
    assert got[1, :, 0].tolist() == [eps, eps - a, eps, eps, eps] and got[1, :, 1].tolist() == [-eps, -eps + a, -eps + a, -eps, -eps]
    assert np.isnan(got[1, 0, 2]) and same(got[[0, 2, 3, 4, 5, 6]], r[[0, 2, 3, 4, 5, 6]])


# ------------------------------------------------------------------------------------------------------------ statistic and close
def sqerr_row(x, img, idx):
    import nerfail_amd.ops as O
    from nerfail_amd import _lib
    dev = _dev()
    row = torch.zeros((16,), dtype=torch.float32, device=dev)
    scratch = torch.empty((_lib.load().nerfail_img_sqerr_scratch_bytes() // 8,), dtype=torch.float64, device=dev)
    O.u2d_sqerr(torch.from_numpy(x).to(dev), torch.from_numpy(img).to(dev), torch.tensor(idx, dtype=torch.int64, device=dev), scratch, row)
    return row.cpu().numpy()


@pytest.mark.parametrize('P', (1, 65, 29 * 37, 5000))
def test_sqerr_against_float64_and_formats_agree(P):
    rs = np.random.RandomState(P)
    img3 = rs.randint(0, 256, size=(N_STORE, P, 3)).astype(np.uint8)
    img4 = np.concatenate([img3, rs.randint(1, 256, size=(N_STORE, P, 1)).astype(np.uint8)], -1)     # alpha > 0: the same values
    for idx in ([6, 2, 0, 5, 3], [i % N_STORE for i in range(20)]):       # 20 views: two launches of the statistic
        x = (rs.uniform(0, 255, size=(len(idx), P, 3))).astype(np.float32)
        r3, r4 = sqerr_row(x, img3, idx), sqerr_row(x, img4, idx)
        assert np.array_equal(r3.view(np.int32), r4.view(np.int32))
        s, n = IR.u2d_sqerr(x, img3, idx)
        assert abs(R.unpair(r3, 7) - s) <= 1e-12 * s and R.unpair(r3, 9) == n == 3 * P * len(idx)
        assert not r3[[0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15]].any()
    white = img4.copy()
    white[..., 3] = 0                                                      # transparent everywhere: every original is white
    s, _ = IR.u2d_sqerr(x[:2], white, [1, 4])
    assert abs(R.unpair(sqerr_row(x[:2], white, [1, 4]), 7) - s) <= 1e-12 * s and s == float(((x[:2].astype(np.float64) - 255.) ** 2).sum())


@pytest.mark.parametrize('targeted', (False, True))
def test_epoch_close_is_strict_where_the_nerfail_s_close_is_not(targeted):
    import nerfail_amd.ops as O
    dev = _dev()
    row = np.zeros(16, np.float32)
    row = R.add_to_row(row, stats=(3.5, 7.25, 4, 2, 4), sqerr=(1234.5, 4 * 3 * 64))
    best0 = np.array([0.5, 1.25, 0., 0.], np.float32)                      # the best so far has THIS epoch's accuracy: a tie
    out = {}
    for name, fn in (('strict', O.u2d_epoch_close), ('lax', torch.ops.nerfail_mi.attack_epoch_close)):
        best = torch.from_numpy(best0.copy()).to(dev)
        rec = torch.zeros((16,), dtype=torch.float32, device=dev)
        flag = torch.full((1,), -1, dtype=torch.int32, device=dev)
        fn(torch.from_numpy(row).to(dev), best, 3, targeted, rec, flag)
        out[name] = (rec.cpu().numpy(), best.cpu().numpy(), int(flag.item()))
    rec, best, take = IR.epoch_close_strict(row, best0, 3, targeted)
    assert not take and out['strict'][2] == 0 and out['lax'][2] == 1
    assert np.array_equal(out['strict'][0], rec) and np.array_equal(out['strict'][1], best) and np.array_equal(best, best0)
    lax = R.epoch_close(row, best0, 3, targeted)
    assert np.array_equal(out['lax'][0], lax[0]) and np.array_equal(out['lax'][1], lax[1])
    # and a strictly better epoch is taken by both
    better = np.array([0.75 if not targeted else 0.25, 1.25, 0., 0.], np.float32)
    for fn in (O.u2d_epoch_close, torch.ops.nerfail_mi.attack_epoch_close):
        best = torch.from_numpy(better.copy()).to(dev)
        rec = torch.zeros((16,), dtype=torch.float32, device=dev)
        flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        fn(torch.from_numpy(row).to(dev), best, 3, targeted, rec, flag)
        assert int(flag.item()) == 1 and best.cpu().numpy()[:3].tolist() == [0.5, np.float32(7.25 / 4), 3.]


if __name__ == '__main__':
    _guard_child()
