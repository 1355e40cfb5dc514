"""-m gpu: the NeRFail-S epoch-statistics kernels (csrc/attack_stats.hip, ABI 15) against the numpy restatement
tests/attack_loop_ref.py. Shapes are the smallest that reach every path: one and several views per lane, quads with and without a
tail pixel, view images that are and are not 16-byte aligned, more views than one launch carries, copies with a scalar tail."""
import numpy as np
import pytest
import torch

import attack_loop_ref as R
from hiputil import T, N, dev

pytestmark = pytest.mark.gpu


def _ops():
    from nerfail_amd import ops  # noqa: F401
    return torch.ops.nerfail_mi


def _row():
    return torch.zeros(R.ROW, dtype=torch.float32, device=dev())


def _close(a, b, rel=1e-12):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= rel * max(abs(a), abs(b), 1e-300)


@pytest.mark.parametrize('B', [1, 2, 8])
@pytest.mark.parametrize('C', [2, 8, 24])
def test_logit_stats(B, C):
    rs = np.random.RandomState(100 * B + C)
    for label in (0, C - 1):
        cla = (rs.normal(size=(B, C)) * 20).astype(np.float32)
        ori = (rs.normal(size=(B, C)) * 20).astype(np.float32)
        ori[0, label] = np.abs(ori[0]).max() + 1.                 # at least one correct view
        row = _row()
        _ops().attack_logit_stats(T(cla), T(ori), label, row)
        _ops().attack_logit_stats(T(ori), T(cla), label, row)      # a second batch accumulates
        ref = R.add_to_row(R.add_to_row(np.zeros(R.ROW, np.float32), R.logit_stats(cla, ori, label)), R.logit_stats(ori, cla, label))
        got = N(row)
        assert got[4:7].tolist() == ref[4:7].tolist() and got[6] == 2 * B and got[4] >= 1          # counts: exact
        for i in (0, 2):                                           # device exp / log vs numpy's: last bits of a double
            assert _close(R.unpair(got, i), R.unpair(ref, i)), (B, C, label, i, R.unpair(got, i), R.unpair(ref, i))
        assert (got[7:] == 0).all()


def test_logit_stats_tie_nan_and_many_views():
    z = np.array([[1., 7., 7., 0.], [7., 7., 1., 0.], [np.nan, 9., 0., 0.], [0., 9., np.nan, 0.], [2., 9., 1., 0.]], np.float32)
    clean = np.zeros_like(z)
    clean[:, 1] = 5.
    for label, want in ((1, 2), (2, 0), (0, 1)):                   # first maximum wins; a NaN row never counts
        row = _row()
        _ops().attack_logit_stats(T(z), T(clean), label, row)
        got = N(row)
        assert got[5] == want and got[4] == (5 if label == 1 else 0) and got[6] == 5
        assert np.isnan(got[2]) and not np.isnan(got[0])           # the NaN rows make the attacked CE sum NaN, the clean one not
        assert got[4:7].tolist() == R.add_to_row(np.zeros(R.ROW, np.float32), R.logit_stats(z, clean, label))[4:7].tolist()
    rs = np.random.RandomState(7)                                  # more views than lanes: lane l takes views l and l + 64
    cla, ori = (rs.normal(size=(130, 8)) * 3).astype(np.float32), (rs.normal(size=(130, 8)) * 3).astype(np.float32)
    row = _row()
    _ops().attack_logit_stats(T(cla), T(ori), 3, row)
    ref = R.add_to_row(np.zeros(R.ROW, np.float32), R.logit_stats(cla, ori, 3))
    got = N(row)
    assert got[4:7].tolist() == ref[4:7].tolist()
    assert _close(R.unpair(got, 0), R.unpair(ref, 0)) and _close(R.unpair(got, 2), R.unpair(ref, 2))


@pytest.mark.parametrize('B,P', [(1, 1), (3, 1), (1, 1023), (3, 1023), (1, 1024), (3, 1024), (1, 33 * 33), (3, 33 * 33), (17, 5)])
def test_img_sqerr(B, P):
    rs = np.random.RandomState(B * 10000 + P)
    x = rs.uniform(0, 255, size=(B, P, 4)).astype(np.float32)
    ori8 = rs.randint(0, 256, size=(B, P, 4)).astype(np.uint8)
    rows = []
    for ori in (T(ori8), T(ori8.astype(np.float32)), T(ori8)):      # uint8, float32, uint8 again
        row = _row()
        _ops().img_sqerr(T(x), ori, row)
        rows.append(N(row))
    assert rows[0].tobytes() == rows[2].tobytes()                   # two runs: the same bits
    assert rows[0].tobytes() == rows[1].tobytes()                   # float32 and uint8 images: the same bits
    s, n = R.img_sqerr(x, ori8)
    got = rows[0]
    assert R.unpair(got, 9) == n and got[10] == 0                   # element count: exact
    assert _close(R.unpair(got, 7), s, 1e-13), (R.unpair(got, 7), s)  # a float64 sum in another order
    assert (got[:7] == 0).all()
    row = T(rows[0])
    _ops().img_sqerr(T(x), T(ori8), row)                            # accumulates
    assert R.unpair(N(row), 9) == 2 * n and _close(R.unpair(N(row), 7), 2 * s, 1e-13)


def test_img_sqerr_per_view_images():
    """The loop's form: every view's image an allocation of its own (resident views), through the C ABI's pointer table."""
    from nerfail_amd import _lib
    rs = np.random.RandomState(3)
    B, P = 3, 37
    x = rs.uniform(0, 255, size=(B, P, 4)).astype(np.float32)
    ori8 = rs.randint(0, 256, size=(B, P, 4)).astype(np.uint8)
    views = [T(ori8[b]) for b in range(B)]
    lib = _lib.load()
    row, xt = _row(), T(x)
    scratch = torch.empty(lib.nerfail_img_sqerr_scratch_bytes() // 8, dtype=torch.float64, device=dev())
    table = (_lib.c_p * B)(*[v.data_ptr() for v in views])
    _lib.check(lib.nerfail_img_sqerr(_lib.dev(xt), table, B, P, 1, _lib.c_p(scratch.data_ptr()), _lib.dev(row), _lib.stream()))
    one = _row()
    _ops().img_sqerr(xt, T(ori8), one)
    assert N(row).tobytes() == N(one).tobytes()


@pytest.mark.parametrize('u8', [False, True])
def test_img_sqerr_grad_add(u8):
    rs = np.random.RandomState(5)
    B, P, scale = 2, 131, np.float32(0.25 * 2 / (4 * 131 * 2))
    x = rs.uniform(0, 255, size=(B, P, 4)).astype(np.float32)
    ori = rs.randint(0, 256, size=(B, P, 4)).astype(np.uint8)
    g0 = rs.normal(size=(B, P, 4)).astype(np.float32)
    g = T(g0)
    _ops().img_sqerr_grad_add(T(x), T(ori if u8 else ori.astype(np.float32)), float(scale), g)
    want = g0 + scale * (x - ori.astype(np.float32))               # float32: one subtraction, one product, one sum
    assert want.dtype == np.float32 and np.array_equal(N(g), want)


def test_export_u8():
    k = np.arange(0, 255, dtype=np.float32)
    x = np.concatenate([k + 0.5, np.array([-3., 255.5, 300., np.nan, -0.5, 254.5, 17.49, 17.51, np.inf, -np.inf], np.float32)])
    assert x.size % 4 != 0                                          # a scalar tail behind the 128-bit body
    got = N(_ops().export_u8(T(x)))
    assert got.dtype == np.uint8 and np.array_equal(got, R.export_u8(x))
    assert got[0] == 0 and got[1] == 2 and got[2] == 2 and got[3] == 4                      # k + 0.5 goes to the even neighbour
    assert got[255:259].tolist() == [0, 255, 255, 0]                                        # -3, 255.5, 300, NaN
    img = np.random.RandomState(1).uniform(-20, 280, size=(2, 5, 7, 4)).astype(np.float32)
    assert np.array_equal(N(_ops().export_u8(T(img))), R.export_u8(img))


@pytest.mark.parametrize('targeted', [False, True])
def test_epoch_close_and_copy_if(targeted):
    """Fabricated epochs of 6 views: a better epoch, a tie (the later epoch wins and the copy happens), a worse epoch (no copy:
    the best buffer keeps its bits); n is not a multiple of the vector width, and one pass runs on unaligned pointers."""
    correct = [4, 3, 3, 5, 2] if not targeted else [2, 3, 3, 1, 4]
    want_take = [True, True, True, False, True]
    n = 4 * 300 + 3
    rs = np.random.RandomState(11)
    best_dev = T(R.best_init(targeted))
    best_ref = R.best_init(targeted)
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    for off in (0, 1):                                              # off = 1: 4-byte aligned only -> the scalar path
        keep = torch.full((n + 1,), -1., device=dev())
        dst = keep[off:off + n]
        for e, k in enumerate(correct):
            row = np.zeros(R.ROW, np.float32)
            row = R.add_to_row(row, stats=(1.5 * (e + 1), 7.25 * (e + 2), 6, k, 6), sqerr=(1000.5 * (e + 1), 6 * 40))
            rec_dev = _row()
            _ops().attack_epoch_close(T(row), best_dev, e, targeted, rec_dev, flag)
            rec, best_ref, take = R.epoch_close(row, best_ref, e, targeted)
            assert take == want_take[e] and int(N(flag)[0]) == int(take), (e, take)
            assert N(rec_dev).tobytes() == rec.tobytes() and N(best_dev).tobytes() == best_ref.tobytes(), (e, N(rec_dev), rec)
            src = T(rs.normal(size=n).astype(np.float32))
            before = N(dst).copy()
            _ops().copy_if(flag, src, dst)
            assert np.array_equal(N(dst), N(src) if take else before), e
        assert N(keep)[n if off == 0 else 0] == -1.                 # nothing written outside [off, off + n)
        best_dev, best_ref = T(R.best_init(targeted)), R.best_init(targeted)
    empty = _row()
    _ops().attack_epoch_close(_row(), best_dev, 0, targeted, empty, flag)       # an epoch without views: NaN, never taken
    assert int(N(flag)[0]) == 0 and np.isnan(N(empty)[3])


def test_attack_stats_ops_pass_opcheck():
    from nerfail_amd import ops as O
    assert set(O.ATTACK_STATS_OPS) == {'attack_logit_stats', 'img_sqerr', 'img_sqerr_grad_add', 'attack_epoch_close', 'copy_if', 'export_u8'}
    rs = np.random.RandomState(0)
    cla, ori_cla = T(rs.normal(size=(3, 8)).astype(np.float32)), T(rs.normal(size=(3, 8)).astype(np.float32))
    x, ori = T(rs.uniform(0, 255, size=(2, 9, 4)).astype(np.float32)), T(rs.randint(0, 256, size=(2, 9, 4)).astype(np.uint8))
    flag = torch.ones(1, dtype=torch.int32, device=dev())
    samples = {'attack_logit_stats': (cla, ori_cla, 2, _row()), 'img_sqerr': (x, ori, _row()),
               'img_sqerr_grad_add': (x, ori, 0.5, torch.zeros_like(x)),
               'attack_epoch_close': (T(R.add_to_row(np.zeros(R.ROW, np.float32), (1., 2., 3, 2, 4), (5., 16))), T(R.best_init(False)), 1, False,
                                      _row(), torch.zeros(1, dtype=torch.int32, device=dev())),
               'copy_if': (flag, torch.arange(7., device=dev()), torch.zeros(7, device=dev())), 'export_u8': (x,)}
    for name in O.ATTACK_STATS_OPS:
        torch.library.opcheck(getattr(torch.ops.nerfail_mi, name).default, samples[name],
                              test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_dynamic'))
