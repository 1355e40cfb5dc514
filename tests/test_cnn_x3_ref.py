"""CPU: the numpy restatement of the bf16x3 split and weight image (tests/cnn_x3_ref.py) has the properties the header states,
and the cases of the x3 GPU tests reach a partial tile of the kernel's geometry in every direction."""
import numpy as np

import cnn_inputs as CI
import cnn_ref as R
import cnn_x3_ref as X


def _random_f32(n, seed, emin=-90, emax=100):
    """f32 values with random signs, full 24-bit significands and exponents in [emin, emax]: every piece stays normal."""
    rs = np.random.RandomState(seed)
    m = rs.randint(1 << 23, 1 << 24, size=n).astype(np.float64)
    e = rs.randint(emin, emax + 1, size=n)
    x = (np.where(rs.randint(0, 2, size=n) == 1, -1.0, 1.0) * np.ldexp(m, e - 23)).astype(np.float32)
    return x


def test_rne_on_the_upper_16_bits():
    f = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, -(1.0 + 2.0 ** -8), 0.0, -0.0,
                  3.0e38], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, -0.0, 3.0e38], np.float32)
    want[-1] = np.float32(2.0 ** 127 * (1 + 98 / 128.0))                       # 3.0e38 = 2^127 x 1.7632: nearest 8-bit significand
    got = X.bf16_rne(f)
    assert np.array_equal(got.view(np.uint32) & 0xffff, np.zeros(f.size, np.uint32))
    assert np.array_equal(got[:7].view(np.uint32), want[:7].view(np.uint32))   # ties go to the even 8-bit significand
    assert abs(float(got[-1]) - 3.0e38) <= 2.0 ** 127 * 2.0 ** -8
    assert np.isinf(X.bf16_rne(np.array([3.4e38], np.float32))[0])             # rounds up to a bf16 Inf


def test_three_pieces_sum_exactly():
    x = np.concatenate([_random_f32(200000, 1), np.array([1.0, -1.0, 0.0, 2.0 ** -100, 255.0, 1.0 / 3.0], np.float32)])
    p = X.split3(x)
    assert np.array_equal(p.view(np.uint32) & 0xffff, np.zeros(p.shape, np.uint32))          # every piece is a bf16
    nz = p[:, x != 0]
    assert (np.abs(nz[nz != 0]) >= R.TINY).all()                                             # (and normal: the premise)
    assert np.array_equal(p.astype(np.float64).sum(0), x.astype(np.float64))                 # x0 + x1 + x2 == x, exactly
    ax = np.abs(x.astype(np.float64))
    assert (np.abs(x - p[0].astype(np.float64)) <= 2.0 ** -8 * ax).all()
    assert (np.abs(p[1].astype(np.float64)) <= 2.0 ** -8 * ax).all()
    assert (np.abs(p[2].astype(np.float64)) <= 2.0 ** -16 * ax).all()


def test_six_products_drop_at_most_2_pow_minus_23():
    a, b = _random_f32(100000, 2, -20, 20), _random_f32(100000, 3, -20, 20)
    pa, pb = X.split3(a).astype(np.float64), X.split3(b).astype(np.float64)
    kept = sum(pa[i] * pb[j] for i, j in ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0)))
    exact = a.astype(np.float64) * b.astype(np.float64)
    rel = np.abs(kept - exact) / np.abs(exact)
    print('dropped terms: worst %.3g, mean %.3g of |a||b| (2^-23 = %.3g)' % (rel.max(), rel.mean(), 2.0 ** -23))
    assert rel.max() <= 2.0 ** -23 and rel.mean() <= 2.0 ** -25


def test_nan_and_inf():
    p = X.split3(np.array([np.nan, np.inf, -np.inf, 3.4e38, 1.5], np.float32))
    assert np.isnan(p[:, 0]).all()                                             # NaN is NaN in all three pieces
    assert np.isinf(p[0, 1:4]).all() and np.isnan(p[1:, 1:3]).all()            # Inf - Inf in the split: NaN pieces follow
    assert p[1, 3] == -np.inf and np.isnan(p[2, 3])                            # a finite value that rounds to Inf: one piece later
    assert np.array_equal(p[:, 4], np.array([1.5, 0.0, 0.0], np.float32))


def test_image_layout():
    C = 8
    sd = CI.state_dict(3, C)
    img = X.x3_image(sd, C)
    assert img.dtype == np.uint8 and img.size == X.x3_bytes() == 16146432
    h = img.view(np.uint16)
    # stage 2 (s = 1) forward, the first region: [KC/16 = 2][NC = 64][9][3][16] of conv2.weight [64][32][3][3]
    w = sd['conv2.weight']
    first = h[:2 * 64 * 9 * 3 * 16].reshape(2, 64, 9, 3, 16)
    for cb, n, t, c in ((0, 0, 0, 0), (1, 63, 8, 15), (1, 5, 4, 7)):
        pieces = X.bf16_bits(X.split3(w[n, 16 * cb + c, t // 3, t % 3].reshape(1)))[:, 0]
        assert np.array_equal(first[cb, n, t, :, c], pieces), (cb, n, t, c)
    # its backward image follows: rows are input channels, K-channels are output channels, taps not flipped
    second = h[first.size:2 * first.size].reshape(4, 32, 9, 3, 16)
    for cb, n, t, c in ((0, 0, 0, 0), (3, 31, 8, 15), (2, 7, 5, 3)):
        pieces = X.bf16_bits(X.split3(w[16 * cb + c, n, t // 3, t % 3].reshape(1)))[:, 0]
        assert np.array_equal(second[cb, n, t, :, c], pieces), (cb, n, t, c)
    # the three planes of every element add up to the weight
    planes = (first.astype(np.uint32) << 16).view(np.float32).astype(np.float64).sum(3)     # [2][64][9][16]
    assert np.array_equal(np.transpose(planes, (1, 0, 3, 2)).reshape(64, 32, 3, 3), w.astype(np.float64))


def test_cases_reach_partial_tiles():
    """conv_x3_kernel keeps the exact kernel's tiles (forward 8 x 8 pooled cells, backward 8 rows x 32 columns of stage input),
    so cnn_ref.SIZES' coverage (tests/test_cnn_ref.py) applies; the three x3 cases come from SIZES and between them reach, at
    stages 2..7, full and partial tiles in both directions, a mask byte with padding cells and both floor-pool parities."""
    assert all(c[:3] in R.SIZES for c in X.CASES)
    dims = [st for c in X.CASES for st in R.stage_dims(c[0], c[1])[1:]]
    assert any(hp % 8 for _, _, hp, _ in dims) and any(wp % 8 for _, _, _, wp in dims)
    assert any(hp % 8 == 0 for _, _, hp, _ in dims) and any(wp % 8 == 0 for _, _, _, wp in dims)
    assert any(hin % 8 for hin, _, _, _ in dims) and any(win % 32 for _, win, _, _ in dims)
    assert any(wp % 8 in (1, 2) for _, _, _, wp in dims)
    for ax in (0, 1):
        assert {(st[ax] - 2) % 2 for st in dims} == {0, 1}
    assert {c[2] for c in X.CASES} == {1, 3} and {k for c in X.CASES for k in c[3]} == {'c', 'n'}
