"""CPU side of the training-batch front (ABI 13): properties of the index shuffle as tests/batch_ref.py restates it, and the
interface - ABI version, the two entry points in the header and the signature table, and their argument validation through
the loaded library (no GPU: every refusal happens before a launch)."""
import ctypes
import os
import re

import numpy as np
import pytest

import batch_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (1, 2, 3, 5, 16, 17, 100, 1023, 1025, 4097)
KEYS = (0, 0x9E3779B9, (7 << 32) | 123456)          # the last one >= 2^32: the key's high half takes part
_WALK = {}


@pytest.mark.parametrize('m', MS)
def test_shuffle_is_a_bijection(m):
    for key in KEYS:
        p, walk = B.shuffle(key, m, return_walk=True)
        _WALK[(m, key)] = walk
        assert p.dtype == np.int64 and np.array_equal(np.sort(p), np.arange(m)), (m, key)
        # a range of the permutation is that slice of it
        first = m // 3
        assert np.array_equal(B.shuffle(key, m, first, m - first), p[first:])
    if m > 16:
        assert not np.array_equal(B.shuffle(KEYS[0], m), B.shuffle(KEYS[1], m))
        assert not np.array_equal(B.shuffle(KEYS[2], m), B.shuffle(KEYS[2] + (1 << 32), m))    # high half alone


def test_walk_length():
    """The cycle walk is short: the network's domain is < 4 m. (64 leaves room above the 34 seen at m = 4 097.)"""
    worst = 0
    for m in MS:
        for key in KEYS:
            worst = max(worst, B.shuffle(key, m, return_walk=True)[1])
    print('largest number of walk iterations:', worst)
    assert worst <= 64


def _key_sets():
    rs = np.random.RandomState(0)
    hi, lo = rs.randint(0, 2 ** 32, (2, 2000), dtype=np.uint64)
    return {'consecutive': [(7 << 32) | s for s in range(2000)],          # (seed << 32) | global_step, as RayBatcher forms them
            'scattered': [(int(a) << 32) | int(b) for a, b in zip(hi, lo)]}


@pytest.mark.parametrize('which', ['consecutive', 'scattered'])
def test_marginal_uniformity(which):
    """n = 100 of m = 1000 under 2 000 keys. Under uniform sampling without replacement every index is included
    Binomial(2000, 0.1) times (mean 200, variance 180 = 200 * 0.9) and is the first draw Binomial(2000, 0.001) times (mean 2),
    so both statistics are chi-square with 999 degrees of freedom: mean 999, standard deviation sqrt(2 * 999). The bound is
    five standard deviations above the mean."""
    m, n, keys = 1000, 100, _key_sets()[which]
    inc, first = np.zeros(m), np.zeros(m)
    for k in keys:
        s = B.shuffle(k, m, 0, n)
        assert len(np.unique(s)) == n
        inc[s] += 1
        first[s[0]] += 1
    chi_inc = float(((inc - 200.) ** 2 / 200. / 0.9).sum())
    chi_first = float(((first - 2.) ** 2 / 2.).sum())
    print('%s keys: inclusion statistic %.1f, first-position statistic %.1f' % (which, chi_inc, chi_first))
    bound = 999 + 5 * np.sqrt(2 * 999)
    assert chi_inc < bound and chi_first < bound


def test_population_map():
    view, row, col = B.population(np.arange(2 * 2 * 4), 2, 4, row0=1, col0=2, view_ids=[2, 0])
    assert view.tolist() == [2] * 8 + [0] * 8
    assert row.tolist() == [1, 1, 1, 1, 2, 2, 2, 2] * 2
    assert col.tolist() == [2, 3, 4, 5] * 4
    view, row, col = B.population([0, 34, 35, 69], 5, 7, view0=3)
    assert (view.tolist(), row.tolist(), col.tolist()) == ([3, 3, 4, 4], [0, 4, 0, 4], [0, 6, 0, 6])


# ---------------------------------------------------------------------------------------------- interface
def test_abi_13_declares_both_entry_points():
    from nerfail_amd import _lib
    assert _lib.ABI_VERSION >= 13
    header = open(os.path.join(ROOT, 'include', 'nerfail_hip.h')).read()
    assert int(re.search(r'#define NERFAIL_ABI_VERSION (\d+)', header).group(1)) == _lib.ABI_VERSION
    for name in ('nerfail_index_shuffle', 'nerfail_train_batch'):
        assert name in _lib.SIGNATURES
        assert re.search(r'\bint %s\(' % name, header)
    lib = _lib.load()
    assert lib.nerfail_abi_version() == _lib.ABI_VERSION


def test_ops_are_registered():
    import torch
    from nerfail_amd import ops  # noqa: F401
    assert hasattr(torch.ops.nerfail_mi, 'index_shuffle') and hasattr(torch.ops.nerfail_mi, 'train_batch')
    from nerfail_amd import train
    assert callable(train.train) and callable(train.RayBatcher)


def test_argument_validation_without_gpu():
    from nerfail_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)                          # any non-NULL pointer: every case below is refused before a launch

    def shuffle(m, first, n, out=one):
        return lib.nerfail_index_shuffle(5, m, first, n, out, None)
    assert shuffle(0, 0, 0) == 1 and b'm must be' in lib.nerfail_last_error()            # m = 0
    assert shuffle((1 << 31) + 1, 0, 1) == 1
    assert shuffle(10, 4, 7) == 1 and b'range' in lib.nerfail_last_error()               # n > m - first
    assert shuffle(10, -1, 2) == 1 and shuffle(10, 0, -1) == 1 and shuffle(10, 11, 0) == 1
    assert shuffle(10, 0, 10, None) == 1 and b'out is NULL' in lib.nerfail_last_error()  # NULL output
    assert shuffle(10, 10, 0, None) == 0                                                 # an empty range is a no-op

    k4 = _lib.host_floats([10., 10., 3.5, 2.5])

    def batch(H=5, W=7, win=(0, 0, 5, 7), n_img=3, view0=0, n_views=2, first=0, n=4, K=k4, poses=one, images=one, rays=one,
              target=one, view_ids=None):
        return lib.nerfail_train_batch(H, W, K, 2., 6., poses, n_img, images, win[0], win[1], win[2], win[3], view_ids, view0,
                                       n_views, None, 9, first, n, rays, target, None, None)
    for win in ((1, 2, 5, 4), (1, 2, 2, 6), (-1, 0, 2, 2), (0, 8, 1, 0), (0, 0, 6, 7)):  # window outside the image
        assert batch(win=win) == 1 and b'window' in lib.nerfail_last_error(), win
    assert batch(n=71) == 1 and b'outside the population' in lib.nerfail_last_error()    # n > m - first (m = 70)
    assert batch(first=60, n=11) == 1
    assert batch(win=(1, 2, 2, 4), n=17) == 1                                            # the window's population: 16
    assert batch(n_views=0) == 1 and b'population' in lib.nerfail_last_error()           # m = 0
    assert batch(win=(1, 2, 0, 4), n=0) == 1
    assert batch(view0=2) == 1 and b'views' in lib.nerfail_last_error()                  # slots 2, 3 of 3 images
    assert batch(rays=None) == 1 and b'rays is NULL' in lib.nerfail_last_error()         # NULL outputs / inputs
    assert batch(target=None) == 1 and b'target is NULL' in lib.nerfail_last_error()
    assert batch(poses=None) == 1 and batch(K=None) == 1
    assert batch(H=0) == 1
    assert batch(n=0, rays=None, target=None) == 0                                       # an empty batch is a no-op
