"""tests/resize_ref.py, the numpy definition of the classifier-input resize, held to torch's own op: the float64 matrix form against
F.interpolate(mode='bilinear', antialias=True) on the CPU in float64, forward and adjoint (through autograd); the fixed-order
float32 restatement against the float64 form within the roundings it makes; an identity shape; the inverted tables."""
import numpy as np
import pytest
import torch

import resize_ref as RR

SHAPES = [((800, 800), (299, 299)), ((800, 800), (224, 224)), ((37, 53), (16, 16)), ((20, 23), (29, 29)), ((16, 16), (16, 16)),
          ((5, 7), (3, 3)), ((299, 300), (299, 299)), ((3, 3), (8, 8))]
IDS = ['%dx%d-%dx%d' % (s + d) for s, d in SHAPES]


def _image(shape, seed, B=1):
    return np.random.RandomState(seed).uniform(0, 255, size=(B, 3) + shape)


@pytest.mark.parametrize('src, dst', SHAPES, ids=IDS)
def test_float64_form_is_torchs_op(src, dst):
    v = _image(src, 1)
    g = np.random.RandomState(2).normal(size=(1, 3) + dst)
    x = torch.from_numpy(v).requires_grad_(True)
    y = torch.nn.functional.interpolate(x, size=dst, mode='bilinear', align_corners=False, antialias=True)
    y.backward(torch.from_numpy(g))
    bound = 1e-12 * 255
    assert np.abs(RR.forward64(v, *dst) - y.detach().numpy()).max() <= bound
    assert np.abs(RR.adjoint64(g, *src) - x.grad.numpy()).max() <= bound * np.abs(g).max()


@pytest.mark.parametrize('src, dst', SHAPES, ids=IDS)
def test_fixed_order_float32_is_the_float64_form_up_to_its_roundings(src, dst):
    """One rounding per weight, per product and per partial sum: (kx + ky + 4) * 2^-24 * max|v|, forward and adjoint (for the
    adjoint v is g). Measured on these inputs: at most 0.52 of the bound (adjoint, 3x3 -> 8x8)."""
    ty, tx = RR.axis_table(src[0], dst[0]), RR.axis_table(src[1], dst[1])
    bound = (tx['kmax'] + ty['kmax'] + 4) * 2.0 ** -24
    v = _image(src, 3, B=2).astype(np.float32)
    got, want = RR.forward32(v, 1, *dst), RR.forward64(v, *dst)
    assert got.dtype == np.float32 and got.shape == (2, 3) + dst
    err = np.abs(got - want).max()
    print('forward  %s -> %s: %.3g of the bound' % (src, dst, err / (bound * np.abs(v).max())))
    assert err <= bound * np.abs(v).max()
    g = np.random.RandomState(4).uniform(-255, 255, size=(2, 2, 3) + dst).astype(np.float32)
    got, want = RR.adjoint32(g, None, 1, *src), RR.adjoint64(g, *src)
    assert got.dtype == np.float32 and got.shape == (2, 2, 3) + src
    err = np.abs(got - want).max()
    print('adjoint  %s -> %s: %.3g of the bound' % (src, dst, err / (bound * np.abs(g).max())))
    assert err <= bound * np.abs(g).max()


def test_an_identity_shape_returns_its_input():
    v = _image((16, 16), 5, B=2).astype(np.float32)
    assert np.array_equal(RR.forward32(v, 1, 16, 16), v)
    g = np.random.RandomState(6).normal(size=(3, 2, 3, 16, 16)).astype(np.float32)
    assert np.array_equal(RR.adjoint32(g, None, 1, 16, 16), g)


@pytest.mark.parametrize('n_in, n_out', sorted(set([(s[i], d[i]) for s, d in SHAPES for i in (0, 1)] + [(800, 64), (3, 40)])))
def test_inverted_ranges_are_contiguous_and_cover_every_input(n_in, n_out):
    t = RR.axis_table(n_in, n_out)                      # (the builder asserts both facts)
    for j in range(n_in):
        readers = [i for i in range(n_out) if t['start'][i] <= j < t['start'][i] + t['count'][i]]
        assert readers == list(range(t['ostart'][j], t['ostart'][j] + t['ocount'][j])) and readers
    assert t['refused'] == ((n_in, n_out) in ((800, 64), (3, 40)))
    assert np.all(t['w'].sum(1) > 0.999) and np.all(t['w'] >= 0)


def test_the_white_background_rule_and_the_adjoint_through_it():
    rs = np.random.RandomState(7)
    x = rs.uniform(0, 255, size=(1, 6, 5, 4)).astype(np.float32)
    x[0, :, :, 3] = np.array([0., -0., 1e-38, -3., np.nan, 1.], np.float32)[:, None]
    v = RR.source_values(x, 0)
    assert v.shape == (1, 3, 6, 5)
    for row, on in enumerate([False, False, True, False, False, True]):
        assert np.array_equal(v[0, :, row], np.moveaxis(x[0, row, :, :3], -1, 0) if on else np.full((3, 5), 255, np.float32))
    t = torch.from_numpy(x).requires_grad_(True)
    c = t.permute(0, 3, 1, 2)
    y = torch.nn.functional.interpolate(torch.where(c[:, 3:4] > 0, c[:, :3], torch.full_like(c[:, :3], 255.)).double(), size=(4, 3),
                                        mode='bilinear', align_corners=False, antialias=True)
    g = rs.normal(size=(1, 3, 4, 3))
    y.backward(torch.from_numpy(g))
    got = RR.adjoint32(g[None].astype(np.float32), x, 0, 6, 5)[0]
    assert np.abs(got - t.grad.numpy()).max() <= 1e-5 and not got[..., 3].any()
    assert not got[0, [0, 1, 3, 4]].any() and not np.signbit(got[0, [0, 1, 3, 4]]).any()
