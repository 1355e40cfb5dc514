"""-m gpu: nerfail_cls_input_resize_fwd / _bwd (nerfail_amd/csrc/resize.hip) against tests/resize_ref.py's fixed-order float32
restatement, compared with == on values (NaNs in the same places): the shapes of the definition, output and source sides of
tile - 1, tile and tile + 1 for every tile the kernels take, both layouts, B in {1, 3}, R in {1, 3, 8}, the workload's shape, the
alpha cases of layout 0, the adjoint identity summed on the host, the autograd function and the two ops, and one run under guard
pages."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import resize_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SHAPES = [((37, 53), (16, 16)), ((20, 23), (29, 29)), ((16, 16), (16, 16)), ((5, 7), (3, 3)), ((3, 3), (8, 8)), ((300, 301), (299, 299)),
          ((53, 37), (16, 29))]
# forward tiles are 16 x 32 outputs (8 x 32 from scale 3.3 on, 2 x 8 at scale 7), adjoint tiles 16 x 64 source pixels (smaller only
# below scale 1/4): output sides around the forward tile at a source size that is a multiple of nothing, and source sides around
# the adjoint tile
TILE_SHAPES = [((41, 83), (15, 31)), ((41, 83), (16, 32)), ((41, 83), (17, 33)), ((113, 131), (33, 65)), ((15, 63), (7, 30)), ((16, 64), (7, 30)),
               ((17, 65), (7, 30)), ((33, 129), (12, 50)), ((119, 113), (17, 16)), ((40, 50), (200, 250))]
_ids = lambda v: '%dx%d' % v if isinstance(v, tuple) else None   # noqa: E731


def _dev():
    return torch.device('cuda:0')


def same(a, b):
    """Equal values, NaNs in the same places (and, stricter than ==, the same sign of zero)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


def _src(layout, B, hw, seed):
    rs = np.random.RandomState(seed)
    if layout == 1:
        return rs.uniform(0, 255, size=(B, 3) + hw).astype(np.float32)
    x = rs.uniform(0, 255, size=(B,) + hw + (4,)).astype(np.float32)
    x[..., 3] = rs.randint(0, 3, size=(B,) + hw) * 127.5                                # about a third transparent
    return x


def _ops():
    import nerfail_amd.ops as O
    return O


def fwd(src, layout, dst):
    out = _ops().cls_input_resize(torch.from_numpy(src).to(_dev()), layout, dst[0], dst[1])
    return out.cpu().numpy()


def bwd(g, src, layout, hw):
    s = None if layout == 1 else torch.from_numpy(src).to(_dev())
    return _ops().cls_input_resize_bwd(torch.from_numpy(g).to(_dev()), s, layout, hw[0], hw[1]).cpu().numpy()


def _check(hw, dst, layout, B, Rs, seed):
    src = _src(layout, B, hw, seed)
    assert same(fwd(src, layout, dst), RR.forward32(src, layout, *dst)), ('forward', hw, dst, layout, B)
    g = np.random.RandomState(seed + 1).normal(scale=3., size=(max(Rs), B, 3) + dst).astype(np.float32)
    want = RR.adjoint32(g, src, layout, *hw)
    for R in Rs:
        assert same(bwd(g[:R], src, layout, hw), want[:R]), ('adjoint', hw, dst, layout, B, R)


@pytest.mark.parametrize('layout', (0, 1))
@pytest.mark.parametrize('hw, dst', SHAPES, ids=_ids)
def test_the_definitions_shapes(hw, dst, layout):
    for B in (1, 3):
        _check(hw, dst, layout, B, (1, 3, 8), seed=hw[0] + B)


@pytest.mark.parametrize('layout', (0, 1))
@pytest.mark.parametrize('hw, dst', TILE_SHAPES, ids=_ids)
def test_around_the_tiles(hw, dst, layout):
    _check(hw, dst, layout, 3, (3,), seed=hw[1])
    if (hw, dst) in (((119, 113), (17, 16)), ((40, 50), (200, 250))):          # the lower rungs of either ladder: also B = 1, R = 1 and 8
        _check(hw, dst, layout, 1, (1, 8), seed=hw[0])


def test_the_tiles_are_the_ones_the_shapes_above_straddle():
    from nerfail_amd import _lib
    f, b = (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 2)()
    got = {}
    for hw, dst in TILE_SHAPES + [((800, 800), (299, 299)), ((800, 800), (224, 224))]:
        assert _lib.load().nerfail_resize_tiles(hw[0], hw[1], dst[0], dst[1], f, b) == 0
        got[(hw, dst)] = (tuple(f), tuple(b))
    assert got[((41, 83), (16, 32))] == ((16, 32), (16, 64)) == got[((16, 64), (7, 30))] == got[((800, 800), (299, 299))]
    assert got[((800, 800), (224, 224))][0] == (8, 32)
    assert got[((119, 113), (17, 16))][0] != (16, 32) and got[((40, 50), (200, 250))][1] != (16, 64)      # a lower rung of either ladder


@pytest.mark.parametrize('size', (299, 224))
def test_the_workloads_shape(size):
    _check((800, 800), (size, size), 0, 2, (1,), seed=size)


def test_layout_0_alpha_cases():
    """alpha 0, -0.0, 1e-38, -3, NaN and 1 on pixels at a window's first and last tap."""
    hw, dst = (37, 53), (16, 16)
    tx, ty = RR.axis_table(53, 16), RR.axis_table(37, 16)
    src = _src(0, 1, hw, seed=3)
    src[..., 3] = 1.
    alphas = np.array([0., -0., 1e-38, -3., np.nan, 1.], np.float32)
    spots = []
    for i, a in enumerate(alphas):
        ox, oy = 2 + 2 * i, 1 + 2 * i
        for x, y in ((tx['start'][ox], ty['start'][oy]), (tx['start'][ox] + tx['count'][ox] - 1, ty['start'][oy] + ty['count'][oy] - 1)):
            src[0, y, x, 3] = a
            spots.append((y, x, bool(a > 0)))
    v = RR.source_values(src, 0)
    for y, x, on in spots:
        assert np.array_equal(v[0, :, y, x], src[0, y, x, :3] if on else np.full(3, 255, np.float32))
    assert same(fwd(src, 0, dst), RR.forward32(src, 0, *dst))
    g = np.random.RandomState(5).normal(size=(3, 1, 3) + dst).astype(np.float32)
    got = bwd(g, src, 0, hw)
    assert same(got, RR.adjoint32(g, src, 0, *hw))
    assert not got[..., 3].any() and not np.signbit(got[..., 3]).any()
    for y, x, on in spots:
        px = got[:, 0, y, x, :3]
        assert (px != 0).all() if on else (not px.any() and not np.signbit(px).any())


@pytest.mark.parametrize('layout', (0, 1))
@pytest.mark.parametrize('hw, dst', [((37, 53), (16, 16)), ((20, 23), (29, 29)), ((300, 301), (299, 299)), ((800, 800), (299, 299))], ids=_ids)
def test_adjoint_identity_on_the_device(hw, dst, layout):
    """sum out * g against sum v * gsrc, both in float64 on the host: a table read with the wrong offset shows here even where a
    restatement shares the mistake. v: the source values (layout 0: where alpha > 0 is false the constant 255 has no gradient,
    those pixels carry 255 * the adjoint without the alpha gate - taken from the layout-1 adjoint of the same g)."""
    src = _src(layout, 1, hw, seed=11)
    g = np.random.RandomState(12).uniform(-1, 1, size=(1, 1, 3) + dst).astype(np.float32)
    out = fwd(src, layout, dst).astype(np.float64)
    lhs, scale = (out * g[0]).sum(), np.abs(out * g[0]).sum()
    v = RR.source_values(src, layout).astype(np.float64)
    gs = bwd(g, src, layout, hw)[0].astype(np.float64)
    if layout == 0:
        full = bwd(g, None, 1, hw)[0].astype(np.float64)                                   # [1,3,H,W]
        on = (src[..., 3] > 0)[:, None]
        assert np.array_equal(np.moveaxis(gs[..., :3], -1, 1), np.where(on, full, 0.))
        gs = full
    rhs = (v * gs).sum()
    kx, ky = RR.axis_table(hw[1], dst[1])['kmax'], RR.axis_table(hw[0], dst[0])['kmax']
    assert abs(lhs - rhs) <= (kx + ky + 4) * 2.0 ** -23 * scale, (lhs, rhs, scale)


def test_the_autograd_function_is_the_two_entry_points_and_opcheck():
    from nerfail_amd import _resize
    dev = _dev()
    for layout, hw, dst in ((0, (37, 53), (16, 16)), (1, (20, 23), (29, 29))):
        src = _src(layout, 2, hw, seed=21)
        x = torch.from_numpy(src).to(dev).requires_grad_(True)
        y = (_resize.classifier_input if layout == 0 else _resize.resize_native)(x, dst[0])
        g = torch.randn_like(y)
        y.backward(g)
        assert same(y.detach().cpu().numpy(), fwd(src, layout, dst))
        assert same(x.grad.cpu().numpy(), bwd(g.cpu().numpy()[None], src, layout, hw)[0])
        x2 = torch.from_numpy(src).to(dev).requires_grad_(True)
        y2 = torch.ops.nerfail_mi.cls_input_resize(x2, layout, dst[0], dst[1])
        y2.backward(g)
        assert torch.equal(y2, y) and same(x2.grad.cpu().numpy(), x.grad.cpu().numpy())
        tests = ('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_dynamic')
        res = torch.library.opcheck(torch.ops.nerfail_mi.cls_input_resize.default, (x2, layout, dst[0], dst[1]), test_utils=tests)
        assert all(v == 'SUCCESS' for v in res.values()), res
        res = torch.library.opcheck(torch.ops.nerfail_mi.cls_input_resize_bwd.default,
                                    (g.detach()[None].contiguous(), x2.detach() if layout == 0 else None, layout, hw[0], hw[1]),
                                    test_utils=('test_schema', 'test_faketensor'))
        assert all(v == 'SUCCESS' for v in res.values()), res
    with pytest.raises(ValueError):
        _resize.resize_native(torch.zeros(1, 3, 8, 8, dtype=torch.float64, device=dev), 4)
    with pytest.raises(ValueError):
        _resize.resize_native(torch.zeros(1, 3, 8, 8), 4)
    with pytest.raises(ValueError):
        _resize.classifier_input(torch.zeros(1, 8, 8, 4, device=dev)[:, :, ::2], 4)
    from nerfail_amd import _lib
    with pytest.raises(_lib.NerfailError):
        _resize.resize_native(torch.zeros(1, 3, 800, 800, device=dev), 64)                  # more than 16 taps: refused, no fall-back here


def test_under_guard_pages(rank_launcher):
    """One forward and one adjoint at (37, 53) -> 16, both layouts, every tensor ending its own mapping with unmapped pages behind it
    (tests/guard): a window that reads one pixel past its tile faults here and not in an attack."""
    rep = rank_launcher(os.path.abspath(__file__), 1, [], timeout=300, env={'NERFAIL_GUARD_ALLOC': '1'})
    log = '\n'.join(rep['logs'])
    assert rep['rc'] == [0], log
    assert 'Memory access fault' not in log and '[guard_alloc] active' in log and 'RESIZE GUARD OK' in log, log


def _guard_child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import guard
    assert guard.install_if_wanted()
    for layout in (0, 1):
        _check((37, 53), (16, 16), layout, 3, (3,), seed=31)
    torch.cuda.synchronize()
    print('RESIZE GUARD OK', flush=True)


if __name__ == '__main__':
    _guard_child()
