"""-m gpu: nerfail_export_train_views against the file path, bit for bit. The uint8 store must hold what nerfail_export_u8 writes
(= np.rint(np.clip(x, 0, 255)), cv2.imwrite's conversion) and the float32 store what the reference makes of those bytes: fixture
g30 (the reference's load_blender_data(train_dir=...) RUN on the 256 x 256 image of every (colour, alpha) pair and on 3-channel
PNGs) composited by training_images, and tests/poison_ref.py - that same chain in numpy, pinned to g30 by
tests/test_retrain_paths.py - for every other input."""
import ctypes
import os

import numpy as np
import pytest
import torch

import poison_ref as PR
from hiputil import T, N, dev

pytestmark = pytest.mark.gpu

SENT_U8, SENT_F = 0xA5, -7.25


def _ops():
    from nerfail_amd import ops
    return ops


def _stores(n, H, W, C):
    return (torch.full((n, H, W, C), SENT_U8, dtype=torch.uint8, device=dev()),
            torch.full((n, H, W, 3), SENT_F, dtype=torch.float32, device=dev()))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(x, slots, n_slots):
    """Exports x [B,H,W,C] into `slots` of sentinel-filled stores; every named slot must hold the file path's bits, every other
    slot its sentinel, and adv_u8 must be ops.export_u8 of the view."""
    B, H, W, C = x.shape
    adv, tgt = _stores(n_slots, H, W, C)
    xd = T(x)
    _ops().export_train_views(xd, list(slots), adv, tgt)
    want_u8, want_t = PR.targets_of_export(x)
    got_u8, got_t = N(adv), N(tgt)
    assert np.array_equal(N(_ops().export_u8(xd)), want_u8)
    for b, s in enumerate(slots):
        assert np.array_equal(got_u8[s], want_u8[b]), (b, s)
        assert np.array_equal(_bits(got_t[s]), _bits(want_t[b])), (b, s, np.abs(got_t[s] - want_t[b]).max())
    for s in set(range(n_slots)) - set(slots):
        assert (got_u8[s] == SENT_U8).all() and (got_t[s] == SENT_F).all(), s


def _edge_values():
    """k +- 0.5 and one ulp either side of them, -0.0, negatives, values above 255, 1e9."""
    k = np.arange(0, 256, dtype=np.float32)
    half = np.concatenate([k - np.float32(.5), k + np.float32(.5)])
    vals = [half, np.nextafter(half, np.float32(-1e9)), np.nextafter(half, np.float32(1e9)), k,
            np.array([-0.0, 0.0, -1e-30, -1.0, -300.5, 255.0, 255.49, 255.5, 255.51, 256.0, 300.0, 1e9, -1e9], np.float32)]
    return np.concatenate(vals).astype(np.float32)


def _random_export(rs, B, H, W, C):
    x = rs.uniform(-20., 280., size=(B, H, W, C)).astype(np.float32)
    edge = _edge_values()
    flat = x.reshape(-1)
    take = min(flat.size // 2, edge.size)
    flat[rs.choice(flat.size, take, replace=False)] = rs.choice(edge, take, replace=False)
    if C == 4:                                                             # opaque, transparent and partly transparent pixels
        a = x[..., 3]
        m = rs.uniform(size=a.shape)
        a[m < .35], a[m > .7] = 255., 0.
    return x


def test_every_colour_alpha_pair_matches_the_reference_fixture():
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g30_train_dir.npz'))
    raw = g['full_raw_adv']                                                # RGBA, the PNG's order
    x = np.ascontiguousarray(raw[..., [2, 1, 0, 3]]).astype(np.float32)    # the export holds BGRA
    adv, tgt = _stores(1, 256, 256, 4)
    _ops().export_train_views(T(x), [0], adv, tgt)
    assert np.array_equal(N(adv)[..., [2, 1, 0, 3]], raw)
    t = g['full_train_imgs']                                               # what the reference's loader returned ...
    want = (t[..., :3] * t[..., 3:]).astype(np.float32) + (np.float32(1.) - t[..., 3:])      # ... through RN:588, float32
    got = N(tgt)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4])


def test_three_channel_views_match_the_reference_fixture():
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g30_train_dir.npz'))
    raw = g['rgb_raw_adv']                                                 # [3,12,12,3] RGB
    x = np.ascontiguousarray(raw[..., ::-1]).astype(np.float32)            # BGR, as x_rgb
    adv, tgt = _stores(3, 12, 12, 3)
    _ops().export_train_views(T(x), [2, 0, 1], adv, tgt)
    for b, s in enumerate([2, 0, 1]):
        assert np.array_equal(N(adv)[s][..., ::-1], raw[b])
        assert np.array_equal(_bits(N(tgt)[s]), _bits(g['rgb_train_imgs'][b]))


@pytest.mark.parametrize('C', [4, 3])
@pytest.mark.parametrize('H, W', [(1, 1), (1, 3), (3, 5), (5, 7), (16, 16), (17, 67)])
def test_shapes_slots_and_sentinels(H, W, C):
    """P below 4, P odd with slot > 0 (the slot's base is then only 4-byte aligned: the pixel-by-pixel path), P a multiple of 4
    (the wide path) and 17 x 67 (more than one quad per lane's stride, a scalar tail); B = 1 and B = 3 into a 5-slot store."""
    rs = np.random.RandomState(1000 * H + 10 * W + C)
    _check(_random_export(rs, 3, H, W, C), [4, 0, 2], 5)
    _check(_random_export(rs, 1, H, W, C), [3], 5)
    _check(_random_export(rs, 1, H, W, C), [0], 1)


@pytest.mark.parametrize('C', [4, 3])
def test_more_views_than_one_launch_carries(C):
    """20 views: the entry point loops over launches of 16; the second launch starts at view 16 of x."""
    rs = np.random.RandomState(77 + C)
    slots = list(rs.permutation(23)[:20])
    _check(_random_export(rs, 20, 3, 5, C), [int(s) for s in slots], 23)
    _check(_random_export(rs, 20, 4, 4, C), [int(s) for s in slots], 23)


@pytest.mark.parametrize('C', [4, 3])
def test_rounding_edges(C):
    """Every k +- 0.5 (round half to even), one ulp either side, -0.0, negative, above 255 and 1e9 - in every channel, alpha
    included, so that the composite sees the rounded alpha."""
    e = _edge_values()
    n = e.size
    rs = np.random.RandomState(5)
    x = np.stack([e[rs.permutation(n)] if c else e for c in range(C)], -1).reshape(1, 1, n, C)
    assert n % 2 == 1 and (n - 1) % 4 == 0
    _check(np.ascontiguousarray(x), [1], 2)                                # P odd, slot 1: pixel by pixel
    _check(np.ascontiguousarray(x[:, :, :n - 1]), [1], 2)                  # all but one of them with P a multiple of 4: the wide path


def test_a_later_export_replaces_an_earlier_one_and_leaves_the_rest():
    rs = np.random.RandomState(9)
    a, b = _random_export(rs, 2, 5, 7, 4), _random_export(rs, 1, 5, 7, 4)
    adv, tgt = _stores(3, 5, 7, 4)
    _ops().export_train_views(T(a), [0, 1], adv, tgt)
    _ops().export_train_views(T(b), [1], adv, tgt)
    (u_a, t_a), (u_b, t_b) = PR.targets_of_export(a), PR.targets_of_export(b)
    assert np.array_equal(N(adv)[0], u_a[0]) and np.array_equal(N(adv)[1], u_b[0]) and (N(adv)[2] == SENT_U8).all()
    assert np.array_equal(_bits(N(tgt)[0]), _bits(t_a[0])) and np.array_equal(_bits(N(tgt)[1]), _bits(t_b[0])) and (N(tgt)[2] == SENT_F).all()


def test_error_returns_leave_the_stores_alone():
    from nerfail_amd import _lib
    lib = _lib.load()
    H, W = 3, 5
    P = H * W
    adv, tgt = _stores(5, H, W, 4)
    big = torch.zeros((3 * P * 4 + 4,), dtype=torch.float32, device=dev())
    x = big[:3 * P * 4]

    def call(src, slots, n_slots=5):
        tab = (ctypes.c_int32 * len(slots))(*slots)
        return lib.nerfail_export_train_views(_lib.c_p(src.data_ptr()), 4, len(slots), P, tab, n_slots, _lib.c_p(adv.data_ptr()),
                                              _lib.c_p(tgt.data_ptr()), _lib.stream())
    assert call(x, [4, 0, 4]) == 1 and b'distinct' in lib.nerfail_last_error()
    assert call(x, [4, 5, 0]) == 1 and b'outside' in lib.nerfail_last_error()
    assert call(x, [4, -1, 0]) == 1 and b'outside' in lib.nerfail_last_error()
    assert call(big[1:], [4, 0, 2]) == 1 and b'aligned' in lib.nerfail_last_error()      # a 4-channel source on a 4-byte boundary
    torch.cuda.synchronize()
    assert (N(adv) == SENT_U8).all() and (N(tgt) == SENT_F).all()
    ops = _ops()
    xv = x.view(3, H, W, 4)
    with pytest.raises(ValueError, match='outside'):
        ops.export_train_views(xv, [0, 1, 5], adv, tgt)
    with pytest.raises(_lib.NerfailError, match='distinct'):
        ops.export_train_views(xv, [1, 1, 2], adv, tgt)
    with pytest.raises(_lib.NerfailError, match='aligned'):
        ops.export_train_views(big[1:1 + 3 * P * 4].view(3, H, W, 4), [0, 1, 2], adv, tgt)
    with pytest.raises(ValueError, match='one slot per view'):
        ops.export_train_views(xv, [0, 1], adv, tgt)
    with pytest.raises(ValueError, match='adv_u8'):
        ops.export_train_views(xv, [0, 1, 2], adv[:, :, :, :3].contiguous(), tgt)
    assert (N(adv) == SENT_U8).all() and (N(tgt) == SENT_F).all()
    assert 'export_train_views' in ops.POISON_OPS and hasattr(torch.ops.nerfail_mi, 'export_train_views')


def test_op_passes_opcheck():
    _ops()
    tests = ('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_static')
    for C in (4, 3):
        adv, tgt = _stores(4, 3, 5, C)
        x = T(_random_export(np.random.RandomState(C), 2, 3, 5, C))
        res = torch.library.opcheck(torch.ops.nerfail_mi.export_train_views.default, (x, [1, 3], adv, tgt), test_utils=tests)
        assert all(v == 'SUCCESS' for v in res.values()), (C, res)
