"""No GPU: the composition rule of the folded bf16x3 image (feature_linear into views_linears[0]) in numpy against the
two-stage float64 forward, the size helper, and the refusals of the shapes the kernel does not cover."""
import ctypes

import numpy as np
import pytest
import torch

import synth
import x3fold_ref as R
from test_hip_mlp_x3 import _f64_forward


def _cpu_net(D, skips, seed):
    from nerfail_amd.run_nerf_helpers import NeRF
    sd = synth.nerf_state_dict(D=D, W=256, skips=tuple(skips), seed=seed)
    net = NeRF(D=D, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=list(skips), use_viewdirs=True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return sd, net


@pytest.mark.parametrize('D,skips', [(8, [4]), (2, [])])
def test_composition_agrees_with_the_two_stage_float64_forward(D, skips):
    sd, net = _cpu_net(D, skips, seed=308)
    x = np.random.RandomState(D).uniform(-1, 1, size=(257, 90))
    ref = _f64_forward(net, x)
    scale = np.abs(ref).max()
    # the rule itself, before its one rounding: double sums in another order than `feat @ Wv.T` - 1e-12 relative
    wc, bc = R.compose64(sd)
    got, h = R.folded_f64_forward(sd, D, skips, x, wc, bc)
    assert np.abs(got - ref).max() <= 1e-12 * scale, (np.abs(got - ref).max(), scale)
    # rounded once to f32, as the image holds it: |dWc| <= 2^-24 |Wc| and |dbc| <= 2^-24 |bc| elementwise move the views
    # pre-activation by at most 2^-24 (|Wc| |h| + |bc|); the ReLU does not amplify, rgb_linear maps it by |Wrgb|
    wc32, bc32 = R.compose(sd)
    assert wc32.dtype == np.float32 and np.isfinite(wc32).all() and np.isfinite(bc32).all()
    got32, _ = R.folded_f64_forward(sd, D, skips, x, wc32, bc32)
    bound = 2. ** -24 * (np.abs(h) @ np.abs(wc).T + np.abs(bc)) @ np.abs(sd['rgb_linear.weight'].astype(np.float64)).T
    assert (np.abs(got32 - got)[:, :3] <= bound * (1 + 1e-9)).all()
    assert np.array_equal(got32[:, 3], got[:, 3])                  # alpha does not pass through the composed layer
    assert np.abs(got32 - ref).max() < 2e-7 * scale


def test_composition_is_sequential_in_m():
    """The rule fixes the ORDER: summing from the other end gives other bits in some elements, the rule's order does not."""
    sd = synth.nerf_state_dict(D=2, W=256, skips=(), seed=7)
    wc, _ = R.compose64(sd)
    wv = sd['views_linears.0.weight'].astype(np.float64)[:, :256]
    wf = sd['feature_linear.weight'].astype(np.float64)
    again = np.zeros_like(wc)
    back = np.zeros_like(wc)
    for m in range(256):
        again += wv[:, m:m + 1] * wf[m:m + 1, :]
        back += wv[:, 255 - m:256 - m] * wf[255 - m:256 - m, :]
    assert np.array_equal(again, wc)
    assert not np.array_equal(back, wc)


def test_overflowing_product_is_not_finite():
    sd = synth.nerf_state_dict(D=2, W=256, skips=(), seed=7)
    sd = dict(sd)
    sd['feature_linear.weight'] = (sd['feature_linear.weight'] * 1e20).astype(np.float32)
    sd['views_linears.0.weight'] = sd['views_linears.0.weight'].copy()
    sd['views_linears.0.weight'][:, :256] *= np.float32(1e20)
    wc32, _ = R.compose(sd)
    assert not np.isfinite(wc32).all()


def test_bias_index_inverts_the_accumulator_order():
    """Position p of a bias piece holds channel 32 (p // 32) + acc_channel(p % 16, (p // 16) % 2) (mlp_layout.h)."""
    p = np.arange(256)
    ch = 32 * (p >> 5) + ((p & 15) & 3) + 8 * ((p & 15) >> 2) + 4 * ((p >> 4) & 1)
    assert np.array_equal(np.sort(ch), p)
    assert np.array_equal(R.bias_index(ch), p)


def _lib_or_skip():
    from nerfail_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('D,skip', [(8, 4), (8, 3), (8, -1), (6, 2), (4, 1), (2, -1)])
def test_size_helper(D, skip):
    lib = _lib_or_skip()
    folded, unfolded = R.stream_tile_steps(D, skip)
    assert folded % 8 == 0                                           # whole ring groups of 8 tile-steps
    n_x3 = lib.nerfail_mlp_packed_x3_bytes(D, 256, skip)
    assert n_x3 == unfolded * 3 * 1024
    n_f32 = lib.nerfail_mlp_packed_floats(D, 256, skip)
    const_floats = (D + 2) * 256 + 512 + 512                         # bias pieces, alpha head, rgb head (mlp_layout.h)
    composed = lib.nerfail_mlp_x3f_composed_floats(D, 256, skip)
    assert composed == 128 * 256 + 256
    n = lib.nerfail_mlp_packed_x3f_bytes(D, 256, skip)
    assert n == folded * 3 * 1024 + 4 * (const_floats + composed)
    assert n_x3 - folded * 3 * 1024 == 128 * 3 * 1024                # the stream is 128 tile-steps (384 KB) shorter
    assert n_f32 > const_floats
    if (D, skip) == (8, 4):
        assert folded == 1032


@pytest.mark.parametrize('D,W,skip', [(8, 128, 4), (4, 64, 2), (5, 256, 2), (7, 256, -1), (10, 256, 4), (1, 256, -1), (8, 200, 4)])
def test_uncovered_shapes_are_refused(D, W, skip):
    lib = _lib_or_skip()
    assert lib.nerfail_mlp_packed_x3f_bytes(D, W, skip) == 0
    assert lib.nerfail_mlp_x3f_composed_floats(D, W, skip) == 0
    one = ctypes.c_void_p(16)                                        # never dereferenced: the shape is refused first
    assert lib.nerfail_mlp_pack_x3f(one, D, W, skip, one, None) == 1  # NERFAIL_EINVAL
    assert lib.nerfail_mlp_pack_x3f(None, 8, 256, 4, one, None) == 1
    assert lib.nerfail_mlp_pack_x3f(one, 8, 256, 4, None, None) == 1


@pytest.mark.parametrize('D,W,skips', [(8, 128, [4]), (4, 64, [2]), (5, 256, [2])])
def test_no_image_for_uncovered_shapes_without_a_device(D, W, skips):
    """packed_x3f() of a shape without an image is None, asked for once; the f32 image it starts from is stubbed, there is
    no GPU here."""
    from nerfail_amd._images import ImageCache
    from nerfail_amd.run_nerf_helpers import NeRF
    net = NeRF(D=D, W=W, input_ch=63, input_ch_views=27, output_ch=5, skips=list(skips), use_viewdirs=True)
    asked = []

    def pack_x3f(f32):
        asked.append(f32)
        return net._pack_x3f(f32)
    net._images = ImageCache(net.ordered_params, {'f32': (lambda: torch.zeros(1), None), 'x3f': (pack_x3f, 'f32')})
    assert net.packed_x3f() is None
    assert net.packed_x3f() is None and len(asked) == 1                      # cached
