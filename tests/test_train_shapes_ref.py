"""CPU: the two references that judge the training kernels at architectures other than (8, 256, skip 4), against each
other before either judges a kernel: the float64 torch network under autograd (hiputil.torch_nerf_mlp, the truth of
tests/test_hip_train_shapes.py) and the oracle's closed-form backward (oracle.nerf.mlp_backward on the float32 forward
cache, what oracle.nerf.train_step_grads is made of), on identical inputs."""
import numpy as np
import pytest
import torch

import synth
from conftest import l2_err
from hiputil import mlp_shape_inputs as shape_inputs, torch_mlp_grads as torch_grads
from oracle import nerf as O

# Measured on the inputs below (x86-64, numpy + OpenBLAS, torch CPU): worst per-parameter L2 distance 3.3e-7 at (3, 128, 0),
# 2.9e-7 at (6, 256, 3) - the float32 forward cache (activations rounded to 2^-24 relative, encodings from float32
# sin / cos) against a float64 forward. 2e-6 leaves 6x for another BLAS's summation order. A wrong skip rule, a missed
# `i < D - 1`, or a [:, 63:] cut at the wrong layer is an error of order 1.
REF_BOUND = 2e-6


@pytest.mark.parametrize('D,W,skip,seed', [(3, 128, 0, 330), (6, 256, 3, 366)])     # (seeds: nearest pre-activation 1.5e-5 / 5.5e-6)
def test_oracle_backward_equals_float64_autograd(D, W, skip, seed):
    sd, skips, pts, dirs, d_raw = shape_inputs(D, W, skip, 3, 16, seed)
    raw, cache = O._mlp_forward_cached(sd, pts, dirs, D, W, skips)
    # no ReLU sits on its kink: a float32 pre-activation within 1e-6 of zero could have the other sign in float64, and the
    # two references would then differ by a whole sample's contribution instead of by rounding
    nearest = min(float(np.abs(p).min()) for p in cache['pre'] + [cache['hv_pre']])
    assert nearest > 1e-6, nearest
    got = O.mlp_backward(sd, cache, d_raw, D, W, skips)
    truth = torch_grads(sd, pts, dirs, d_raw, torch.float64, D, W, skips)
    assert set(got) == set(truth) == set(sd)
    worst = 0.0
    for k in sd:
        assert got[k].shape == sd[k].shape
        e = l2_err(got[k], truth[k])
        worst = max(worst, e)
        print('%-26s oracle backward vs float64 autograd %.2e' % (k, e))
    print('(D, W, skip) = (%d, %d, %d): nearest pre-activation to zero %.1e, worst %.2e (bound %.0e)' % (D, W, skip, nearest, worst, REF_BOUND))
    assert worst < REF_BOUND


def test_skip_at_or_past_the_last_layer_is_no_skip():
    """RH:106 as make_layout reads it: a skip index >= D - 1 never fires; both references must build the plain network."""
    sd, _, pts, dirs, d_raw = shape_inputs(4, 64, -1, 2, 8, 77)
    a = torch_grads(sd, pts, dirs, d_raw, torch.float64, 4, 64, (4,))
    b = torch_grads(sd, pts, dirs, d_raw, torch.float64, 4, 64, ())
    c = torch_grads(sd, pts, dirs, d_raw, torch.float64, 4, 64, (3,))
    for k in sd:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k])


def test_train_step_grads_takes_an_architecture_per_network():
    """oracle.nerf.train_step_grads with arch_coarse / arch_fine: the defaults are today's, a shared network sums both passes."""
    R, Ns, Ni = 3, 8, 12
    rs = np.random.RandomState(5)
    rays = synth.ray_batch(R, seed=4)
    target = rs.uniform(size=(R, 3)).astype(np.float32)
    t_rand, u = rs.uniform(size=(R, Ns)).astype(np.float32), rs.uniform(size=(R, Ni)).astype(np.float32)
    sc, sf = synth.nerf_state_dict(D=4, W=64, seed=1), synth.nerf_state_dict(D=4, W=64, seed=2)
    a = O.train_step_grads(rays, sc, sf, target, Ns, Ni, t_rand=t_rand, u=u, D=4, W=64)
    b = O.train_step_grads(rays, sc, sf, target, Ns, Ni, t_rand=t_rand, u=u, arch_coarse=(4, 64, (4,)), arch_fine=(4, 64, ()))
    assert a['loss'] == b['loss']
    for tag in ('grads_coarse', 'grads_fine'):
        for k in a[tag]:
            assert np.array_equal(a[tag][k], b[tag][k])
    # different architectures: the fine network's gradients have the fine network's shapes
    s5 = synth.nerf_state_dict(D=5, W=128, skips=(2,), seed=3)
    s4 = synth.nerf_state_dict(D=4, W=64, skips=(2,), seed=4)
    c = O.train_step_grads(rays, s4, s5, target, Ns, Ni, t_rand=t_rand, u=u, arch_coarse=(4, 64, (2,)), arch_fine=(5, 128, (2,)))
    assert {k: v.shape for k, v in c['grads_fine'].items()} == {k: v.shape for k, v in s5.items()}
    assert {k: v.shape for k, v in c['grads_coarse'].items()} == {k: v.shape for k, v in s4.items()}
    assert c['grads_fine']['pts_linears.3.weight'].shape == (128, 128 + 63)
    # one network for both passes: its gradient is the sum of the two passes' gradients
    s1 = synth.nerf_state_dict(D=4, W=128, skips=(1,), seed=6)
    d = O.train_step_grads(rays, s1, None, target, Ns, Ni, t_rand=t_rand, u=u, arch_coarse=(4, 128, (1,)))
    e = O.train_step_grads(rays, s1, s1, target, Ns, Ni, t_rand=t_rand, u=u, arch_coarse=(4, 128, (1,)), arch_fine=(4, 128, (1,)))
    assert d['grads_fine'] is None and d['loss'] == e['loss']
    for k in s1:
        assert l2_err(d['grads_coarse'][k], e['grads_coarse'][k].astype(np.float64) + e['grads_fine'][k]) < 1e-6
