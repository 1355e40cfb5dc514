"""CPU only: the weight-gradient reference of tests/cnn_ref_dw.py pinned to ATen, and the CPU-visible side of the MyCNN
training feature (ABI 11): size helpers, op registration, the fake, the opt-in constructor."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_inputs as CI
import cnn_ref as R
import cnn_ref_dw as D


def rel_l2(a, b):
    return float(np.linalg.norm((np.asarray(a, np.float64) - b).reshape(-1)) / np.linalg.norm(np.asarray(b).reshape(-1)))


@pytest.fixture(scope='module')
def pinned():
    """float64 autograd of the network on an odd size with ties, and the forced-routing chain on forward64's routing."""
    H, W = 767, 769
    sd = CI.state_dict(7)
    x = np.stack([CI.cold_tail_image(101, H, W)[0], R.noise_image(5, H, W)])
    logits, acts, codes, hidden = R.forward64(sd, x)
    d_logits = np.random.RandomState(0).normal(size=logits.shape)
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
    h = torch.from_numpy(x).double()
    for i in range(1, 8):
        h = F.max_pool2d(F.relu(F.conv2d(h, p['conv%d.weight' % i], p['conv%d.bias' % i])), 2)
    h = F.relu(F.linear(h.reshape(h.shape[0], -1), p['fc1.weight'], p['fc1.bias']))
    lg = F.linear(h, p['fc2.weight'], p['fc2.bias'])
    assert np.array_equal(lg.detach().numpy(), logits)
    want = torch.autograd.grad((lg * torch.from_numpy(d_logits)).sum(), [p[k] for k in D.names()])
    want = {k: g.numpy() for k, g in zip(D.names(), want)}
    got, pooled, dh, dx = D.chain_dw(sd, x, acts, codes, hidden, d_logits, torch.float64, (H, W))
    return {'sd': sd, 'x': x, 'acts': acts, 'codes': codes, 'hidden': hidden, 'd': d_logits, 'want': want, 'got': got,
            'pooled': pooled, 'dx': dx, 'hw': (H, W)}


def test_chain_dw_equals_autograd_float64(pinned):
    """With the routing forward64 chose the chain IS the network's gradient: every one of the 18 parameters equals
    torch.autograd.grad in float64 (allclose at float64 rounding), and d_x equals cnn_ref.chain_backward."""
    assert list(pinned['got']) != D.names() and sorted(pinned['got']) == sorted(D.names())
    for k in D.names():
        got, want = pinned['got'][k], pinned['want'][k]
        assert got.shape == want.shape and got.dtype == np.float64, k
        e = rel_l2(got, want)
        print('%-13s relative L2 %.2e' % (k, e))
        assert np.allclose(got, want, rtol=1e-9, atol=1e-12 * np.abs(want).max()), (k, e)
        assert e <= 1e-12, (k, e)
    p = pinned
    dx = R.chain_backward(p['sd'], p['acts'], p['codes'], p['hidden'], p['d'], torch.float64, p['hw'])
    assert np.array_equal(dx, p['dx'])
    dims = R.stage_dims(*p['hw'])
    assert [g.shape for g in p['pooled']] == [(2, R.CHANS[s + 1], d[2], d[3]) for s, d in enumerate(dims)]


def test_reference_breaks_on_lost_or_transposed_taps_and_nhwc_columns(pinned):
    w = pinned['want']
    for k in ('conv2.weight', 'conv7.weight'):
        got = pinned['got'][k]
        lost = got.copy()
        lost[:, :, 1, 2] = 0
        assert rel_l2(lost, w[k]) > 1e-2                                     # (agreement is 1e-12: a structural error is ten orders above)
        assert rel_l2(np.transpose(got, (0, 1, 3, 2)), w[k]) > 1e-2         # ky and kx swapped (the three diagonal taps stay)
        assert rel_l2(got[:, :, ::-1, ::-1], w[k]) > 1e-2                  # flipped taps (the backward-data order)
    g1 = pinned['got']['fc1.weight']
    nhwc = g1.reshape(512, 64, 16).transpose(0, 2, 1).reshape(512, 1024)    # columns left in (y * 4 + x) * 64 + c order
    assert rel_l2(nhwc, w['fc1.weight']) > 0.5
    # the same chain in float32 is the stock yardstick: close, not equal
    p = pinned
    g32 = D.chain_dw(p['sd'], p['x'], p['acts'], p['codes'], p['hidden'], p['d'], torch.float32, p['hw'])[0]
    for k in D.names():
        e = rel_l2(g32[k], p['got'][k])
        assert 0 < e < 5e-6, (k, e)


def test_buffer_codecs():
    lay, total = D.grad_layout(37)
    assert [n for n, _, _ in lay] == D.names(37) and all(o % 4 == 0 for _, o, _ in lay)
    assert lay[1][1] == 864 and lay[-1][1] + 40 == total and lay[-2][2] == (37, 512)
    g, defined = D.split_grads(np.arange(total, dtype=np.float64), 37)
    assert g['conv1.bias'][0] == 864 and g['fc2.bias'].shape == (37,) and int((~defined).sum()) == 3
    B, H, W = 3, 769, 772
    n = sum(B * d[2] * d[3] * R.CHANS[s + 1] for s, d in enumerate(R.stage_dims(H, W))) + B * 512
    pooled, dh, used = D.split_scratch(np.arange(n + 100, dtype=np.float64), B, H, W)
    assert used == n and dh.reshape(-1)[-1] == n - 1 and pooled[1].reshape(-1)[0] == pooled[0].size
    assert [p.shape for p in pooled] == [(B, d[2], d[3], R.CHANS[s + 1]) for s, d in enumerate(R.stage_dims(H, W))]


def test_abi_11_size_helpers_and_registration():
    from nerfail_amd import _lib
    import nerfail_amd.ops as O
    assert _lib.ABI_VERSION >= 11 and 'cnn_bwd_weights' in O.CNN_OPS
    lib = _lib.load()
    for C in (1, 24, 37):
        assert lib.nerfail_cnn_grad_floats(C) == D.grad_layout(C)[1] == O.cnn_grad_layout(C)[1]
        assert [(o, tuple(s)) for _, o, s in D.grad_layout(C)[0]] == O.cnn_grad_layout(C)[0]
    for C in (0, -1, 4097):                                     # what makes nerfail_cnn_packed_floats return 0
        assert lib.nerfail_cnn_packed_floats(C) == 0 and lib.nerfail_cnn_grad_floats(C) == 0
    good = lib.nerfail_cnn_bwd_weights_scratch_bytes(3, 769, 772, 24)
    assert good >= 4 * D.split_scratch(np.zeros(0), 0, 769, 772)[2] and good % 16 == 0
    assert good > 4 * sum(3 * d[2] * d[3] * R.CHANS[s + 1] for s, d in enumerate(R.stage_dims(769, 772)))
    for B, H, W, C in ((0, 800, 800, 24), (65536, 800, 800, 24), (1, 765, 800, 24), (1, 800, 894, 24), (1, 800, 800, 0),
                       (1, 800, 800, 4097), (-1, 800, 800, 24)):
        assert lib.nerfail_cnn_workspace_bytes(B, H, W, C) == 0, (B, H, W, C)
        assert lib.nerfail_cnn_bwd_weights_scratch_bytes(B, H, W, C) == 0, (B, H, W, C)


def test_fake_shapes():
    import nerfail_amd.ops as O
    from torch._subclasses.fake_tensor import FakeTensorMode
    from nerfail_amd import _lib
    lib = _lib.load()
    B, H, W, C = 2, 769, 772, 8
    with FakeTensorMode():
        x = torch.empty((B, 3, H, W))
        ws = torch.empty((lib.nerfail_cnn_workspace_bytes(B, H, W, C) // 4,))
        masks = torch.empty((lib.nerfail_cnn_mask_bytes(B, H, W),), dtype=torch.uint8)
        packed = torch.empty((lib.nerfail_cnn_packed_floats(C),))
        for need in (True, False):
            dp, dx = torch.ops.nerfail_mi.cnn_bwd_weights(packed, x, ws, masks, torch.empty((B, C)), need)
            assert tuple(dp.shape) == (lib.nerfail_cnn_grad_floats(C),) and dp.dtype == torch.float32
            assert tuple(dx.shape) == ((B, 3, H, W) if need else (0,))


def test_trainable_is_opt_in():
    from nerfail_amd.MyModel import MyCNN
    sd = {k: torch.from_numpy(v) for k, v in CI.state_dict(3, 8).items()}
    a, b = MyCNN(8), MyCNN(8, trainable=True)
    a.load_state_dict(sd, strict=True)
    b.load_state_dict(sd, strict=True)
    assert list(a.state_dict()) == list(b.state_dict()) == D.names(8)
    assert all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), b.state_dict().values()))
    assert a.trainable is False and b.trainable is True and MyCNN().num_classes == 24
    for m in (a, b):                                            # no CPU path either way
        with pytest.raises(RuntimeError, match='no CPU path'):
            m(torch.zeros((1, 3, 766, 766)))
