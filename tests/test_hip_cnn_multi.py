"""-m gpu: the multi-right-hand-side backward of the native MyCNN victim (nerfail_cnn_bwd_data_multi, the op
torch.ops.nerfail_mi.cnn_bwd_data_multi, MyCNN.input_gradients, gauss_net.logit_gradients' batched classifier path).

The contract is bitwise: slice r is what the single backward (nerfail_cnn_bwd_data) returns for d_logits[r], so every
comparison here is torch.equal and the accuracy evidence of tests/test_hip_cnn_stages.py carries over."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import cnn_inputs as CI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZES = [(800, 800), (766, 893), (893, 766)]


def _dev():
    return torch.device('cuda:0')


def native(seed=23, num_classes=24):
    from nerfail_amd.MyModel import MyCNN
    m = MyCNN(num_classes)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CI.state_dict(seed, num_classes).items()}, strict=True)
    return m.to(_dev()).requires_grad_(False).eval()


@functools.lru_cache(maxsize=None)
def _image(seed, H, W):
    return CI.cold_tail_image(seed, H, W)[0]


def images(n, seed0=0, H=800, W=800):
    """n images with different objects (different pool routing per image)."""
    return torch.from_numpy(np.stack([_image(seed0 + i, H, W) for i in range(n)])).to(_dev())


def rows(R, B, C=24, seed=0):
    """Dense random d_logits [R,B,C], every row different."""
    return torch.from_numpy(np.random.RandomState(1000 + seed).normal(size=(R, B, C)).astype(np.float32)).to(_dev())


def forward(m, x):
    import nerfail_amd.ops as O
    _, ws, masks = O.cnn_fwd(m.packed(), x, m.num_classes, True)
    return ws, masks


def multi_vs_single(m, x, d):
    """Runs the multi backward and the R single backwards; asserts slice r == single(d[r]) bit for bit. Returns the multi."""
    import nerfail_amd.ops as O
    H, W = x.shape[2], x.shape[3]
    ws, masks = forward(m, x)
    out = O.cnn_bwd_data_multi(m.packed(), ws, masks, d, H, W)
    assert out.shape == (d.shape[0], x.shape[0], 3, H, W)
    for r in range(d.shape[0]):
        ref = O.cnn_bwd_data(m.packed(), ws, masks, d[r].contiguous(), H, W)
        assert torch.equal(out[r], ref), 'slice %d differs from the single backward' % r
    return out


# ---------------------------------------------------------------------------------------------------------- 1. bitwise
@pytest.mark.parametrize('HW', SIZES)
@pytest.mark.parametrize('RB', [(1, 1), (8, 1), (3, 2), (9, 1), (2, 8)])
def test_bitwise_against_single_backward(RB, HW):
    R, B = RB
    m = native(31)
    x = images(B, seed0=10, H=HW[0], W=HW[1])
    out = multi_vs_single(m, x, rows(R, B, seed=R * 16 + B))
    if R > 1 and B > 1:
        # different routing per image and different rows per right-hand side: a swapped b / r index cannot pass the above,
        # and the slices it would confuse are in fact different
        for r in range(R):
            for b in range(B):
                for r2 in range(r + 1, R):
                    assert not torch.equal(out[r, b], out[r2, b]), (r, r2, b)
                for b2 in range(b + 1, B):
                    assert not torch.equal(out[r, b], out[r, b2]), (r, b, b2)


# ---------------------------------------------------------------------------------------------------------- 2. isolation
def test_rows_are_isolated_and_inputs_untouched():
    import nerfail_amd.ops as O
    m = native(32)
    x = images(1, seed0=20)
    ws, masks = forward(m, x)
    d = rows(3, 1, seed=2)
    d[1] = float('nan')
    d[2] = 0.0
    keep = (ws.clone(), masks.clone(), d.clone())
    out = O.cnn_bwd_data_multi(m.packed(), ws, masks, d, 800, 800)
    again = O.cnn_bwd_data_multi(m.packed(), ws, masks, d, 800, 800)
    assert torch.isnan(out[1]).any()                                    # the NaN row reaches its own slice ...
    assert not torch.isnan(out[0]).any() and not torch.isnan(out[2]).any()     # ... and no other
    assert torch.equal(out[0], O.cnn_bwd_data(m.packed(), ws, masks, d[0].contiguous(), 800, 800))
    assert (out[2] == 0).all()                                          # an all-zero row: an exactly zero slice
    assert torch.equal(ws, keep[0]) and torch.equal(masks, keep[1])
    assert torch.equal(torch.nan_to_num(d, nan=7.0), torch.nan_to_num(keep[2], nan=7.0))
    assert torch.equal(torch.isnan(d), torch.isnan(keep[2]))
    assert torch.equal(torch.nan_to_num(out, nan=7.0), torch.nan_to_num(again, nan=7.0))
    assert torch.equal(torch.isnan(out), torch.isnan(again))


# ---------------------------------------------------------------------------------------------------------- 3. one-hot rows
def test_input_gradients_one_hot_rows_match_autograd():
    m = native(33)
    x = images(1, seed0=30).requires_grad_(True)
    logits = m(x)
    d = torch.zeros((8, 1, 24), device=_dev())
    d[torch.arange(8), 0, torch.arange(8)] = 1.0
    G = m.input_gradients(logits, d)
    assert G.shape == (8, 1, 3, 800, 800)
    for k in range(8):
        ref = torch.autograd.grad(logits[0, k], x, retain_graph=True)[0]
        assert torch.equal(G[k], ref), k
    assert torch.equal(G, m.input_gradients(logits, d))                 # the forward's buffers were not consumed


# ---------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals():
    import nerfail_amd.ops as O
    from nerfail_amd import _lib
    lib = _lib.load()
    m = native(34)
    x = images(1, seed0=40)
    ws, masks = forward(m, x)
    # the C entry points: R = 0, R * B beyond the grid's z dimension
    assert lib.nerfail_cnn_bwd_multi_scratch_bytes(0, 1, 800, 800) == 0
    assert lib.nerfail_cnn_bwd_multi_scratch_bytes(65536, 1, 800, 800) == 0
    assert lib.nerfail_cnn_bwd_multi_scratch_bytes(256, 256, 800, 800) == 0
    assert lib.nerfail_cnn_bwd_multi_scratch_bytes(8, 1, 800, 800) == 8 * lib.nerfail_cnn_bwd_scratch_bytes(1, 800, 800)
    d = rows(1, 1)
    dx = torch.empty((1, 1, 3, 800, 800), device=_dev())
    scratch = torch.empty((lib.nerfail_cnn_bwd_multi_scratch_bytes(1, 1, 800, 800) // 4,), device=_dev())
    for R, B in ((0, 1), (65536, 1), (256, 256)):
        rc = lib.nerfail_cnn_bwd_data_multi(_lib.dev(m.packed()), 24, _lib.dev(ws), _lib.dev(masks), _lib.dev(d), R, B, 800, 800,
                                            _lib.dev(scratch), _lib.dev(dx), _lib.stream())
        assert rc != 0 and b'R * B' in lib.nerfail_last_error(), (R, B)
    # the op
    with pytest.raises(ValueError):
        O.cnn_bwd_data_multi(m.packed(), ws, masks, torch.empty((0, 1, 24), device=_dev()), 800, 800)
    with pytest.raises(ValueError):
        O.cnn_bwd_data_multi(m.packed(), ws, masks, rows(1, 1)[0], 800, 800)            # [B,C]: not [R,B,C]
    with pytest.raises(ValueError):
        O.cnn_bwd_data_multi(m.packed(), ws, masks, rows(2, 2), 800, 800)               # B = 2 rows for a forward of 1 image
    with pytest.raises(ValueError):
        O.cnn_bwd_data_multi(m.packed(), ws, masks, rows(2, 1), 700, 800)               # unsupported size
    with pytest.raises(RuntimeError, match='no masks'):
        O.cnn_bwd_data_multi(m.packed(), ws, masks[:0], rows(2, 1), 800, 800)
    # MyCNN.input_gradients
    xg = x.clone().requires_grad_(True)
    logits = m(xg)
    with pytest.raises(ValueError):
        m.input_gradients(logits, rows(2, 1)[0])
    with pytest.raises(ValueError):
        m.input_gradients(logits, rows(2, 2))
    with pytest.raises(ValueError):
        m.input_gradients(logits, rows(2, 1, C=8))
    with pytest.raises(ValueError):
        m.input_gradients(logits, torch.empty((0, 1, 24), device=_dev()))
    with torch.no_grad():
        plain = m(xg)
    with pytest.raises(RuntimeError, match='mask-keeping forward'):
        m.input_gradients(plain, rows(2, 1))
    with pytest.raises(RuntimeError, match='mask-keeping forward'):
        m.input_gradients(logits * 1.0, rows(2, 1))                     # not the forward's own tensor
    with pytest.raises(RuntimeError, match='this module'):
        native(35).input_gradients(logits, rows(2, 1))
    m.input_gradients(logits, rows(2, 1))                               # (fine until a parameter is written)
    with torch.no_grad():
        m.fc1.bias.add_(0.0)
    with pytest.raises(RuntimeError, match='written or moved'):
        m.input_gradients(logits, rows(2, 1))
    logits = m(xg)                                                      # a new forward repacks: the old logits stay refused
    m.input_gradients(logits, rows(2, 1))


# ---------------------------------------------------------------------------------------------------------- 5. opcheck
def test_opcheck_cnn_bwd_data_multi():
    import nerfail_amd.ops  # noqa: F401
    m = native(36)
    x = images(1, seed0=50, H=766, W=766)
    ws, masks = forward(m, x)
    res = torch.library.opcheck(torch.ops.nerfail_mi.cnn_bwd_data_multi.default, (m.packed(), ws, masks, rows(2, 1), 766, 766),
                                test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_static'))
    assert all(v == 'SUCCESS' for v in res.values()), res


# ---------------------------------------------------------------------------------------------------------- 6. attack integration
def _stock(m):
    chans = CI.CHANS
    layers = []
    for i in range(7):
        layers += [torch.nn.Conv2d(chans[i], chans[i + 1], 3), torch.nn.ReLU(), torch.nn.MaxPool2d(2)]
    s = torch.nn.Sequential(*layers, torch.nn.Flatten(), torch.nn.Linear(1024, 512), torch.nn.ReLU(), torch.nn.Linear(512, m.num_classes))
    with torch.no_grad():
        for p, v in zip(s.parameters(), list(m.state_dict().values())):
            p.copy_(v)
    return s.to(_dev()).requires_grad_(False).eval()


def test_logit_gradients_and_deepfool_batched_equal_per_class(monkeypatch):
    import bench_sections as BS
    import nerfail_amd.ops as O
    from nerfail_amd.GaussNet import gauss_net
    from nerfail_amd.deepfool import deepfool
    BS._heavy_imports()
    dev = _dev()
    m = native(19, num_classes=8)
    wi, ori, s_init = BS._attack_inputs(dev, 2, seed=0)
    calls = []
    real = O.cnn_bwd_data_multi

    def counted(*a):
        calls.append(tuple(a[3].shape))
        return real(*a)
    monkeypatch.setattr(O, 'cnn_bwd_data_multi', counted)

    def nets(victim):
        out = []
        for mode in (None, False):
            net = gauss_net(dev, 0.02, victim, 'my_model', epsilon=None)
            assert net.batched_classifier_backward is None              # automatic is the default
            net.batched_classifier_backward = mode
            net.cache_ori_cla = True
            out.append(net)
        return out

    # logit_gradients: the batched path against the forced per-class loop, on deepfool's own call shape (cla + bump)
    classes = [5, 0, 1, 2, 3, 4, 6, 7]
    G = []
    for net in nets(m):
        st = s_init.clone().requires_grad_(True)
        x, x_rgba, cla, _, _ = net(st, wi[:1], ori[:1])
        bump = torch.zeros_like(cla)
        bump[0, 3] = 1e6
        n0 = len(calls)
        G.append(net.logit_gradients(st, None, x, x_rgba, cla + bump, classes))
        G.append(net.logit_gradients(st, None, x, x_rgba, cla, classes[:3]))
        assert len(calls) - n0 == (2 if net.batched_classifier_backward is None else 0)
    assert calls == [(8, 1, 8), (3, 1, 8)]                              # ONE classifier backward per logit_gradients call
    assert torch.equal(G[0], G[2]) and torch.equal(G[1], G[3])
    assert G[0].abs().max() > 0 and not torch.equal(G[0][0], G[0][1])

    # deepfool end to end, both ways
    res = [deepfool((s_init, wi[:1], ori[:1]), 1.0, net, num_classes=8, max_iter=3, m1=1e6, m2=30) for net in nets(m)]
    (rot_a, it_a, oi_a, ci_a, s_a), (rot_b, it_b, oi_b, ci_b, s_b) = res
    assert it_a == it_b and it_a >= 1 and int(oi_a) == int(oi_b) and int(ci_a) == int(ci_b)
    assert torch.equal(rot_a, rot_b) and torch.equal(s_a, s_b)
    assert len(calls) > 2                                               # deepfool took the batched path

    # a stock nn.Sequential victim never takes it
    n0 = len(calls)
    net = nets(_stock(m))[0]
    r = deepfool((s_init, wi[:1], ori[:1]), 1.0, net, num_classes=8, max_iter=2, m1=1e6, m2=30)
    assert r[1] >= 1 and len(calls) == n0


# ---------------------------------------------------------------------------------------------------------- 7. guard pages
def test_under_guard_pages(rank_launcher):
    """Every buffer ends at an unmapped page: an index that uses r * B + b where b belongs is a fault in the child's log."""
    rep = rank_launcher(os.path.abspath(__file__), 1, [], timeout=400, env={'NERFAIL_GUARD_ALLOC': '1'})
    log = '\n'.join(rep['logs'])
    assert rep['rc'] == [0], log
    assert 'Memory access fault' not in log and '[guard_alloc] active' in log and 'CNN MULTI GUARD OK' in log, log


def _guard_child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import guard
    assert guard.install_if_wanted()
    m = native(21)
    multi_vs_single(m, images(2, seed0=5, H=799, W=801), rows(3, 2, seed=9))
    torch.cuda.synchronize()
    print('CNN MULTI GUARD OK', flush=True)


if __name__ == '__main__':
    _guard_child()
