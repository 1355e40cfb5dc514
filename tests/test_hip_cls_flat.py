"""-m gpu: MyCNN with flat parameters (MyCNN.flatten_parameters, MyCNN.sgd_step): the same logits, a reference-order state dict
round trip, pack calls counted at the C ABI with the proxy pattern of tests/test_hip_image_cache.py, and the frozen uses
(input_gradients, DeepFool) unchanged."""
import collections
import io

import numpy as np
import pytest
import torch

import cnn_inputs as CI
import cls_inputs as XI

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda:0')


def module(seed=41, num_classes=8, trainable=True):
    from nerfail_amd.MyModel import MyCNN
    m = MyCNN(num_classes, trainable=trainable)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CI.state_dict(seed, num_classes).items()}, strict=True)
    return m.to(_dev())


def images(n=1, seed=410):
    st, _ = XI.views(seed, XI.VAL_LABELS[:n])
    return torch.from_numpy(XI.white_nchw(st)).to(_dev())


class CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ('nerfail_cnn_pack', 'nerfail_cnn_sgd_step'):
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


@pytest.fixture
def lib(monkeypatch):
    from nerfail_amd import _lib
    proxy = CountingLib(_lib.load())
    monkeypatch.setattr(_lib, '_lib', proxy)
    return proxy


def test_flatten_keeps_logits_and_state_dict():
    from nerfail_amd import ops
    m = module()
    x = images()
    with torch.no_grad():
        before = m(x)
    names = [id(p) for p in m.parameters()]
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    flat = m.flatten_parameters()
    assert m.flatten_parameters() is flat                                        # twice: a no-op
    assert names == [id(p) for p in m.parameters()]                              # the Parameter objects are the same ones
    layout, total = ops.cnn_grad_layout(8)
    assert flat.numel() == total and all(p.data_ptr() == flat.data_ptr() + 4 * o for (o, _), p in zip(layout, m._params()))
    with torch.no_grad():
        after = m(x)
    assert torch.equal(before, after)
    assert list(m.state_dict()) == [k for k, _ in CI.param_shapes(8)]
    assert all(torch.equal(sd[k], v) for k, v in m.state_dict().items())
    # a reference-order state dict round-trips through torch.save and load_state_dict(strict=True), and the module stays flat
    buf = io.BytesIO()
    torch.save(m.state_dict(), buf)
    other = {k: torch.from_numpy(v) for k, v in CI.state_dict(42, 8).items()}
    m.load_state_dict(other, strict=True)
    assert m._is_flat() and not torch.equal(m(x).detach(), before)
    buf.seek(0)
    m.load_state_dict(torch.load(buf), strict=True)
    with torch.no_grad():
        assert m._is_flat() and torch.equal(m(x), before)
    m.to('cpu')
    assert not m._is_flat()                                                       # .to() re-homes: an ordinary module again
    with pytest.raises(RuntimeError, match='not flat'):
        m.sgd_step(flat, flat, 0.001, 0.9, True)


def test_sgd_step_then_forward_packs_nothing(lib):
    from nerfail_amd import ops
    x = images()
    m = module()
    m.flatten_parameters()
    with torch.no_grad():
        m(x)
    assert lib.calls['nerfail_cnn_pack'] == 1
    g = torch.full_like(m._flat, 1e-3)
    buf = torch.zeros_like(m._flat)
    versions = [p._version for p in m.parameters()]
    m.sgd_step(g, buf, 0.001, 0.9, True)
    assert all(p._version > v for p, v in zip(m.parameters(), versions))          # the step told autograd and the caches
    with torch.no_grad():
        stepped = m(x)
    assert lib.calls['nerfail_cnn_pack'] == 1 and lib.calls['nerfail_cnn_sgd_step'] == 1          # ZERO packs after the step
    # ... and that forward saw the stepped weights: an un-flattened module given the same parameters agrees bitwise
    plain = module(trainable=True)
    plain.load_state_dict(m.state_dict(), strict=True)
    with torch.no_grad():
        assert torch.equal(plain(x), stepped)
    assert lib.calls['nerfail_cnn_pack'] == 2
    # an un-flattened module under a stock optimizer step still issues its one pack per step
    for p in plain.parameters():
        p.grad = torch.full_like(p, 1e-3)
    torch.optim.SGD(plain.parameters(), lr=0.001, momentum=0.9).step()
    with torch.no_grad():
        plain(x)
    assert lib.calls['nerfail_cnn_pack'] == 3
    # a write that bypasses sgd_step drops the adopted image: the next forward packs again
    with torch.no_grad():
        m.fc2.bias.add_(1.0)
        m(x)
    assert lib.calls['nerfail_cnn_pack'] == 4
    assert ops.cnn_grad_layout(8)[1] == m._flat.numel()


def test_sgd_step_equals_torch_sgd_on_the_module():
    """Two steps of MyCNN.sgd_step from the gradients of cnn_bwd_weights = two steps of torch.optim.SGD on an ordinary trainable
    module given the same .grad tensors, bitwise (the arithmetic is pinned to torch's CPU kernels in tests/test_cls_train_ref.py;
    torch's HIP kernel fuses differently, so the comparison runs the stock step on the CPU)."""
    from nerfail_amd import ops
    m = module()
    flat = m.flatten_parameters()
    cpu = {k: torch.nn.Parameter(v.detach().cpu().clone()) for k, v in m.state_dict().items()}
    opt = torch.optim.SGD(list(cpu.values()), lr=0.001, momentum=0.9)
    layout, total = ops.cnn_grad_layout(8)
    buf = torch.full_like(flat, 5.0)                                               # garbage before the first step
    rs = np.random.RandomState(3)
    for t in range(2):
        g = torch.from_numpy(rs.standard_normal(total).astype(np.float32) * 0.1)
        for (o, sh), p in zip(layout, cpu.values()):
            p.grad = g[o:o + p.numel()].view(sh).clone()
        opt.step()
        m.sgd_step(g.to(_dev()), buf, 0.001, 0.9, t == 0)
        for k, v in m.state_dict().items():
            assert torch.equal(v.cpu(), cpu[k].detach()), (t, k)


def test_frozen_uses_are_unchanged_on_a_flattened_module():
    x = images(2)
    plain, flat = module(trainable=False), module(trainable=True)
    flat.flatten_parameters()
    outs = []
    for m in (plain, flat):
        m.requires_grad_(False).eval()
        xi = x.clone().requires_grad_(True)
        logits = m(xi)
        d = torch.zeros((3, 2, 8), device=_dev())
        d[0, :, 1], d[1, :, 6], d[2, 0, 3] = 1.0, 1.0, -2.0
        gi = m.input_gradients(logits, d)
        ga = torch.autograd.grad(logits[:, 6].sum(), xi)[0]
        outs.append((logits.detach(), gi, ga))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.equal(outs[1][1][1], outs[1][2])                                  # row 1 of input_gradients is autograd's


def test_deepfool_is_unchanged_on_a_flattened_module():
    import bench_sections as BS
    from nerfail_amd.GaussNet import gauss_net
    from nerfail_amd.deepfool import deepfool
    BS._heavy_imports()
    dev = _dev()
    wi, ori, s_init = BS._attack_inputs(dev, 1, seed=0)
    results = []
    for flatten in (False, True):
        m = module(seed=19, trainable=flatten)
        if flatten:
            m.flatten_parameters()
        m.requires_grad_(False).eval()
        net = gauss_net(dev, 0.02, m, 'my_model', epsilon=None)
        results.append(deepfool((s_init, wi[:1], ori[:1]), 1.0, net, num_classes=8, max_iter=2, m1=1e6, m2=30))
    for a, b in zip(*results):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b)
        else:
            assert a == b
