"""-m gpu: the bf16x3 victim as a product: MyCNN(precision='bf16x3') as a module (state dict, accuracy, autograd,
input_gradients, the weight-image cache, the original-logit cache of gauss_net) and inside the graph-free loops (IGSM-2D,
the 2-D DeepFool, a NeRFail-S step), with the launch trace as the witness of which conv kernels ran; and the dispatch
refactor's guard: a default victim's forward_masks / backward_data are bit for bit the exact ops called directly."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import cnn_inputs as CI
import test_hip_cnn as TC

pytestmark = pytest.mark.gpu

X3_FWD = ['cnn_x3_conv_fwd_s%d' % s for s in range(2, 8)]
X3_BWD = ['cnn_x3_conv_bwd_s%d' % s for s in range(2, 8)]
EXACT = ['cnn_conv_fwd_s%d' % s for s in range(2, 8)] + ['cnn_conv_bwd_s%d' % s for s in range(2, 8)]


def dev():
    return torch.device('cuda:0')


def victim(seed, precision, num_classes=8):
    from nerfail_amd.MyModel import MyCNN
    m = MyCNN(num_classes, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CI.state_dict(seed, num_classes).items()}, strict=True)
    return m.to(dev()).requires_grad_(False).eval()


class Trace:
    """The library's launch trace (common.h: every launched kernel's name on stderr) switched on for a block, read through
    pytest's capfd."""
    def __init__(self, capfd):
        from nerfail_amd import _lib
        self.word = ctypes.c_int.in_dll(_lib.load(), '_ZN7nerfail7g_traceE')
        self.capfd, self.names = capfd, []

    def __enter__(self):
        torch.cuda.synchronize()
        self.capfd.readouterr()
        self.old, self.word.value = self.word.value, 1
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.word.value = self.old
        err = self.capfd.readouterr().err
        self.names = [ln[len('[nerfail] '):].strip() for ln in err.splitlines() if ln.startswith('[nerfail] ')]

    def assert_x3(self, backward=True):
        got = collections.Counter(self.names)
        assert all(got[n] > 0 for n in X3_FWD + (X3_BWD if backward else [])), got
        assert not any(got[n] for n in EXACT), got
        assert got['cnn_conv_fwd_s1'] > 0 and got['cnn_fc_fwd'] > 0           # stage 1 and the head stay exact
        if backward:
            assert got['cnn_conv1_bwd'] > 0 and got['cnn_fc_bwd'] > 0


# ---------------------------------------------------------------------------------------------------------- module
def test_module_against_fp64():
    """The criterion tests/test_hip_cnn.py applies to the exact module (check_fp64), on the bf16x3 module."""
    m = victim(7, 'bf16x3', 24)
    TC.check_fp64(m, TC.images(2, seed0=102, H=767, W=783))


def test_input_gradients_are_autograd_bitwise(capfd):
    m = victim(9, 'bf16x3')
    x = TC.images(2, seed0=31, H=767, W=767).to(dev()).requires_grad_(True)
    with Trace(capfd) as tr:
        logits = m(x)
        d = torch.randn(3, 2, 8, device=dev())
        G = m.input_gradients(logits, d)
    tr.assert_x3()
    for r in range(3):
        one = torch.autograd.grad(logits, x, d[r], retain_graph=True)[0]
        assert torch.equal(G[r].view(torch.int32), one.view(torch.int32)), r
    # the backward follows the family that made `logits`, not the module's precision at the time of the call
    m.precision = 'f32'
    assert torch.equal(m.input_gradients(logits, d), G)
    exact = m(x)
    m.precision = 'bf16x3'
    Ge = m.input_gradients(exact, d)
    assert torch.equal(Ge[0], torch.autograd.grad(exact, x, d[0], retain_graph=True)[0]) and not torch.equal(Ge, G)


class CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ('nerfail_cnn_pack', 'nerfail_cnn_pack_x3'):
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


def test_a_parameter_write_repacks_the_x3_image_once(monkeypatch):
    from nerfail_amd import _lib
    lib = CountingLib(_lib.load())
    monkeypatch.setattr(_lib, '_lib', lib)
    m = victim(11, 'bf16x3')
    x = TC.images(1, seed0=5, H=767, W=767).to(dev())
    with torch.no_grad():
        a = m(x)
        m(x)
        assert dict(lib.calls) == {'nerfail_cnn_pack': 1, 'nerfail_cnn_pack_x3': 1}
        m.conv4.weight.mul_(1.25)
        b = m(x)
        m(x)
        m.forward_masks(x)
        assert dict(lib.calls) == {'nerfail_cnn_pack': 2, 'nerfail_cnn_pack_x3': 2}
        m.precision = 'f32'
        m(x)
        m.precision = 'bf16x3'
        assert torch.equal(m(x), b) and not torch.equal(a, b)
        assert dict(lib.calls) == {'nerfail_cnn_pack': 2, 'nerfail_cnn_pack_x3': 2}     # the switch itself packs nothing
    lib.calls.clear()
    d = victim(11, 'f32')
    with torch.no_grad():
        d(x)
    assert dict(lib.calls) == {'nerfail_cnn_pack': 1}                                   # a default victim never makes the image


@pytest.fixture(scope='module')
def scene():
    import bench_sections as BS
    BS._heavy_imports()
    wi, ori, s_init = BS._attack_inputs(dev(), 1, seed=0)
    return wi, ori.to(torch.uint8), s_init


def test_switching_precision_refreshes_the_original_logits(scene):
    from nerfail_amd.GaussNet import gauss_net
    wi, ori, s_init = scene
    m = victim(19, 'f32')
    net = gauss_net(dev(), 0.02, m, 'my_model', epsilon=None)
    ids = ['view-a']
    ori_f32 = net.attack_forward(s_init, wi, ori, view_ids=ids)[2].clone()
    assert torch.equal(net.attack_forward(s_init, wi, ori, view_ids=ids)[2], ori_f32)
    m.precision = 'bf16x3'
    ori_x3 = net.attack_forward(s_init, wi, ori, view_ids=ids)[2].clone()
    fresh = gauss_net(dev(), 0.02, victim(19, 'bf16x3'), 'my_model', epsilon=None).attack_forward(s_init, wi, ori, view_ids=ids)[2]
    assert torch.equal(ori_x3, fresh) and not torch.equal(ori_x3, ori_f32)
    m.precision = 'f32'
    assert torch.equal(net.attack_forward(s_init, wi, ori, view_ids=ids)[2], ori_f32)


# ---------------------------------------------------------------------------------------------------------- loops
@pytest.fixture(scope='module')
def store():
    rs = np.random.RandomState(7)
    images = rs.randint(0, 256, size=(2, 766, 766, 4)).astype(np.uint8)
    images[..., 3] = np.where(rs.uniform(size=(2, 766, 766)) < 0.7, 255, 0)
    return torch.from_numpy(images).to(dev())


def test_igsm_2d_with_an_x3_victim(store, capfd):
    from nerfail_amd import attack
    m = victim(23, 'bf16x3')
    runs = []
    for _ in range(2):
        with Trace(capfd) as tr:
            res = attack.igsm_2d(m, 'my_model', store, 3, 2, a=2., epsilon=4., targeted=False, batch_size=2, log=None, native=True)
        tr.assert_x3()
        runs.append(res)
    assert torch.equal(runs[0].best, runs[1].best) and torch.equal(runs[0].last, runs[1].last) and runs[0].stats == runs[1].stats
    assert bool(runs[0].last.any())


def test_deepfool_2d_native_with_an_x3_victim(store, capfd):
    from nerfail_amd import deepfool as DF
    from nerfail_amd.GaussNet import universal_2D_net
    m = victim(23, 'bf16x3')
    net = universal_2D_net(dev(), 0.02, m, 'my_model')
    table = torch.zeros((766, 766, 3), device=dev())
    args = dict(num_classes=8, max_iter=2, target_label=None, overshoot=50., m1=0, m2=1, images=store, view=1)
    runs = []
    for _ in range(2):
        with Trace(capfd) as tr:
            out = DF.deepfool_2d_native((table, None), None, net, **args)
        tr.assert_x3()
        assert out[5] is not None and out[1] >= 1                             # the native path ran and iterated
        runs.append(out)
    assert runs[0][1] == runs[1][1] and runs[0][5] == runs[1][5]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][4], runs[1][4])


def test_nerfail_s_step_with_an_x3_victim(scene, capfd):
    from nerfail_amd.GaussNet import gauss_net
    from nerfail_amd.attack import nerfail_s_step
    wi, ori, s_init = scene
    m = victim(19, 'bf16x3')
    label = torch.tensor(4, device=dev())
    runs = []
    for _ in range(2):
        net = gauss_net(dev(), 0.02, m, 'my_model', epsilon=None)
        with Trace(capfd) as tr:
            s, loss = nerfail_s_step(net, s_init.clone(), s_init, wi, ori, label, 2.0, 32.0, False)
        tr.assert_x3()
        runs.append((s, float(loss)))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    net = gauss_net(dev(), 0.02, victim(19, 'f32'), 'my_model', epsilon=None)
    s_e, loss_e = nerfail_s_step(net, s_init.clone(), s_init, wi, ori, label, 2.0, 32.0, False)
    assert abs(runs[0][1] - float(loss_e)) <= 1e-5 * abs(float(loss_e))       # f32-accurate: the exact victim's loss
    assert float((runs[0][0] != s_e).float().mean()) < 1e-3                   # sign flips only where the gradient is rounding noise


# ---------------------------------------------------------------------------------------------------------- default victim
def test_a_default_victim_dispatches_to_the_exact_ops(capfd):
    import nerfail_amd.ops as O
    m = victim(29, 'f32')
    x = TC.images(2, seed0=61, H=767, W=767).to(dev())
    d1 = torch.randn(2, 8, device=dev())
    d3 = torch.randn(3, 2, 8, device=dev())
    with Trace(capfd) as tr:
        logits, ws, masks = m.forward_masks(x)
        g1 = m.backward_data(ws, masks, d1, 767, 767)
        g3 = m.backward_data(ws, masks, d3, 767, 767)
    assert not any(n.startswith('cnn_x3') or n == 'cnn_pack_x3' for n in tr.names) and 'cnn_conv_fwd_s2' in tr.names
    assert logits.grad_fn is None and g1.grad_fn is None
    l0, ws0, mk0 = O.cnn_fwd(m.packed(), x, 8, True)
    assert torch.equal(logits, l0) and torch.equal(ws, ws0) and torch.equal(masks, mk0)
    assert torch.equal(g1, O.cnn_bwd_data(m.packed(), ws0, mk0, d1, 767, 767))
    assert torch.equal(g3, O.cnn_bwd_data_multi(m.packed(), ws0, mk0, d3, 767, 767))
    with torch.no_grad():
        assert torch.equal(m(x), l0)
    m.precision = 'bf16x3'
    lx, wsx, mkx = m.forward_masks(x)
    assert torch.equal(lx, O.cnn_fwd_x3(m.packed(), m.packed_x3(), x, 8, True)[0]) and not torch.equal(lx, l0)
    assert torch.equal(m.backward_data(wsx, mkx, d3, 767, 767), O.cnn_bwd_data_multi_x3(m.packed(), m.packed_x3(), wsx, mkx, d3, 767, 767))
