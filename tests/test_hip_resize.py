"""-m gpu: the opt-in wiring of the native classifier-input stage: gauss_net.native_classifier_input (cold tail, nerfail_s_step,
logit_gradients) and eval_views.evaluate_views(native_resize=True), with a small stock nn.Sequential victim in eval()."""
import numpy as np
import pytest
import torch

import resize_ref as RR
from hiputil import T, N, dev

pytestmark = pytest.mark.gpu
H, W = 48, 44                                   # 299 / 44 = 6.8: the widest inverted range (15) still within the 16 taps


def _problem(seed, B=1, P=3):
    import synth
    from nerfail_amd.GaussNet import create_gauss_w
    rs = np.random.RandomState(seed)
    s = rs.uniform(-40, 40, size=(P, H, W, 4)).astype(np.float32)
    s[..., 3] = rs.choice([0.0, 128.0, 255.0], size=(P, H, W))
    ori = synth.disc_alpha_image(B, H, W, seed=seed + 1)
    dist = np.sort(np.abs(rs.normal(scale=0.02, size=(B, H, W, 8))).astype(np.float32), -1)
    idx = rs.randint(0, P * H * W, size=(B, H, W, 8)).astype(np.float32)
    wi, _ = create_gauss_w(dev(), 0.02)(T(np.stack([dist, idx], 1)))
    return T(s), wi, T(ori)


def _victim(C=8):
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.ReLU(), torch.nn.AdaptiveAvgPool2d(2), torch.nn.Flatten(),
                            torch.nn.Linear(16, C)).to(dev()).eval()
    return m.requires_grad_(False)


def _net(native, name='inception'):
    from nerfail_amd.GaussNet import gauss_net
    net = gauss_net(dev(), 0.02, _victim(), name, epsilon=32.0)
    net.native_classifier_input = native
    return net


def test_the_classifier_input_is_the_definition_and_the_flag_off_is_the_stock_path():
    from nerfail_amd import _resize
    s, wi, ori = _problem(5, B=2)
    seen = []
    for native in (True, False):
        net = _net(native)
        hook = net.model.register_forward_pre_hook(lambda m, a: seen.append(a[0].detach().clone()))
        x, x_rgba, cla, _, ori_cla = net(s, wi, ori)
        hook.remove()
        if native:
            assert np.array_equal(N(seen[0]), RR.forward32(N(x_rgba), 0, 299, 299))
            assert np.array_equal(N(seen[1]), RR.forward32(N(ori.float()), 0, 299, 299))
        else:                                       # the parent commit's path: the same tensors through _resize.resize
            c = x_rgba.detach().permute(0, 3, 1, 2)
            want = _resize.resize(torch.where(c[:, 3:4] > 0, c[:, :3], torch.full_like(c[:, :3], 255.)).contiguous(), 299)
            assert torch.equal(seen[2], want) and torch.equal(cla, net.model(want))
            assert net._last_native is None
    assert np.abs(N(seen[0]) - N(seen[2])).max() < 0.05              # the two definitions agree to float32 rounding of values <= 255


def test_a_my_model_net_is_unaffected_by_the_flag():
    s, wi, ori = _problem(6)
    outs = []
    for native in (True, False):
        net = _net(native, 'my_model')
        outs.append(net(s, wi, ori))
        assert net._last_native is None
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


def test_two_runs_of_nerfail_s_step_give_identical_bits():
    from nerfail_amd.attack import nerfail_s_step
    s, wi, ori = _problem(7, B=2)
    label = torch.tensor(3, device=dev())
    runs = []
    for _ in range(2):
        net = _net(True)
        s1, loss = nerfail_s_step(net, s.clone(), s, wi, ori.to(torch.uint8), label, 2.0, 32.0, False)
        _, _, cla, _, _ = net(s1, wi, ori)
        runs.append((N(s1), N(cla)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert not np.array_equal(runs[0][0], N(s))


def test_logit_gradients_are_the_r1_autograd_slices_bit_for_bit():
    s, wi, ori = _problem(8)
    net = _net(True)
    st = s.clone().requires_grad_(True)
    x, x_rgba, cla, _, _ = net(st, wi, ori)
    assert net._last_native is not None and net._last_native[1] is x_rgba
    classes = [5, 0, 2]
    G = net.logit_gradients(st, wi, x, x_rgba, cla, classes)
    for i, k in enumerate(classes):
        ref = torch.autograd.grad(cla[0, k], st, retain_graph=True)[0]
        assert torch.equal(G[i], ref), k


def test_evaluate_views_native_resize_is_evaluate_record_on_the_definitions_inputs():
    """eval_views.evaluate_views(native_resize=True) against the record of the same steps on inputs resized by resize_ref: the
    metrics on the resized pairs, the classifier on the resized attacked views, the fold. Every field compared exactly. With the
    default the call is model_test's."""
    from nerfail_amd import _lib, eval_views, model_test as MT, ops
    rs = np.random.RandomState(9)
    n = 3
    att = rs.randint(0, 256, size=(n, H, W, 4)).astype(np.uint8)
    org = rs.randint(0, 256, size=(n, H, W, 4)).astype(np.uint8)
    att[..., 3] = rs.randint(0, 2, size=(n, H, W)) * 255
    org[..., 3] = att[..., 3]
    model = _victim()
    got = eval_views.evaluate_views(model, 'inception', T(att), T(org), 2, batch=2, native_resize=True)
    a = RR.forward32(att.astype(np.float32), 0, 299, 299)
    o = RR.forward32(org.astype(np.float32), 0, 299, 299)
    record = torch.zeros(_lib.EVAL_RECORD_DOUBLES, dtype=torch.float64, device=dev())
    with torch.no_grad():
        for b0 in range(0, n, 2):
            ca, co = T(a[b0:b0 + 2]), T(o[b0:b0 + 2])
            rows, _ = ops.eval_view_metrics(MT._flat(ca), _lib.EVAL_FLAT, MT._flat(co), _lib.EVAL_FLAT, False)
            pred, ce = ops.eval_logit_stats(model(ca), 2)
            ops.eval_fold(rows, pred, ce, 8, record)
    assert got == MT.report(record.cpu().numpy(), 2, 8)
    rec = eval_views.evaluate_record(model, 'inception', T(att), T(org), 2, batch=2, native_resize=True)
    assert torch.equal(rec, record)
    off = eval_views.evaluate_record(model, 'inception', T(att), T(org), 2, batch=2)
    assert torch.equal(off, MT.evaluate_record(model, 'inception', T(att), T(org), 2, batch=2))
