"""-m gpu: the native MyCNN victim classifier (nerfail_amd/MyModel.py, nerfail_amd/csrc/cnn.hip): parity with the reference
classifier (fixture g23), with stock torch.nn.functional in float64, pool ties / odd sizes / NaN, reproducibility, the weight
pack's invalidation, the refusals, opcheck, the attack loops with the native victim, and one run under guard pages."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_inputs as CI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda:0')


def native(seed=23, num_classes=24):
    from nerfail_amd.MyModel import MyCNN
    m = MyCNN(num_classes)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CI.state_dict(seed, num_classes).items()}, strict=True)
    return m.to(_dev()).requires_grad_(False).eval()


def ref64(m, x, label=4, dtype=torch.float64):
    """Logits and CE(label, sum) input gradient of the module's own parameters through stock torch.nn.functional on the CPU,
    in fp64 (or `dtype`)."""
    p = {k: v.detach().cpu().to(dtype) for k, v in m.state_dict().items()}
    xt = x.detach().cpu().to(dtype).requires_grad_(True)
    h = xt
    for i in range(1, 8):
        h = F.max_pool2d(F.relu(F.conv2d(h, p['conv%d.weight' % i], p['conv%d.bias' % i])), 2)
    h = F.relu(F.linear(h.reshape(h.shape[0], -1), p['fc1.weight'], p['fc1.bias']))
    logits = F.linear(h, p['fc2.weight'], p['fc2.bias'])
    F.cross_entropy(logits, torch.full((x.shape[0],), label), reduction='sum').backward()
    return logits.detach().double().numpy(), xt.grad.double().numpy()


def run(m, x, label=4):
    x = x.to(_dev()).contiguous().requires_grad_(True)
    logits = m(x)
    F.cross_entropy(logits, torch.full((x.shape[0],), label, device=_dev()), reduction='sum').backward()
    return logits.detach().cpu().double().numpy(), x.grad.cpu().double().numpy()


def l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def check_fp64(m, x):
    """Logits: relative L2 <= 1e-5 against fp64. Input gradient: a 2x2 pool window whose two largest values differ by less
    than fp32 rounding takes another argmax in any fp32 computation than in fp64 and moves a whole patch of the gradient
    (measured relative L2 against fp64 on these inputs: stock fp32 on the CPU 9e-5 .. 3e-1, this kernel 7e-7 .. 3e-1, within
    8x of stock either way). So the gradient bound is max(2e-2, 4 x stock fp32's spread), and signs must agree wherever
    |g| > 1e-3 max|g| but for at most 1e-3 of those entries or 4 x stock fp32's count of flips."""
    lg, g = run(m, x)
    lr, gr = ref64(m, x)
    l32, g32 = ref64(m, x, dtype=torch.float32)
    assert l2(lg, lr) <= max(1e-5, 2 * l2(l32, lr)), (l2(lg, lr), l2(l32, lr))
    assert l2(g, gr) <= max(2e-2, 4 * l2(g32, gr)), (l2(g, gr), l2(g32, gr))
    big = np.abs(gr) > 1e-3 * np.abs(gr).max()
    flips, flips32 = int((np.sign(g[big]) != np.sign(gr[big])).sum()), int((np.sign(g32[big]) != np.sign(gr[big])).sum())
    assert flips <= max(4 * flips32, 1e-3 * big.sum()), (flips, flips32, int(big.sum()))
    print('fp64 check: logits %.2e (fp32 %.2e), grad %.2e (fp32 %.2e), sign flips %d (fp32 %d) of %d'
          % (l2(lg, lr), l2(l32, lr), l2(g, gr), l2(g32, gr), flips, flips32, int(big.sum())))
    return lg, g


def images(n, seed0=0, H=800, W=800):
    return torch.from_numpy(np.stack([CI.cold_tail_image(seed0 + i, H, W)[0] for i in range(n)]))


# ---------------------------------------------------------------------------------------------------------- 1. reference parity
def test_reference_held_parity(golden):
    g = golden('g23_mycnn')
    m = native(int(g['weight_seed']))
    assert list(m.state_dict().keys()) == [str(k) for k in g['keys']]
    sd = CI.state_dict(int(g['weight_seed']))
    assert np.allclose([np.asarray(v, np.float64).sum() for v in sd.values()], g['weight_sums'], rtol=0, atol=1e-9)
    imgs, edges = zip(*[CI.cold_tail_image(int(s)) for s in g['image_seeds']])
    assert np.allclose([np.asarray(i, np.float64).sum() for i in imgs], g['image_sums'], rtol=0, atol=1e-3)
    lg, gx = run(m, torch.from_numpy(np.stack(imgs)), int(g['label']))
    crops, blocks, norms = map(np.stack, zip(*[CI.summaries(gx[i], edges[i]) for i in range(len(imgs))]))
    for name, got in (('logits', lg), ('crop', crops), ('blocks', blocks), ('norm', norms)):
        r32, r64 = g[name + '_f32'], g[name + '_f64']
        bound = 2 * np.linalg.norm(r32 - r64) + 1e-6 * np.linalg.norm(r64)
        assert np.linalg.norm(got - r64) <= bound, (name, np.linalg.norm(got - r64), bound)


# ---------------------------------------------------------------------------------------------------------- 2. fp64 check
@pytest.mark.parametrize('B', [1, 2, 8])
def test_matches_fp64_functional(B):
    check_fp64(native(7), images(B, seed0=100 + B))


# ---------------------------------------------------------------------------------------------------------- 3. edge cases
def test_pool_ties_constant_and_single_pixel():
    m = native(11)
    check_fp64(m, torch.full((1, 3, 800, 800), 255.0))
    rs = np.random.RandomState(3)
    x = np.zeros((2, 3, 800, 800), np.float32)
    pos = rs.randint(0, 4, size=(2, 400, 400))                 # one bright pixel per 2x2 window, in a random position
    yy, xx = np.mgrid[0:400, 0:400]
    for b in range(2):
        x[b, :, 2 * yy + pos[b] // 2, 2 * xx + pos[b] % 2] = 255.0
    check_fp64(m, torch.from_numpy(x))


@pytest.mark.parametrize('HW', [(799, 801), (801, 799), (766, 893)])
def test_odd_sizes(HW):
    check_fp64(native(12), images(1, seed0=7, H=HW[0], W=HW[1]))


def test_batch_9_and_nan():
    m = native(13)
    check_fp64(m, images(9, seed0=20))
    x = images(2, seed0=40)
    x[1, 1, 300, 301] = float('nan')
    with torch.no_grad():
        got = m(x.to(_dev())).cpu().numpy()
    ref = ref64(m, x)[0]
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got[1]).all()
    assert l2(got[0], ref[0]) <= 1e-5


# ---------------------------------------------------------------------------------------------------------- 4. behaviour
def test_bitwise_reproducible_and_pack_invalidation():
    m = native(14)
    x = images(2, seed0=60)
    l1, g1 = run(m, x)
    l2_, g2 = run(m, x)
    assert np.array_equal(l1, l2_) and np.array_equal(g1, g2)
    p0 = m.packed()
    with torch.no_grad():
        m.conv3.weight.mul_(1.5)
    assert m.packed() is not p0
    l3, g3 = run(m, x)
    fresh = native(14)
    with torch.no_grad():
        fresh.conv3.weight.mul_(1.5)
    l4, g4 = run(fresh, x)
    assert not np.array_equal(l1, l3) and np.array_equal(l3, l4) and np.array_equal(g3, g4)


def test_reference_state_dict_and_refusals(golden):
    from nerfail_amd.MyModel import MyCNN
    g = golden('g23_mycnn')
    sd = {str(k): torch.zeros([int(d) for d in s if d]) for k, s in zip(g['keys'], g['shapes'])}
    MyCNN(24).load_state_dict(sd, strict=True)
    m = native(15)
    x = images(1, seed0=80)
    with pytest.raises(RuntimeError, match='no CPU path'):
        m(x)
    with pytest.raises(TypeError):
        m(x.to(_dev()).double())
    with pytest.raises(ValueError):
        m(torch.zeros((1, 3, 700, 800), device=_dev()))
    with pytest.raises(ValueError):
        m(torch.zeros((1, 4, 800, 800), device=_dev()))
    m.fc2.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match='weight gradients'):
        m(x.to(_dev()))
    with torch.no_grad():
        m(x.to(_dev()))                                        # under no_grad a trainable parameter is fine


def test_no_masks_without_input_grad():
    import nerfail_amd.ops as O
    m = native(16)
    x = images(1, seed0=90).to(_dev())
    _, _, masks = O.cnn_fwd(m.packed(), x, 24, False)
    assert masks.numel() == 0
    with torch.no_grad():
        a = m(x)
    assert torch.equal(a, m(x))


# ---------------------------------------------------------------------------------------------------------- 5. opcheck
def test_opcheck_cnn_fwd():
    import nerfail_amd.ops  # noqa: F401
    m = native(17)
    x = images(1, seed0=95).to(_dev()).requires_grad_(True)
    res = torch.library.opcheck(torch.ops.nerfail_mi.cnn_fwd.default, (m.packed(), x, 24, True),
                                test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_static'))
    assert all(v == 'SUCCESS' for v in res.values()), res


def test_repeated_backward_retain_graph():
    m = native(18)
    x = images(1, seed0=96).to(_dev()).requires_grad_(True)
    logits = m(x)
    gs = [torch.autograd.grad(logits[0, k], x, retain_graph=True)[0] for k in (0, 3, 0)]
    assert torch.equal(gs[0], gs[2]) and not torch.equal(gs[0], gs[1])


# ---------------------------------------------------------------------------------------------------------- 6. attack integration
def _stock(m):
    chans = CI.CHANS
    layers = []
    for i in range(7):
        layers += [torch.nn.Conv2d(chans[i], chans[i + 1], 3), torch.nn.ReLU(), torch.nn.MaxPool2d(2)]
    s = torch.nn.Sequential(*layers, torch.nn.Flatten(), torch.nn.Linear(1024, 512), torch.nn.ReLU(), torch.nn.Linear(512, m.num_classes))
    src = list(m.state_dict().values())
    with torch.no_grad():
        for p, v in zip(s.parameters(), src):
            p.copy_(v)
    return s.to(_dev()).requires_grad_(False).eval()


def test_attack_step_and_deepfool_with_native_victim():
    import bench_sections as BS
    from nerfail_amd.GaussNet import gauss_net
    from nerfail_amd.attack import nerfail_s_step
    from nerfail_amd.deepfool import deepfool
    BS._heavy_imports()
    dev = _dev()
    m = native(19, num_classes=8)
    wi, ori, s_init = BS._attack_inputs(dev, 2, seed=0)
    label = torch.tensor(4, device=dev)
    outs = []
    for victim in (m, _stock(m)):
        net = gauss_net(dev, 0.02, victim, 'my_model', epsilon=None)
        net.cache_ori_cla = True
        s, loss = nerfail_s_step(net, s_init.clone(), s_init, wi, ori.to(torch.uint8), label, 2.0, 32.0, False)
        outs.append((s.cpu().numpy(), float(loss)))
    (sa, la), (sb, lb) = outs
    assert abs(la - lb) <= 1e-5 * abs(lb)
    assert (sa != sb).mean() < 1e-3, (sa != sb).mean()      # sign flips only where the gradient is rounding noise
    net = gauss_net(dev, 0.02, m, 'my_model', epsilon=None)
    net.cache_ori_cla = True
    key = net._classifier_state_key()
    with torch.no_grad():
        m.fc1.bias.add_(0.0)
    assert net._classifier_state_key() != key
    r = deepfool((s_init, wi[:1], ori[:1]), 1.0, net, num_classes=8, max_iter=2, m1=1e6, m2=30)
    assert r[1] >= 1


# ---------------------------------------------------------------------------------------------------------- 7. guard pages
def test_under_guard_pages(rank_launcher):
    rep = rank_launcher(os.path.abspath(__file__), 1, [], timeout=400, env={'NERFAIL_GUARD_ALLOC': '1'})
    log = '\n'.join(rep['logs'])
    assert rep['rc'] == [0], log
    assert 'Memory access fault' not in log and '[guard_alloc] active' in log and 'CNN GUARD OK' in log, log


def _guard_child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import guard
    assert guard.install_if_wanted()
    for HW, B in (((800, 800), 1), ((799, 801), 2)):
        m = native(21)
        x = images(B, seed0=5, H=HW[0], W=HW[1])
        run(m, x)
    torch.cuda.synchronize()
    print('CNN GUARD OK', flush=True)


if __name__ == '__main__':
    _guard_child()
