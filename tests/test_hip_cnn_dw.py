"""-m gpu: the native weight gradients of MyCNN (nerfail_cnn_bwd_weights, torch.ops.nerfail_mi.cnn_bwd_weights,
MyCNN(trainable=True)) against the float64 forced-routing chain of tests/cnn_ref_dw.py (pinned to ATen by
tests/test_cnn_dw_ref.py).

  1 stage by stage   every dW / db element within cnn_ref.elem_bound(K, mag) of float64 on the DEVICE'S OWN operands (the
                     per-stage pooled gradients of the scratch, the workspace, the masks): K = B x conv pixels, any
                     summation order meets it, so a miss is a bug; and the L2 form cnn_ref.l2_bound. fc1, fc2 alike (K = B).
  2 whole chain      all 18 gradients against the float64 chain on the forward's routing: relative L2 within
                     4 x stock fp32's (the same chain with dtype=torch.float32 on the CPU) + 1e-7, per parameter.
  3 fabricated       the same with a made-up workspace, masks and hidden layer, NaNs included.
  4 isolation        reproducible bits, canaries, d_x bitwise cnn_bwd_data's, d_x = NULL, batch of 3 = sum of three batch-1.
  5 module           MyCNN(8, trainable=True): .grad through autograd, a frozen parameter, SGD step, the default's refusal, opcheck.
  6 free routing     against stock PyTorch on the GPU, bound of tests/test_hip_cnn.py (sanity only).
  7 guard pages      one run with unmapped pages behind every tensor."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_inputs as CI
import cnn_ref as R
import cnn_ref_dw as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

NUM_CLASSES = 8
LABEL = 4
CANARY = -12345.5
# (H, W, B, image kinds): the smallest input, odd / even floor-pool drops with a batch sum and partial mask bytes, B = 2, 800 x 800
CASES = [(766, 766, 1, 'n'), (769, 772, 3, 'ncn'), (767, 767, 2, 'cn'), (800, 800, 1, 'c')]


def _dev():
    return torch.device('cuda:0')


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def native(seed, trainable=False, num_classes=NUM_CLASSES):
    from nerfail_amd.MyModel import MyCNN
    sd = CI.state_dict(seed, num_classes)
    m = MyCNN(num_classes, trainable=True) if trainable else MyCNN(num_classes)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return sd, m.to(_dev()).requires_grad_(trainable).eval()


def images(kinds, H, W, seed0):
    return np.stack([CI.cold_tail_image(seed0 + i, H, W)[0] if k == 'c' else R.noise_image(seed0 + i, H, W)
                     for i, k in enumerate(kinds)])


def entry(packed, C, x, ws, masks, d, want_dx=True, fill=CANARY):
    """nerfail_cnn_bwd_weights through the C ABI on canary-filled buffers: (d_params, scratch, d_x or None), device tensors."""
    from nerfail_amd import _lib
    lib = _lib.load()
    B, _, H, W = x.shape
    scratch = torch.full((lib.nerfail_cnn_bwd_weights_scratch_bytes(B, H, W, C) // 4,), fill, dtype=torch.float32, device=_dev())
    dp = torch.full((lib.nerfail_cnn_grad_floats(C),), fill, dtype=torch.float32, device=_dev())
    dx = torch.full((B, 3, H, W), fill, dtype=torch.float32, device=_dev()) if want_dx else None
    _lib.check(lib.nerfail_cnn_bwd_weights(_ptr(packed), C, _ptr(x), _ptr(ws), _ptr(masks), _ptr(d), B, H, W, _ptr(scratch),
                                           _ptr(dp), _ptr(dx), _lib.stream()))
    torch.cuda.synchronize()
    return dp, scratch, dx


def ce_grad(logits):
    d = torch.softmax(logits.double(), 1)
    d[:, LABEL] -= 1.0
    return d.float().contiguous()


@pytest.fixture(scope='module', params=range(len(CASES)), ids=['%dx%dxB%d-%s' % c for c in CASES])
def case(request):
    import nerfail_amd.ops as O
    H, W, B, kinds = CASES[request.param]
    sd, m = native(50 + request.param)
    x = images(kinds, H, W, 300 + 10 * request.param)
    xd = torch.from_numpy(x).to(_dev())
    logits, ws, masks = O.cnn_fwd(m.packed(), xd, NUM_CLASSES, True)
    d = ce_grad(logits)
    dp, scratch, dx = entry(m.packed(), NUM_CLASSES, xd, ws, masks, d)
    acts, hidden = R.split_workspace(ws.cpu().numpy(), B, H, W)
    c = {'H': H, 'W': W, 'B': B, 'sd': sd, 'm': m, 'x': x, 'xd': xd, 'ws': ws, 'masks': masks, 'd': d, 'dp': dp,
         'scratch': scratch, 'dx': dx, 'acts': [R.nchw(a) for a in acts], 'hidden': hidden,
         'codes': R.decode_masks(masks.cpu().numpy(), B, H, W), 'tag': '%dx%d B%d %s' % (H, W, B, kinds)}
    yield c
    c.clear()


def device_stage_refs(x, acts, codes, hidden, d, scratch, H, W):
    """Per parameter (float64 value, magnitude sum, K) recomputed from the device's own operands: the pooled gradients and
    d hidden of the scratch, the forward's acts / codes / hidden, the input."""
    B = x.shape[0]
    pooled, dh, _ = D.split_scratch(scratch, B, H, W)
    refs = {}
    for s, (hin, win, hp, wp) in enumerate(R.stage_dims(H, W)):
        up = D.unpool(R.nchw(pooled[s]), acts[s], codes[s], hin, win, torch.float64)
        xin = R._t(x if s == 0 else acts[s - 1])
        K = B * (hin - 2) * (win - 2)
        refs['conv%d.weight' % (s + 1)] = (D.conv_dw(up, xin).numpy(), D.conv_dw(up.abs(), xin.abs()).numpy(), K)
        refs['conv%d.bias' % (s + 1)] = (up.sum((0, 2, 3)).numpy(), up.abs().sum((0, 2, 3)).numpy(), K)
    dh, dl, hid = R._t(dh), R._t(d), R._t(hidden)
    flat = D.fc1_columns(R._t(acts[6]))
    refs['fc1.weight'] = ((dh.T @ flat).numpy(), (dh.abs().T @ flat.abs()).numpy(), B)
    refs['fc1.bias'] = (dh.sum(0).numpy(), dh.abs().sum(0).numpy(), B)
    refs['fc2.weight'] = ((dl.T @ hid).numpy(), (dl.abs().T @ hid.abs()).numpy(), B)
    refs['fc2.bias'] = (dl.sum(0).numpy(), dl.abs().sum(0).numpy(), B)
    return refs


def _refs(c):
    if 'refs' not in c:
        c['refs'] = device_stage_refs(c['x'], c['acts'], c['codes'], c['hidden'], c['d'].cpu().numpy(),
                                      c['scratch'].cpu().numpy(), c['H'], c['W'])
    return c['refs']


def check_stage_bounds(got, refs, tag):
    worst = {}
    for k, (want, mag, K) in refs.items():
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got[k]), nan), (tag, k, int(np.isnan(got[k]).sum()), int(nan.sum()))
        err = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, np.asarray(got[k], np.float64)) - np.where(nan, 0.0, want)))
        magf = np.where(np.isnan(mag), 0.0, mag)
        el = float((err / np.maximum(R.elem_bound(K, magf), 1e-300)).max())
        l2 = float(np.linalg.norm(err.reshape(-1)) / max(R.l2_bound(K, magf), 1e-300))
        worst[k] = (el, l2)
        print('1 %s %-13s K %8d: largest element %.5f of the worst-case bound, L2 %.4f of the probabilistic bound'
              % (tag, k, K, el, l2))
    for k, (el, l2) in worst.items():
        assert el <= 1.0 and l2 <= 1.0, (tag, k, el, l2)


# ---------------------------------------------------------------------------------------------------------- 1
def test_stage_by_stage_worst_case_bound(case):
    got, _ = D.split_grads(case['dp'].cpu().numpy(), NUM_CLASSES)
    check_stage_bounds(got, _refs(case), case['tag'])


# ---------------------------------------------------------------------------------------------------------- 2 / 3
def check_chain(got, r64, r32, tag):
    fails = []
    for k in D.names(NUM_CLASSES):
        nan = np.isnan(r64[k])
        assert np.array_equal(np.isnan(got[k]), nan), (tag, k, int(np.isnan(got[k]).sum()), int(nan.sum()))
        a, b, c = (np.where(nan, 0.0, np.asarray(v[k], np.float64)) for v in (got, r64, r32))
        n = np.linalg.norm(b.reshape(-1))
        e, e32 = float(np.linalg.norm((a - b).reshape(-1)) / n), float(np.linalg.norm((c - b).reshape(-1)) / n)
        print('%s %-13s relative L2 %.2e (stock fp32 %.2e, ratio %.2f)' % (tag, k, e, e32, e / max(e32, 1e-30)))
        if not e <= 4 * e32 + 1e-7:
            fails.append((k, e, e32))
    assert not fails, (tag, fails)


def test_whole_chain_kernel_routing(case):
    c = case
    d = c['d'].cpu().numpy()
    got, _ = D.split_grads(c['dp'].cpu().numpy(), NUM_CLASSES)
    r64 = D.chain_dw(c['sd'], c['x'], c['acts'], c['codes'], c['hidden'], d, torch.float64, (c['H'], c['W']))[0]
    r32 = D.chain_dw(c['sd'], c['x'], c['acts'], c['codes'], c['hidden'], d, torch.float32, (c['H'], c['W']))[0]
    check_chain(got, r64, r32, '2 ' + c['tag'])


def fabricated(B, H, W, seed):
    """Workspace, codes, masks and hidden no forward produced (tests/test_hip_cnn_stages.py's recipe): values about half <= 0
    with exact 0.0 and -0.0, one NaN per stage and one in hidden, and in every stage the four corner windows of image 0
    pointing at the four window positions (the image-edge conv pixels)."""
    rs = np.random.RandomState(seed)
    ws = rs.normal(size=R.workspace_floats(B, H, W)).astype(np.float32)
    pick = rs.randint(0, 100, size=ws.size)
    ws[pick == 0] = 0.0
    ws[pick == 1] = -0.0
    acts, hidden = R.split_workspace(ws, B, H, W)
    codes = [rs.randint(0, 4, size=(B, a.shape[3], a.shape[1], a.shape[2])).astype(np.uint8) for a in acts]
    for a, c in zip(acts, codes):
        a.reshape(-1)[rs.randint(a.size)] = np.nan
        hp, wp = c.shape[-2:]
        for q, (pr, pc) in enumerate(((0, 0), (0, wp - 1), (hp - 1, 0), (hp - 1, wp - 1))):
            for k in range(4):                                  # channel k % 4 == j: corner q gets position (q + j) % 4
                c[0, k::4, pr, pc] = (q + k) % 4
            a[0, pr, pc, :] = np.abs(a[0, pr, pc, :]) + 0.5     # open gates there
    hidden[0, 7] = np.nan
    return ws, acts, hidden, codes, R.encode_masks(codes)


@pytest.mark.parametrize('HWB', [(766, 766, 1), (769, 772, 3)], ids=['766x766xB1', '769x772xB3'])
def test_whole_chain_fabricated_routing(HWB):
    H, W, B = HWB
    sd, m = native(61 + B)
    ws, acts, hidden, codes, masks = fabricated(B, H, W, H * 1000 + W)
    assert np.isnan(hidden).sum() == 1 and all(np.isnan(a).sum() >= 1 for a in acts)
    x = images('nc' * B, H, W, 500)[:B]
    d = np.random.RandomState(W).normal(size=(B, NUM_CLASSES)).astype(np.float32)
    dp, scratch, dx = entry(m.packed(), NUM_CLASSES, *(torch.from_numpy(a).to(_dev()) for a in (x, ws, masks, d)))
    got, _ = D.split_grads(dp.cpu().numpy(), NUM_CLASSES)
    acts = [R.nchw(a) for a in acts]
    r64, _, _, dx64 = D.chain_dw(sd, x, acts, codes, hidden, d, torch.float64, (H, W))
    r32 = D.chain_dw(sd, x, acts, codes, hidden, d, torch.float32, (H, W))[0]
    assert sum(int(np.isnan(v).sum()) for v in r64.values()) > 0
    tag = '3 %dx%d B%d fabricated' % (H, W, B)
    check_chain(got, r64, r32, tag)
    check_stage_bounds(got, device_stage_refs(x, acts, codes, hidden, d, scratch.cpu().numpy(), H, W), tag)
    nan = np.isnan(dx64)
    assert np.array_equal(np.isnan(dx.cpu().numpy()), nan)
    e = np.linalg.norm(np.where(nan, 0, dx.cpu().numpy() - dx64)) / np.linalg.norm(np.where(nan, 0, dx64))
    assert e < 1e-4, e


# ---------------------------------------------------------------------------------------------------------- 4
def test_reproducible_and_isolated(case):
    import nerfail_amd.ops as O
    c = case
    B, H, W = c['B'], c['H'], c['W']
    packed = c['m'].packed()
    dp2, sc2, dx2 = entry(packed, NUM_CLASSES, c['xd'], c['ws'], c['masks'], c['d'], fill=float('nan'))
    assert torch.equal(c['dp'][c['dp'] == c['dp']], dp2[dp2 == dp2]) and torch.equal(c['dx'], dx2)
    _, defined = D.split_grads(c['dp'].cpu().numpy(), NUM_CLASSES)
    defined = torch.from_numpy(defined).to(_dev())
    assert bool((c['dp'][~defined] == CANARY).all()) and bool(torch.isnan(dp2[~defined]).all())
    assert bool(torch.isfinite(dp2[defined]).all()) and torch.equal(c['dp'][defined], dp2[defined])
    pooled, dh, used = D.split_scratch(sc2.cpu().numpy(), B, H, W)
    assert all(np.isfinite(p).all() for p in pooled) and np.isfinite(dh).all()          # every defined float overwritten
    assert np.array_equal(sc2.cpu().numpy()[:used], c['scratch'].cpu().numpy()[:used])
    assert torch.equal(c['dx'], O.cnn_bwd_data(packed, c['ws'], c['masks'], c['d'], H, W))
    dp3, _, none = entry(packed, NUM_CLASSES, c['xd'], c['ws'], c['masks'], c['d'], want_dx=False)
    assert none is None and torch.equal(dp3, c['dp'])
    opd, opx = O.cnn_bwd_weights(packed, c['xd'], c['ws'], c['masks'], c['d'], True)
    assert torch.equal(opd[defined], c['dp'][defined]) and torch.equal(opx, c['dx']) and not bool(opd[~defined].any())
    if B == 3:                                                  # the batch sum: three batch-1 runs, to test 1's bound
        total = {k: 0.0 for k in D.names(NUM_CLASSES)}
        for i in range(B):
            lg, ws1, mk1 = O.cnn_fwd(packed, c['xd'][i:i + 1].contiguous(), NUM_CLASSES, True)
            d1, _, _ = entry(packed, NUM_CLASSES, c['xd'][i:i + 1].contiguous(), ws1, mk1, c['d'][i:i + 1].contiguous())
            for k, v in D.split_grads(d1.cpu().numpy(), NUM_CLASSES)[0].items():
                total[k] = total[k] + v.astype(np.float64)
        got, _ = D.split_grads(c['dp'].cpu().numpy(), NUM_CLASSES)
        for k, (want, mag, K) in _refs(c).items():
            assert (np.abs(got[k] - total[k]) <= R.elem_bound(K, mag)).all(), k


# ---------------------------------------------------------------------------------------------------------- 5
def test_through_the_module():
    import nerfail_amd.ops as O
    sd, m = native(71, trainable=True)
    m.conv3.bias.requires_grad_(False)
    x = torch.from_numpy(images('cn', 767, 767, 700)).to(_dev())
    y = torch.tensor([LABEL, 1], device=_dev())
    logits = m(x)
    F.cross_entropy(logits, y).backward()
    assert x.grad is None and m.conv3.bias.grad is None
    with torch.no_grad():
        lg, ws, masks = O.cnn_fwd(m.packed(), x, NUM_CLASSES, True)
    lg2 = lg.clone().requires_grad_(True)
    d = torch.autograd.grad(F.cross_entropy(lg2, y), lg2)[0].contiguous()
    dp, dx = O.cnn_bwd_weights(m.packed(), x, ws, masks, d, True)
    assert torch.equal(lg, logits.detach())
    want, _ = D.split_grads(dp.cpu().numpy(), NUM_CLASSES)
    for k, p in m.named_parameters():
        if k != 'conv3.bias':
            assert p.grad is not None and np.array_equal(p.grad.cpu().numpy(), want[k]), k
    m.zero_grad()
    xg = x.clone().requires_grad_(True)
    F.cross_entropy(m(xg), y).backward()
    assert torch.equal(xg.grad, dx) and np.array_equal(m.fc1.weight.grad.cpu().numpy(), want['fc1.weight'])
    # an optimizer step: the next forward runs on the new weights
    m.conv3.bias.requires_grad_(True)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9)
    opt.zero_grad()
    F.cross_entropy(m(x), y).backward()
    opt.step()
    with torch.no_grad():
        after = m(x)
    from nerfail_amd.MyModel import MyCNN
    fresh = MyCNN(NUM_CLASSES, trainable=True).to(_dev())
    fresh.load_state_dict(m.state_dict(), strict=True)
    with torch.no_grad():
        assert not torch.equal(after, logits.detach()) and torch.equal(after, fresh(x))
    # frozen use of a trainable module is the old path: input gradient through cnn_fwd's own node
    m.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    out = m(xg)
    assert O.cnn_fwd_saved(out) is not None
    # the default module still refuses
    _, plain = native(71)
    plain.fc2.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match='weight gradients'):
        plain(x)


def test_opcheck_cnn_bwd_weights():
    import nerfail_amd.ops as O
    _, m = native(72)
    x = torch.from_numpy(images('n', 766, 766, 720)).to(_dev())
    lg, ws, masks = O.cnn_fwd(m.packed(), x, NUM_CLASSES, True)
    for need in (True, False):
        res = torch.library.opcheck(torch.ops.nerfail_mi.cnn_bwd_weights.default, (m.packed(), x, ws, masks, ce_grad(lg), need),
                                    test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_static'))
        assert all(v == 'SUCCESS' for v in res.values()), res
    with pytest.raises(RuntimeError, match='kept no masks'):
        O.cnn_bwd_weights(m.packed(), x, ws, masks[:0], ce_grad(lg), False)
    with pytest.raises(ValueError):
        O.cnn_bwd_weights(m.packed(), x, ws[:-4], masks, ce_grad(lg), False)
    with pytest.raises(ValueError):
        O.cnn_bwd_weights(m.packed(), x, ws, masks[:-1], ce_grad(lg), False)
    with pytest.raises(TypeError):
        O.cnn_bwd_weights(m.packed(), x, ws, masks, ce_grad(lg).double(), False)


# ---------------------------------------------------------------------------------------------------------- 6
def test_against_stock_pytorch_free_routing():
    """Sanity only: the stock module (MIOpen) on the GPU and this module against float64 autograd on the CPU, each free to
    choose its pool argmax. Bound of tests/test_hip_cnn.py's free-routing input gradient: max(2e-2, 4 x stock fp32's)."""
    H = W = 766
    sd, m = native(73, trainable=True)
    x = torch.from_numpy(images('n', H, W, 730))
    y = torch.tensor([LABEL])
    F.cross_entropy(m(x.to(_dev())), y.to(_dev()), reduction='sum').backward()

    def functional(dtype, device):
        p = {k: torch.from_numpy(v).to(device, dtype).requires_grad_(True) for k, v in sd.items()}
        h = x.to(device, dtype)
        for i in range(1, 8):
            h = F.max_pool2d(F.relu(F.conv2d(h, p['conv%d.weight' % i], p['conv%d.bias' % i])), 2)
        h = F.relu(F.linear(h.reshape(1, -1), p['fc1.weight'], p['fc1.bias']))
        F.cross_entropy(F.linear(h, p['fc2.weight'], p['fc2.bias']), y.to(device), reduction='sum').backward()
        return {k: v.grad.double().cpu().numpy() for k, v in p.items()}
    r64, s32 = functional(torch.float64, 'cpu'), functional(torch.float32, _dev())
    for k, p in m.named_parameters():
        n = np.linalg.norm(r64[k])
        e, e32 = np.linalg.norm(p.grad.double().cpu().numpy() - r64[k]) / n, np.linalg.norm(s32[k] - r64[k]) / n
        print('6 %-13s relative L2 to float64 %.2e (stock on the GPU %.2e)' % (k, e, e32))
        assert e <= max(2e-2, 4 * e32), (k, e, e32)


# ---------------------------------------------------------------------------------------------------------- 7
def test_under_guard_pages(rank_launcher):
    rep = rank_launcher(os.path.abspath(__file__), 1, [], timeout=400, env={'NERFAIL_GUARD_ALLOC': '1'})
    log = '\n'.join(rep['logs'])
    assert rep['rc'] == [0], log
    assert 'Memory access fault' not in log and '[guard_alloc] active' in log and 'CNN DW GUARD OK' in log, log


def _guard_child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import guard
    assert guard.install_if_wanted()
    _, m = native(74, trainable=True)
    x = torch.from_numpy(images('ncn', 769, 772, 740)).to(_dev()).requires_grad_(True)
    F.cross_entropy(m(x), torch.tensor([1, 2, 3], device=_dev())).backward()
    torch.cuda.synchronize()
    assert x.grad is not None and all(p.grad is not None for p in m.parameters())
    print('CNN DW GUARD OK', flush=True)


if __name__ == '__main__':
    _guard_child()
