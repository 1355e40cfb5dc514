"""-m gpu: the MyCNN kernels (nerfail_amd/csrc/cnn.hip) stage by stage, with the pool routing held fixed.

tests/test_hip_cnn.py judges the whole network against a float64 run that is free to choose its own pool argmax, which can
only bound the input gradient to a few percent. Here the reference (tests/cnn_ref.py, pinned to ATen by tests/test_cnn_ref.py)
takes the routing the kernel itself published in `workspace` / `masks` (include/nerfail_hip.h, buffer contract) - or routing the
test made up - so every operation is a linear map and is held to f32 rounding level:

  forward stages   every pooled output within the worst-case rounding bound of a length-K f32 dot product of its f64 value on
                   the stage's ACTUAL f32 input, the stage as a whole within the probabilistic bound; NaN positions exact;
  argmax codes     a maximum up to rounding everywhere, float64's argmax where the window is clearly ordered, position 0 where
                   the window is clearly all zero; all 0 on a constant image;
  backward chain   d_x within 4 x stock fp32's own error (same routing, CPU) of float64, overall and on the six outermost rows
                   and columns, with the forward's routing and with fabricated workspace / masks / hidden;
  buffers          everything written, nothing behind the buffers touched, scratch contents irrelevant;
  weight image     bit for bit the documented layout.

Sizes: cnn_ref.SIZES (their tile / mask / floor-pool residues are asserted by tests/test_cnn_ref.py). Images: cold-tail images
(white background: exact ties outside the object) and uniform noise (no ties).

Undecided windows: the rules leave a window undecided when its two largest values are within t = 2 x the element bound and it
is not clearly all zero. t grows with K while the spread of a stage's values grows with sqrt(K), so the share rises with depth
whatever the noise amplitude (stock fp32 on the CPU, +-255 / 0..255 / +-1 noise alike: 0.002 % at stage 1, 0.08 %, 0.3 %, 1.0 %,
3.7 %, 4.3 %, 3.3 % at stage 7); stages 1..3 hold nine tenths of all windows. The condition asserted is: below 1 % of ALL windows
of a noise image, and below 1 % at each of stages 1..3 (0.18 % overall with stock fp32)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_inputs as CI
import cnn_ref as R

pytestmark = pytest.mark.gpu

NUM_CLASSES = 24
LABEL = 4
TAIL = 4096                      # bytes of canary behind every buffer of the ctypes tests
# (H, W, B, kinds of the B images): both kinds at the attack's own size, mixed batches at B = 3
CASES = [(800, 800, 1, 'c'), (800, 800, 1, 'n'), (766, 893, 3, 'cnc'), (893, 766, 1, 'n'), (767, 767, 1, 'c'),
         (769, 772, 3, 'ncn'), (783, 785, 1, 'n')]
assert sorted({c[:3] for c in CASES}) == sorted(R.SIZES)


def _dev():
    return torch.device('cuda:0')


def native(seed, num_classes=NUM_CLASSES):
    from nerfail_amd.MyModel import MyCNN
    sd = CI.state_dict(seed, num_classes)
    m = MyCNN(num_classes)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return sd, m.to(_dev()).requires_grad_(False).eval()


def images(kinds, H, W, seed0):
    return np.stack([CI.cold_tail_image(seed0 + i, H, W)[0] if k == 'c' else R.noise_image(seed0 + i, H, W)
                     for i, k in enumerate(kinds)])


def forward(m, x):
    import nerfail_amd.ops as O
    logits, ws, masks = O.cnn_fwd(m.packed(), torch.from_numpy(x).to(_dev()), m.num_classes, True)
    torch.cuda.synchronize()
    return logits, ws, masks


def stage_report(sd, x, ws, masks, logits):
    """Per stage and image: the kernel's pooled output and codes against stage_forward64 of the stage's actual f32 input."""
    B, _, H, W = x.shape
    acts, hidden = R.split_workspace(ws, B, H, W)
    codes = R.decode_masks(masks, B, H, W)
    rep = []
    for s in range(R.STAGES):
        w, b = sd['conv%d.weight' % (s + 1)], sd['conv%d.bias' % (s + 1)]
        K = 9 * w.shape[1]
        r = {'stage': s + 1, 'K': K, 'elem': 0.0, 'err2': 0.0, 'mag2': 0.0, 'nan_equal': True, 'judge': []}
        for i in range(B):
            xin = x[i:i + 1] if s == 0 else R.nchw(acts[s - 1][i:i + 1])
            ref = R.stage_forward64(xin, w, b)
            got = R.nchw(acts[s][i:i + 1]).astype(np.float64)
            want, magp = ref.pooled.numpy(), F.max_pool2d(ref.mag, 2).numpy()
            nan = np.isnan(want)
            r['nan_equal'] &= bool(np.array_equal(np.isnan(got), nan))
            bound = R.elem_bound(K, magp)
            err = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, want)))
            fin = ~np.isnan(bound)
            r['elem'] = max(r['elem'], float((err[fin] / bound[fin]).max()))
            r['err2'] += float((err[fin] ** 2).sum())
            r['mag2'] += float((magp[fin] ** 2).sum())
            r['judge'].append(R.judge_codes(codes[s][i:i + 1], ref, 2 * np.where(fin, bound, 0.0)))
        r['l2'] = float(np.sqrt(r['err2']) / (np.sqrt(K + 2) * R.U * np.sqrt(r['mag2'])))
        rep.append(r)
    flat = R.nchw(acts[6]).reshape(B, -1)                       # PyTorch's flatten order c * 16 + y * 4 + x
    head = []
    for name, xin, got, wk, bk, relu in (('fc1', flat, hidden, 'fc1.weight', 'fc1.bias', True),
                                         ('fc2', hidden, logits, 'fc2.weight', 'fc2.bias', False)):
        y, mag = R.linear64(xin, sd[wk], sd[bk])
        y, mag = (F.relu(y) if relu else y).numpy(), mag.numpy()
        K = sd[wk].shape[1]
        err = np.abs(np.asarray(got, np.float64) - y)
        head.append({'name': name, 'K': K, 'elem': float((err / R.elem_bound(K, mag)).max()),
                     'l2': float(np.linalg.norm(err.reshape(-1)) / R.l2_bound(K, mag))})
    return rep, head


@pytest.fixture(scope='module', params=range(len(CASES)), ids=['%dx%dxB%d-%s' % c for c in CASES])
def case(request):
    H, W, B, kinds = CASES[request.param]
    sd, m = native(7 + request.param)
    x = images(kinds, H, W, 100 + 10 * request.param)
    logits, ws, masks = forward(m, x)
    c = {'H': H, 'W': W, 'B': B, 'kinds': kinds, 'sd': sd, 'm': m, 'x': x, 'logits': logits, 'ws': ws, 'masks': masks,
         'tag': '%dx%d B%d %s' % (H, W, B, kinds)}
    yield c
    c.clear()


def _report(c):
    if 'report' not in c:
        c['report'] = stage_report(c['sd'], c['x'], c['ws'].cpu().numpy(), c['masks'].cpu().numpy(), c['logits'].cpu().numpy())
    return c['report']


# ---------------------------------------------------------------------------------------------------------- 3a forward stages
def test_forward_stages(case):
    """Every element within (K + 2) 2^-24 mag + K 2^-126 (worst case, any summation order: zero exceptions), the stage within
    sqrt(K + 2) 2^-24 ||mag||_2 (probabilistic); the FC head by the same two bounds."""
    rep, head = _report(case)
    for r in rep:
        print('3a %s stage %d K %4d: largest element %.4f of the worst-case bound, L2 %.4f of the probabilistic bound'
              % (case['tag'], r['stage'], r['K'], r['elem'], r['l2']))
    for h in head:
        print('3a %s %s K %4d: largest element %.4f of the worst-case bound, L2 %.4f of the probabilistic bound'
              % (case['tag'], h['name'], h['K'], h['elem'], h['l2']))
    for r in rep + head:
        assert r['elem'] <= 1.0, r
        assert r['l2'] <= 1.0, r
    assert all(r['nan_equal'] for r in rep)


def test_forward_nan_positions():
    """One NaN pixel: isnan of every stage's pooled output equals isnan of the float64 stage on that stage's actual input, and
    the code of a window that holds a NaN points at one."""
    sd, m = native(13)
    x = images('c', 800, 800, 40)
    x[0, 1, 300, 301] = np.nan
    logits, ws, masks = forward(m, x)
    rep, _ = stage_report(sd, x, ws.cpu().numpy(), masks.cpu().numpy(), logits.cpu().numpy())
    acts, hidden = R.split_workspace(ws.cpu().numpy(), 1, 800, 800)
    counts = [int(np.isnan(a).sum()) for a in acts]
    print('3a NaN pixel: NaN outputs per stage', counts)
    assert counts[0] == 4 * 32 and all(n > 0 for n in counts)   # input (300, 301) is in conv pixels 298..300 x 299..301: 2 x 2 windows
    for r in rep:
        assert r['nan_equal'], r['stage']
        assert r['elem'] <= 1.0 and r['l2'] <= 1.0, r
        assert all(j['not_max'] == j['wrong_clear'] == j['wrong_zero'] == 0 for j in r['judge']), r
    assert np.isnan(hidden).all() and bool(torch.isnan(logits).all())


# ---------------------------------------------------------------------------------------------------------- 3b argmax codes
def test_argmax_codes(case):
    """The rules of cnn_ref.judge_codes with t = twice the element bound of 3a; undecided windows of a noise image: below 1 % of
    all its windows and below 1 % at each of stages 1..3 (module docstring)."""
    rep, _ = _report(case)
    for i, kind in enumerate(case['kinds']):
        und = sum(r['judge'][i]['undecided'] for r in rep)
        win = sum(r['judge'][i]['windows'] for r in rep)
        per = ['%.3f' % (100.0 * r['judge'][i]['undecided'] / r['judge'][i]['windows']) for r in rep]
        print('3b %s image %d (%s): undecided windows %.3f %% of all, per stage %% %s'
              % (case['tag'], i, 'noise' if kind == 'n' else 'cold tail', 100.0 * und / win, ' '.join(per)))
    for r in rep:
        for j in r['judge']:
            assert j['not_max'] == 0 and j['wrong_clear'] == 0 and j['wrong_zero'] == 0, (r['stage'], j)
    for i, kind in enumerate(case['kinds']):
        if kind == 'n':
            assert sum(r['judge'][i]['undecided'] for r in rep) < 0.01 * sum(r['judge'][i]['windows'] for r in rep)
            for r in rep[:3]:
                assert r['judge'][i]['undecided'] < 0.01 * r['judge'][i]['windows'], r['stage']


@pytest.mark.parametrize('HW', [(800, 800), (769, 772)])
def test_constant_image_codes_all_zero(HW):
    """All four conv pixels of a window see identical operands in identical order: an exact tie in any arithmetic, first wins."""
    sd, m = native(11)
    H, W = HW
    _, ws, masks = forward(m, np.full((2, 3, H, W), 255.0, np.float32))
    acts, _ = R.split_workspace(ws.cpu().numpy(), 2, H, W)
    for s, c in enumerate(R.decode_masks(masks.cpu().numpy(), 2, H, W)):
        assert not c.any(), (s + 1, int((c != 0).sum()))
        assert (acts[s] == acts[s][0, 0, 0][None, None, None, :]).all(), s + 1


# ---------------------------------------------------------------------------------------------------------- 3c / 3d backward
def check_backward(got, r64, r32, tag):
    """relative L2 and max-abs / max-abs <= 4 x stock fp32's + 1e-7; the L2 bound again on each of the six outermost rows and
    columns against that row's own reference norm (a row whose reference is exactly zero must be exactly zero)."""
    nan = np.isnan(r64)
    assert np.array_equal(np.isnan(got), nan), (tag, int(np.isnan(got).sum()), int(nan.sum()))
    got, r64, r32 = (np.where(nan, 0.0, np.asarray(a, np.float64)) for a in (got, r64, r32))

    def l2(a, sel):
        return float(np.linalg.norm((a[sel] - r64[sel]).reshape(-1)) / np.linalg.norm(r64[sel].reshape(-1)))
    everything = (slice(None),) * 4
    e, e32 = l2(got, everything), l2(r32, everything)
    mx, mx32 = (float(np.abs(a - r64).max() / np.abs(r64).max()) for a in (got, r32))
    H, W = got.shape[2:]
    worst, lines, fails = 0.0, [], []
    for axis, n in ((2, H), (3, W)):
        for k in (0, 1, 2, n - 3, n - 2, n - 1):
            sel = (slice(None), slice(None), k, slice(None)) if axis == 2 else (slice(None), slice(None), slice(None), k)
            name = '%s %d' % ('row' if axis == 2 else 'column', k)
            if not r64[sel].any():
                if got[sel].any():
                    fails.append(name + ': reference exactly zero, kernel not')
                continue
            a, a32 = l2(got, sel), l2(r32, sel)
            worst = max(worst, a / a32)
            if not a <= 4 * a32 + 1e-7:
                fails.append('%s: %.3e against stock fp32 %.3e' % (name, a, a32))
    print('%s: relative L2 %.2e (stock fp32 %.2e, ratio %.2f), max-abs / max-abs %.2e (stock fp32 %.2e, ratio %.2f), worst '
          'edge row / column ratio %.2f' % (tag, e, e32, e / e32, mx, mx32, mx / mx32, worst))
    assert e <= 4 * e32 + 1e-7, (tag, e, e32)
    assert mx <= 4 * mx32 + 1e-7, (tag, mx, mx32)
    assert not fails, (tag, fails)


def test_backward_chain_kernel_routing(case):
    """d_x of nerfail_cnn_bwd_data on the forward's own workspace and masks against the float64 chain fed the same workspace,
    decoded codes and hidden: the cross-entropy gradient of the forward's logits, and a dense random d_logits."""
    import nerfail_amd.ops as O
    B, H, W = case['B'], case['H'], case['W']
    acts, hidden = R.split_workspace(case['ws'].cpu().numpy(), B, H, W)
    acts = [R.nchw(a) for a in acts]
    codes = R.decode_masks(case['masks'].cpu().numpy(), B, H, W)
    lg = case['logits'].cpu().double()
    ce = torch.softmax(lg, 1)
    ce[:, LABEL] -= 1.0
    dense = np.random.RandomState(B + H).normal(size=tuple(lg.shape))
    assert (np.abs(dense) > 1e-4).all()
    for name, d in (('cross-entropy', ce.numpy()), ('dense', dense)):
        d = np.ascontiguousarray(d, np.float32)
        got = O.cnn_bwd_data(case['m'].packed(), case['ws'], case['masks'], torch.from_numpy(d).to(_dev()), H, W).cpu().numpy()
        r64 = R.chain_backward(case['sd'], acts, codes, hidden, d, torch.float64, (H, W))
        r32 = R.chain_backward(case['sd'], acts, codes, hidden, d, torch.float32, (H, W))
        check_backward(got, r64, r32, '3c %s %s' % (case['tag'], name))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _with_tail(n, dtype, fill, tail_fill):
    """A device buffer of n elements filled with `fill` and TAIL bytes of canary behind it: (whole, buffer, tail)."""
    k = TAIL // torch.empty((), dtype=dtype).element_size()
    whole = torch.empty((n + k,), dtype=dtype, device=_dev())
    whole[:n] = fill
    whole[n:] = tail_fill
    return whole, whole[:n], whole[n:]


def fabricated(B, H, W, seed):
    """Workspace, codes and masks no forward produced: values about half <= 0 with exact 0.0 and -0.0 among them and one NaN
    per stage, all four window positions equally likely, a random hidden layer."""
    rs = np.random.RandomState(seed)
    ws = rs.normal(size=R.workspace_floats(B, H, W)).astype(np.float32)
    pick = rs.randint(0, 100, size=ws.size)
    ws[pick == 0] = 0.0
    ws[pick == 1] = -0.0
    acts, hidden = R.split_workspace(ws, B, H, W)               # views
    for a in acts:
        a.reshape(-1)[rs.randint(a.size)] = np.nan
    codes = [rs.randint(0, 4, size=(B, a.shape[3], a.shape[1], a.shape[2])).astype(np.uint8) for a in acts]
    return ws, acts, hidden, codes, R.encode_masks(codes)


@pytest.mark.parametrize('HWB', R.SIZES, ids=['%dx%dxB%d' % s for s in R.SIZES])
def test_backward_chain_fabricated_routing(HWB):
    """The scatter and the gates independently of the forward: nerfail_cnn_bwd_data through the C ABI on a fabricated workspace,
    masks and hidden layer, same reference and bounds as with the kernel's own routing."""
    from nerfail_amd import _lib
    H, W, B = HWB
    lib = _lib.load()
    sd, m = native(31 + B + H % 7)
    ws, acts, hidden, codes, masks = fabricated(B, H, W, H * 1000 + W)
    assert [int(np.signbit(a[a == 0]).sum()) > 0 and int((~np.signbit(a[a == 0])).sum()) > 0 for a in acts[:5]] == [True] * 5
    d = np.random.RandomState(W).normal(size=(B, NUM_CLASSES)).astype(np.float32)
    assert ws.nbytes == lib.nerfail_cnn_workspace_bytes(B, H, W, NUM_CLASSES) and masks.size == lib.nerfail_cnn_mask_bytes(B, H, W)
    scratch = torch.empty((lib.nerfail_cnn_bwd_scratch_bytes(B, H, W) // 4,), dtype=torch.float32, device=_dev())
    dx = torch.full((B, 3, H, W), float('nan'), dtype=torch.float32, device=_dev())
    g_ws, g_masks, g_d = (torch.from_numpy(a).to(_dev()) for a in (ws, masks, d))
    _lib.check(lib.nerfail_cnn_bwd_data(_ptr(m.packed()), NUM_CLASSES, _ptr(g_ws), _ptr(g_masks), _ptr(g_d), B, H, W,
                                        _ptr(scratch), _ptr(dx), _lib.stream()))
    torch.cuda.synchronize()
    acts = [R.nchw(a) for a in acts]
    r64 = R.chain_backward(sd, acts, codes, hidden, d, torch.float64, (H, W))
    r32 = R.chain_backward(sd, acts, codes, hidden, d, torch.float32, (H, W))
    check_backward(dx.cpu().numpy(), r64, r32, '3d %dx%d B%d fabricated routing' % (H, W, B))


# ---------------------------------------------------------------------------------------------------------- 3e buffers
@pytest.mark.parametrize('HWB', [(800, 800, 1), (769, 772, 3)], ids=['800x800xB1', '769x772xB3'])
def test_everything_written_nothing_beyond(HWB):
    """Forward on a NaN workspace and 0x00 / 0xff masks: no NaN left, the two mask images byte-identical (every byte is
    written, padding bits included), logits bitwise equal. Backward with scratch NaN / zero and d_x NaN: d_x finite and bitwise
    equal. 4 KB of canary behind d_x, workspace, masks and scratch untouched."""
    from nerfail_amd import _lib
    H, W, B = HWB
    lib = _lib.load()
    sd, m = native(17)
    nan = float('nan')
    x = torch.from_numpy(images('cn' * B, H, W, 70)[:B]).to(_dev())
    n_ws, n_mk = lib.nerfail_cnn_workspace_bytes(B, H, W, NUM_CLASSES) // 4, lib.nerfail_cnn_mask_bytes(B, H, W)
    n_sc = lib.nerfail_cnn_bwd_scratch_bytes(B, H, W) // 4
    assert n_ws == R.workspace_floats(B, H, W) and n_mk == R.mask_bytes(B, H, W)
    runs = []
    for mask_fill in (0x00, 0xff):
        ws_all, ws, ws_tail = _with_tail(n_ws, torch.float32, nan, nan)
        mk_all, mk, mk_tail = _with_tail(n_mk, torch.uint8, mask_fill, 0xa5)
        logits = torch.full((B, NUM_CLASSES), nan, dtype=torch.float32, device=_dev())
        _lib.check(lib.nerfail_cnn_fwd(_ptr(m.packed()), NUM_CLASSES, _ptr(x), B, H, W, _ptr(ws), _ptr(mk), _ptr(logits),
                                       _lib.stream()))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(ws).any()) and not bool(torch.isnan(logits).any())
        assert bool(torch.isnan(ws_tail).all()) and bool((mk_tail == 0xa5).all())
        runs.append((ws, mk, logits))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    ws, mk, logits = runs[0]
    d = torch.softmax(logits.double(), 1)
    d[:, LABEL] -= 1.0
    d = d.float().contiguous()
    outs = []
    for scratch_fill in (nan, 0.0):
        sc_all, sc, sc_tail = _with_tail(n_sc, torch.float32, scratch_fill, nan)
        dx_all, dx, dx_tail = _with_tail(B * 3 * H * W, torch.float32, nan, nan)
        _lib.check(lib.nerfail_cnn_bwd_data(_ptr(m.packed()), NUM_CLASSES, _ptr(ws), _ptr(mk), _ptr(d), B, H, W, _ptr(sc),
                                            _ptr(dx), _lib.stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dx).all())
        assert bool(torch.isnan(sc_tail).all()) and bool(torch.isnan(dx_tail).all())
        outs.append(dx)
    assert torch.equal(outs[0], outs[1]) and bool((outs[0] != 0).any())
    assert torch.equal(ws, runs[1][0]) and torch.equal(mk, runs[1][1])          # the backward's inputs are not written


# ---------------------------------------------------------------------------------------------------------- 3f weight image
@pytest.mark.parametrize('C', [1, 24, 37])
def test_weight_image_bit_for_bit(C):
    """nerfail_cnn_pack against cnn_ref.pack_image: forward [Cout][tap][Cin] (stage 1: 10 taps x 4 channels, the padding exactly
    0), backward [Cin][tap][Cout], the raw stage-1 copy, fc1T / fc1P in NHWC column order, biases, fc2; every region rounded up
    to 4 floats (their contents unspecified), the total nerfail_cnn_packed_floats."""
    from nerfail_amd import _lib
    lib = _lib.load()
    sd = CI.state_dict(40 + C, C)
    want, defined = R.pack_image(sd, C)
    n = lib.nerfail_cnn_packed_floats(C)
    assert n == want.size
    src = [torch.from_numpy(v).to(_dev()) for v in sd.values()]
    assert len(src) == 18
    whole, packed, tail = _with_tail(n, torch.float32, float('nan'), float('nan'))
    ptrs = (ctypes.c_void_p * len(src))(*[p.data_ptr() for p in src])
    _lib.check(lib.nerfail_cnn_pack(ptrs, C, _ptr(packed), _lib.stream()))
    torch.cuda.synchronize()
    got = packed.cpu().numpy()
    assert np.array_equal(got.view(np.uint32)[defined], want.view(np.uint32)[defined])
    assert bool(torch.isnan(tail).all())
