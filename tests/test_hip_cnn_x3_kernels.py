"""-m gpu: the bf16x3 kernels of the MyCNN victim (nerfail_amd/csrc/cnn_x3.hip) stage by stage, held to the yardstick of the
exact kernels: tests/cnn_ref.py's float64 stage reference with the routing as an input, and the bounds, rules and backward
criterion of tests/test_hip_cnn_stages.py (imported, not restated). Nothing is loosened for the second arithmetic.

  image            nerfail_cnn_pack_x3 bit for bit the numpy image of tests/cnn_x3_ref.py;
  stage 1          the x3 forward's first pooled output and mask codes bit for bit the exact forward's;
  forward 2..7     every pooled element within elem_bound(K, mag) of float64 on the stage's actual f32 input, the stage within
                   l2_bound, NaN positions equal, the FC head by its bounds;
  argmax codes     judge_codes with t = 2 x the element bound; undecided windows of a noise image below 1 % overall and at
                   each of stages 1..3;
  backward chain   within 4 x stock fp32's own error + 1e-7 of float64 on the same routing, overall and on the six outermost
                   rows and columns: on the x3 forward's own buffers, on fabricated buffers, on an exact forward's buffers;
  bits             run to run, batch position, multi slices;
  buffers          everything written, nothing behind the buffers touched, scratch contents irrelevant.

Measured on the cases below (largest element / worst-case bound, stage L2 / probabilistic bound), bf16x3 | exact f32: the table
"bf16x3 victim: per-stage error" in DESIGN.md."""
import numpy as np
import pytest
import torch

import cnn_inputs as CI
import cnn_ref as R
import cnn_x3_ref as X
import test_hip_cnn_stages as S

pytestmark = pytest.mark.gpu

NUM_CLASSES = S.NUM_CLASSES
CASES = X.CASES


def _dev():
    return torch.device('cuda:0')


def _x3(m):
    import nerfail_amd.ops as O
    return O.cnn_pack_x3(m.packed(), m.num_classes)


def forward_x3(m, x):
    import nerfail_amd.ops as O
    out = O.cnn_fwd_x3(m.packed(), _x3(m), torch.from_numpy(x).to(_dev()), m.num_classes, True)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module', params=range(len(CASES)), ids=['%dx%dxB%d-%s' % c for c in CASES])
def case(request):
    H, W, B, kinds = CASES[request.param]
    sd, m = S.native(57 + request.param)
    x = S.images(kinds, H, W, 300 + 10 * request.param)
    logits, ws, masks = forward_x3(m, x)
    c = {'H': H, 'W': W, 'B': B, 'kinds': kinds, 'sd': sd, 'm': m, 'x': x, 'logits': logits, 'ws': ws, 'masks': masks,
         'img': _x3(m), 'exact': S.forward(m, x), 'tag': 'x3 %dx%d B%d %s' % (H, W, B, kinds)}
    yield c
    c.clear()


def _report(c):
    if 'report' not in c:
        c['report'] = S.stage_report(c['sd'], c['x'], c['ws'].cpu().numpy(), c['masks'].cpu().numpy(), c['logits'].cpu().numpy())
    return c['report']


def _routing(ws, masks, B, H, W):
    acts, hidden = R.split_workspace(ws.cpu().numpy(), B, H, W)
    return [R.nchw(a) for a in acts], R.decode_masks(masks.cpu().numpy(), B, H, W), hidden


# ---------------------------------------------------------------------------------------------------------- image
@pytest.mark.parametrize('C', [8, 37])
def test_x3_image_bit_for_bit(C):
    from nerfail_amd import _lib
    from nerfail_amd.MyModel import MyCNN
    lib = _lib.load()
    sd = CI.state_dict(90 + C, C)
    m = MyCNN(C)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(_dev())
    want = X.x3_image(sd, C)
    n = lib.nerfail_cnn_x3_packed_bytes(C)
    assert n == want.size
    whole, img, tail = S._with_tail(n, torch.uint8, 0x5a, 0xa5)
    _lib.check(lib.nerfail_cnn_pack_x3(S._ptr(m.packed()), C, S._ptr(img), _lib.stream()))
    torch.cuda.synchronize()
    assert np.array_equal(img.cpu().numpy(), want)
    assert bool((tail == 0xa5).all())


# ---------------------------------------------------------------------------------------------------------- stage 1
def test_stage_1_is_the_exact_kernels(case):
    B, H, W = case['B'], case['H'], case['W']
    _, ws0, mk0 = case['exact']
    hp, wp = R.stage_dims(H, W)[0][2:]
    n_act, n_mask = B * hp * wp * 32, B * hp * ((wp + 7) // 8) * 2 * 32
    assert torch.equal(case['ws'][:n_act], ws0[:n_act])
    assert torch.equal(case['masks'][:n_mask], mk0[:n_mask])
    assert not torch.equal(case['ws'][n_act:], ws0[n_act:])                # (and stage 2 on is another arithmetic)


# ---------------------------------------------------------------------------------------------------------- forward stages
def test_forward_stages(case):
    rep, head = _report(case)
    for r in rep + head:
        print('%s %s K %4d: largest element %.4f of the worst-case bound, L2 %.4f of the probabilistic bound'
              % (case['tag'], r.get('name', 'stage %d' % r.get('stage', 0)), r['K'], r['elem'], r['l2']))
    for r in rep + head:
        assert r['elem'] <= 1.0, r
        assert r['l2'] <= 1.0, r
    assert all(r['nan_equal'] for r in rep)


def test_forward_nan_positions():
    sd, m = S.native(13)
    H = W = 767
    x = S.images('c', H, W, 40)
    x[0, 1, 300, 301] = np.nan
    logits, ws, masks = forward_x3(m, x)
    rep, _ = S.stage_report(sd, x, ws.cpu().numpy(), masks.cpu().numpy(), logits.cpu().numpy())
    acts, hidden = R.split_workspace(ws.cpu().numpy(), 1, H, W)
    counts = [int(np.isnan(a).sum()) for a in acts]
    print('x3 NaN pixel: NaN outputs per stage', counts)
    assert counts[0] == 4 * 32 and all(n > 0 for n in counts)
    for r in rep:
        assert r['nan_equal'], r['stage']
        assert r['elem'] <= 1.0 and r['l2'] <= 1.0, r
        assert all(j['not_max'] == j['wrong_clear'] == j['wrong_zero'] == 0 for j in r['judge']), r
    assert np.isnan(hidden).all() and bool(torch.isnan(logits).all())


# ---------------------------------------------------------------------------------------------------------- argmax codes
def test_argmax_codes(case):
    rep, _ = _report(case)
    for i, kind in enumerate(case['kinds']):
        und = sum(r['judge'][i]['undecided'] for r in rep)
        win = sum(r['judge'][i]['windows'] for r in rep)
        per = ['%.3f' % (100.0 * r['judge'][i]['undecided'] / r['judge'][i]['windows']) for r in rep]
        print('%s image %d (%s): undecided windows %.3f %% of all, per stage %% %s'
              % (case['tag'], i, 'noise' if kind == 'n' else 'cold tail', 100.0 * und / win, ' '.join(per)))
    for r in rep:
        for j in r['judge']:
            assert j['not_max'] == 0 and j['wrong_clear'] == 0 and j['wrong_zero'] == 0, (r['stage'], j)
    for i, kind in enumerate(case['kinds']):
        if kind == 'n':
            assert sum(r['judge'][i]['undecided'] for r in rep) < 0.01 * sum(r['judge'][i]['windows'] for r in rep)
            for r in rep[:3]:
                assert r['judge'][i]['undecided'] < 0.01 * r['judge'][i]['windows'], r['stage']


# ---------------------------------------------------------------------------------------------------------- backward chain
def _dense(case):
    return np.ascontiguousarray(np.random.RandomState(case['B'] + case['H']).normal(size=(case['B'], NUM_CLASSES)), np.float32)


def _both_backwards(case, ws, masks, d, tag):
    """x3 and exact backward on the same buffers against float64 / stock fp32 of the same routing. The exact kernel's figures
    are printed first: if x3 misses the criterion, the line above says what the exact kernel did in the same run."""
    import nerfail_amd.ops as O
    B, H, W = case['B'], case['H'], case['W']
    acts, codes, hidden = _routing(ws, masks, B, H, W)
    r64 = R.chain_backward(case['sd'], acts, codes, hidden, d, torch.float64, (H, W))
    r32 = R.chain_backward(case['sd'], acts, codes, hidden, d, torch.float32, (H, W))
    dd = torch.from_numpy(d).to(_dev())
    exact = O.cnn_bwd_data(case['m'].packed(), ws, masks, dd, H, W).cpu().numpy()
    got = O.cnn_bwd_data_x3(case['m'].packed(), case['img'], ws, masks, dd, H, W).cpu().numpy()
    S.check_backward(exact, r64, r32, '%s %s, exact f32 kernel' % (case['tag'], tag))
    S.check_backward(got, r64, r32, '%s %s, bf16x3 kernel' % (case['tag'], tag))


def test_backward_chain_own_routing(case):
    """On the x3 forward's own workspace and masks: the cross-entropy gradient of its logits."""
    lg = case['logits'].cpu().double()
    ce = torch.softmax(lg, 1)
    ce[:, S.LABEL] -= 1.0
    _both_backwards(case, case['ws'], case['masks'], np.ascontiguousarray(ce.numpy(), np.float32), 'own routing, cross-entropy')


def test_backward_chain_on_an_exact_forwards_buffers(case):
    """Interchangeability: the workspace and masks of nerfail_cnn_fwd handed to nerfail_cnn_bwd_data_x3; a dense d_logits."""
    _, ws0, mk0 = case['exact']
    _both_backwards(case, ws0, mk0, _dense(case), 'exact forward\'s buffers, dense')


@pytest.mark.parametrize('HWB', [c[:3] for c in CASES], ids=['%dx%dxB%d' % c[:3] for c in CASES])
def test_backward_chain_fabricated_routing(HWB):
    from nerfail_amd import _lib
    H, W, B = HWB
    lib = _lib.load()
    sd, m = S.native(131 + B + H % 7)
    img = _x3(m)
    ws, acts, hidden, codes, masks = S.fabricated(B, H, W, H * 1000 + W + 1)
    d = np.random.RandomState(W + 1).normal(size=(B, NUM_CLASSES)).astype(np.float32)
    acts = [R.nchw(a) for a in acts]
    r64 = R.chain_backward(sd, acts, codes, hidden, d, torch.float64, (H, W))
    r32 = R.chain_backward(sd, acts, codes, hidden, d, torch.float32, (H, W))
    g_ws, g_masks, g_d = (torch.from_numpy(a).to(_dev()) for a in (ws, masks, d))
    for name, call in (('exact f32', lambda sc, dx: lib.nerfail_cnn_bwd_data(S._ptr(m.packed()), NUM_CLASSES, S._ptr(g_ws), S._ptr(g_masks),
                                                                               S._ptr(g_d), B, H, W, S._ptr(sc), S._ptr(dx), _lib.stream())),
                       ('bf16x3', lambda sc, dx: lib.nerfail_cnn_bwd_data_x3(S._ptr(m.packed()), S._ptr(img), NUM_CLASSES, S._ptr(g_ws),
                                                                             S._ptr(g_masks), S._ptr(g_d), B, H, W, S._ptr(sc), S._ptr(dx),
                                                                             _lib.stream()))):
        scratch = torch.empty((lib.nerfail_cnn_bwd_scratch_bytes(B, H, W) // 4,), dtype=torch.float32, device=_dev())
        dx = torch.full((B, 3, H, W), float('nan'), dtype=torch.float32, device=_dev())
        _lib.check(call(scratch, dx))
        torch.cuda.synchronize()
        S.check_backward(dx.cpu().numpy(), r64, r32, 'x3 %dx%d B%d fabricated routing, %s kernel' % (H, W, B, name))


# ---------------------------------------------------------------------------------------------------------- bits
def test_two_forwards_are_equal_and_a_batch_is_its_images(case):
    import nerfail_amd.ops as O
    again = forward_x3(case['m'], case['x'])
    for a, b in zip(again, (case['logits'], case['ws'], case['masks'])):
        assert torch.equal(a, b)
    if case['B'] > 1:
        B, H, W = case['B'], case['H'], case['W']
        acts, hidden = R.split_workspace(case['ws'].cpu().numpy(), B, H, W)
        codes = R.decode_masks(case['masks'].cpu().numpy(), B, H, W)
        for b in range(B):
            l1, ws1, mk1 = forward_x3(case['m'], case['x'][b:b + 1])
            a1, h1 = R.split_workspace(ws1.cpu().numpy(), 1, H, W)
            c1 = R.decode_masks(mk1.cpu().numpy(), 1, H, W)
            assert torch.equal(l1[0], case['logits'][b])
            assert all(np.array_equal(p[0].view(np.uint32), q[b].view(np.uint32)) for p, q in zip(a1, acts))
            assert np.array_equal(h1[0].view(np.uint32), hidden[b].view(np.uint32))
            assert all(np.array_equal(p[0], q[b]) for p, q in zip(c1, codes))


@pytest.mark.parametrize('RB', [(1, 1), (8, 1), (3, 2)], ids=['R1B1', 'R8B1', 'R3B2'])
def test_multi_slices_are_the_single_backward(RB):
    import nerfail_amd.ops as O
    Rr, B = RB
    H, W = 767, 767
    sd, m = S.native(77)
    img = _x3(m)
    x = S.images('cn'[:B], H, W, 500)
    _, ws, masks = forward_x3(m, x)
    d = np.random.RandomState(Rr * 10 + B).normal(size=(Rr, B, NUM_CLASSES)).astype(np.float32)
    if Rr > 1:
        d[1] = 0.0                                                        # a zero row
        d[Rr - 1, B - 1, 3] = np.nan                                      # and a NaN in the last one
    d = torch.from_numpy(d).to(_dev())
    got = O.cnn_bwd_data_multi_x3(m.packed(), img, ws, masks, d, H, W)
    assert tuple(got.shape) == (Rr, B, 3, H, W)
    for r in range(Rr):
        one = O.cnn_bwd_data_x3(m.packed(), img, ws, masks, d[r].contiguous(), H, W)
        assert torch.equal(got[r].view(torch.int32), one.view(torch.int32)), r
    if Rr > 1:
        assert not bool(got[1].any()) and bool(torch.isnan(got[Rr - 1, B - 1]).any()) and bool(torch.isfinite(got[0]).all())


# ---------------------------------------------------------------------------------------------------------- buffers
@pytest.mark.parametrize('HWB', [(767, 767, 1), (766, 893, 3)], ids=['767x767xB1', '766x893xB3'])
def test_everything_written_nothing_beyond(HWB):
    from nerfail_amd import _lib
    H, W, B = HWB
    lib = _lib.load()
    sd, m = S.native(17)
    img = _x3(m)
    nan = float('nan')
    x = torch.from_numpy(S.images('cn' * B, H, W, 70)[:B]).to(_dev())
    n_ws, n_mk = lib.nerfail_cnn_workspace_bytes(B, H, W, NUM_CLASSES) // 4, lib.nerfail_cnn_mask_bytes(B, H, W)
    n_sc = lib.nerfail_cnn_bwd_scratch_bytes(B, H, W) // 4
    runs = []
    for mask_fill in (0x00, 0xff):
        ws_all, ws, ws_tail = S._with_tail(n_ws, torch.float32, nan, nan)
        mk_all, mk, mk_tail = S._with_tail(n_mk, torch.uint8, mask_fill, 0xa5)
        logits = torch.full((B, NUM_CLASSES), nan, dtype=torch.float32, device=_dev())
        _lib.check(lib.nerfail_cnn_fwd_x3(S._ptr(m.packed()), S._ptr(img), NUM_CLASSES, S._ptr(x), B, H, W, S._ptr(ws), S._ptr(mk),
                                          S._ptr(logits), _lib.stream()))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(ws).any()) and not bool(torch.isnan(logits).any())
        assert bool(torch.isnan(ws_tail).all()) and bool((mk_tail == 0xa5).all())
        runs.append((ws, mk, logits))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    ws, mk, logits = runs[0]
    d = torch.softmax(logits.double(), 1)
    d[:, S.LABEL] -= 1.0
    d = d.float().contiguous()
    outs = []
    for scratch_fill in (nan, 0.0):
        sc_all, sc, sc_tail = S._with_tail(n_sc, torch.float32, scratch_fill, nan)
        dx_all, dx, dx_tail = S._with_tail(B * 3 * H * W, torch.float32, nan, nan)
        _lib.check(lib.nerfail_cnn_bwd_data_x3(S._ptr(m.packed()), S._ptr(img), NUM_CLASSES, S._ptr(ws), S._ptr(mk), S._ptr(d), B, H, W,
                                               S._ptr(sc), S._ptr(dx), _lib.stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dx).all())
        assert bool(torch.isnan(sc_tail).all()) and bool(torch.isnan(dx_tail).all())
        outs.append(dx)
    assert torch.equal(outs[0], outs[1]) and bool((outs[0] != 0).any())
    assert torch.equal(ws, runs[1][0]) and torch.equal(mk, runs[1][1])          # the backward's inputs are not written
