"""CPU only: the float64 references and the buffer codec of tests/cnn_ref.py, which tests/test_hip_cnn_stages.py judges the
MyCNN kernels with. A wrong reference could bless a wrong kernel, so it is pinned to ATen here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_inputs as CI
import cnn_ref as R


def rel_l2(a, b):
    return float(np.linalg.norm((np.asarray(a, np.float64) - b).reshape(-1)) / np.linalg.norm(np.asarray(b).reshape(-1)))


def test_stage_dims_and_accepted_range():
    assert R.stage_dims(800, 800) == [(800, 800, 399, 399), (399, 399, 198, 198), (198, 198, 98, 98), (98, 98, 48, 48),
                                      (48, 48, 23, 23), (23, 23, 10, 10), (10, 10, 4, 4)]
    ok = [h for h in range(700, 960) if R.stage_dims(h, 800) is not None]
    assert ok == list(range(766, 894)) and R.stage_dims(800, 765) is None and R.stage_dims(800, 894) is None


def test_size_list_meets_its_coverage_conditions():
    assert len(R.SIZES) <= 6 and all(B in (1, 3) for _, _, B in R.SIZES)
    assert {(800, 800), (766, 893), (893, 766)} <= {(H, W) for H, W, _ in R.SIZES}
    assert {B for _, _, B in R.SIZES} == {1, 3}
    cov = R.size_coverage(R.SIZES)
    assert len(cov) == 28 and all(cov.values()), [k for k, v in cov.items() if not v]
    # the conditions are not vacuous: the three natural sizes alone miss some
    assert not all(R.size_coverage([(800, 800), (766, 893), (893, 766)]).values())


@pytest.mark.parametrize('HW', [(800, 800), (766, 893), (769, 772), (783, 785)])
def test_mask_codec_round_trip(HW):
    H, W = HW
    B = 2
    rs = np.random.RandomState(H + W)
    dims = R.stage_dims(H, W)
    if HW == (769, 772):
        assert dims[0][3] % 8 == 1 and dims[0][3] % 2 == 1
    codes = [rs.randint(0, 4, size=(B, R.CHANS[s + 1], hp, wp)).astype(np.uint8) for s, (_, _, hp, wp) in enumerate(dims)]
    img = R.encode_masks(codes)
    assert img.dtype == np.uint8 and img.size == R.mask_bytes(B, H, W)
    back = R.decode_masks(img, B, H, W)
    assert all(np.array_equal(a, b) for a, b in zip(codes, back))
    # the layout itself, cell by cell, from the contract's formula (stage 2, a few cells incl. the last column)
    s = 1
    _, _, hp, wp = dims[s]
    C, n8 = R.CHANS[s + 1], (wp + 7) // 8
    o = sum(B * d[2] * ((d[3] + 7) // 8) * 2 * R.CHANS[i + 1] for i, d in enumerate(dims[:s]))
    for b, pr, pc, ch in ((0, 0, 0, 0), (1, hp - 1, wp - 1, C - 1), (1, 3, 9, 5), (0, 7, wp - 2, 17)):
        byte = img[o + (((b * hp + pr) * n8 + (pc >> 3)) * 2 + (pc & 1)) * C + ch]
        assert (byte >> (2 * ((pc & 7) >> 1))) & 3 == codes[s][b, ch, pr, pc]
    # padding cells of a byte are zero: all-3 codes leave the bits beyond wp clear
    full = R.encode_masks([np.full_like(c, 3) for c in codes])
    m = full[o:o + B * hp * n8 * 2 * C].reshape(B, hp, n8, 2, C)
    for cell in range(8):                                       # cell = 2 g + h of the last byte pair
        val = (m[:, :, -1, cell & 1, :] >> (2 * (cell >> 1))) & 3
        assert (val == (3 if (n8 - 1) * 8 + cell < wp else 0)).all()


def test_workspace_split():
    B, H, W = 3, 766, 893
    n = R.workspace_floats(B, H, W)
    acts, hidden = R.split_workspace(np.arange(n, dtype=np.float64), B, H, W)
    assert [a.shape for a in acts] == [(B, hp, wp, R.CHANS[s + 1]) for s, (_, _, hp, wp) in enumerate(R.stage_dims(H, W))]
    assert acts[0][0, 0, 0, 0] == 0 and acts[1].reshape(-1)[0] == acts[0].size and hidden.shape == (B, 512)
    assert hidden.reshape(-1)[-1] == n - 1
    assert R.nchw(acts[6]).shape == (B, 64, 4, 4)


def test_chain_backward_equals_autograd_float64():
    """With the codes ATen's own max_pool2d chose, the forced-routing chain IS the network's gradient: equal to
    torch.autograd in float64 to 1e-12 relative L2, on an odd size (a dropped conv row and column at stage 1) with ties."""
    H, W = 767, 769
    sd = CI.state_dict(7)
    x = np.stack([CI.cold_tail_image(101, H, W)[0], R.noise_image(5, H, W)])
    logits, acts, codes, hidden = R.forward64(sd, x)
    rs = np.random.RandomState(0)
    d_logits = rs.normal(size=logits.shape)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    p = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    h = xt
    for i in range(1, 8):
        h = F.max_pool2d(F.relu(F.conv2d(h, p['conv%d.weight' % i], p['conv%d.bias' % i])), 2)
    h = F.relu(F.linear(h.reshape(h.shape[0], -1), p['fc1.weight'], p['fc1.bias']))
    lg = F.linear(h, p['fc2.weight'], p['fc2.bias'])
    assert np.array_equal(lg.detach().numpy(), logits)
    (lg * torch.from_numpy(d_logits)).sum().backward()
    got = R.chain_backward(sd, acts, codes, hidden, d_logits, torch.float64, (H, W))
    assert got.shape == x.shape and got.dtype == np.float64
    e = rel_l2(got, xt.grad.numpy())
    print('chain_backward(float64) vs autograd: relative L2 %.2e' % e)
    assert e <= 1e-12
    assert not got[:, :, H - 1, :].any() and not got[:, :, :, W - 1].any()      # the dropped conv row / column: no gradient
    # the codes matter: moving every window to the next position is another gradient
    other = R.chain_backward(sd, acts, [(c + 1) & 3 for c in codes], hidden, d_logits, torch.float64, (H, W))
    assert rel_l2(other, xt.grad.numpy()) > 0.5
    # and the same chain in float32 is the yardstick: close, not equal
    e32 = rel_l2(R.chain_backward(sd, acts, codes, hidden, d_logits, torch.float32, (H, W)), got)
    print('chain_backward(float32) vs float64: relative L2 %.2e' % e32)
    assert 0 < e32 < 5e-6


def test_stage_forward_bounds_and_code_rules_on_stock_fp32():
    """Stock fp32 conv2d + max_pool2d meets the two rounding bounds and the argmax rules at every stage (it must: the worst-case
    bound holds for any summation order); a stage that loses one tap of one channel breaks the L2 bound, and codes moved to
    the neighbouring position break the rules. Undecided windows on the noise image: below 1 % of all windows."""
    sd = CI.state_dict(7)
    H, W = 766, 766
    x = torch.from_numpy(R.noise_image(1, H, W))[None]
    und = win = 0
    for s in range(R.STAGES):
        w, b = sd['conv%d.weight' % (s + 1)], sd['conv%d.bias' % (s + 1)]
        K = 9 * w.shape[1]
        pre = F.relu(F.conv2d(x, torch.from_numpy(w), torch.from_numpy(b)))
        got, idx = F.max_pool2d(pre, 2, return_indices=True)
        ref = R.stage_forward64(x.numpy(), w, b)
        magp = F.max_pool2d(ref.mag, 2).numpy()
        err = np.abs(got.double().numpy() - ref.pooled.numpy())
        bound = R.elem_bound(K, magp)
        r_el, r_l2 = float((err / bound).max()), float(np.linalg.norm(err.reshape(-1)) / R.l2_bound(K, magp))
        codes = R.codes_from_indices(idx.numpy(), pre.shape[-1])
        j = R.judge_codes(codes, ref, 2 * bound)
        print('stage %d K %4d: element %.4f, L2 %.4f of the bounds; %s' % (s + 1, K, r_el, r_l2, j))
        assert r_el <= 1 and r_l2 <= 1
        assert j['not_max'] == j['wrong_clear'] == j['wrong_zero'] == 0
        und, win = und + j['undecided'], win + j['windows']
        if s in (1, 6):
            w2 = w.copy()
            w2[:, 3, 1, 2] = 0                                  # one tap of one channel lost
            bad = F.max_pool2d(F.relu(F.conv2d(x, torch.from_numpy(w2), torch.from_numpy(b))), 2)
            r_bad = float(np.linalg.norm((bad.double().numpy() - ref.pooled.numpy()).reshape(-1)) / R.l2_bound(K, magp))
            print('   one tap of one channel lost: L2 %.0f of the bound' % r_bad)
            assert r_bad > 50
            jb = R.judge_codes(codes ^ 1, ref, 2 * bound)
            assert jb['not_max'] > 0.3 * jb['windows'] and jb['wrong_clear'] > 0.3 * jb['windows']
        x = got
    print('undecided windows: %.3f %%' % (100.0 * und / win))
    assert und < 0.01 * win


def test_pack_image_layout():
    for C in (1, 37):
        sd = CI.state_dict(3, C)
        img, defined = R.pack_image(sd, C)
        assert img.size % 4 == 0 and img.dtype == np.float32
        # stage 1 forward [32][10][4]: tap t, channel c of output o; padding channel and tap zero
        f = img[:32 * 40].reshape(32, 10, 4)
        assert f[5, 7, 2] == sd['conv1.weight'][5, 2, 2, 1] and not f[:, 9].any() and not f[:, :, 3].any()
        # fc2 bias is the last region, rounded up to 4 floats
        nb = (C + 3) // 4 * 4
        assert np.array_equal(img[-nb:][:C], sd['fc2.bias']) and defined[-nb:].sum() == C
        # stage 2: forward [64][9][32] right after stage 1's forward and bias; backward [32][9][64] after its own bias
        o = 32 * 40 + 32
        assert img[o + (10 * 9 + 4) * 32 + 7] == sd['conv2.weight'][10, 7, 1, 1]
        o += 64 * 9 * 32 + 64
        assert img[o + (7 * 9 + 4) * 64 + 10] == sd['conv2.weight'][10, 7, 1, 1]
