"""-m gpu: the layout of the bf16x3 inference kernel on 16x16x32 MFMAs (mlp_x3.hip) - the weight image byte for byte
against a numpy split with the k permutation, ragged last tiles with a guarded output tail, and run-to-run equality
over a multi-round persistent grid."""
import numpy as np
import pytest
import torch

import synth
from hiputil import T, N, dev

pytestmark = pytest.mark.gpu


def _net(D, skips, seed):
    from nerfail_amd.run_nerf_helpers import NeRF
    sd = synth.nerf_state_dict(D=D, W=256, skips=tuple(skips), seed=seed)
    net = NeRF(D=D, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=list(skips), use_viewdirs=True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return sd, net.requires_grad_(False).to(dev())


def _enc_channel(s, h, bands):
    """Input channel of encoding k-step s in half h (mlp_layout.h enc_channel); -1 = zero padding."""
    if s < 3 * bands:
        return 3 + 6 * (s // 3) + 3 * h + s % 3
    if s == 3 * bands:
        return h
    if s == 3 * bands + 1:
        return -1 if h else 2
    return -1


def _bf16_rn(x):
    """float32 -> the bf16 bit pattern nearest to it (ties to even), as uint16."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def _split3(w):
    hi = _bf16_rn(w)
    r = (w - _bf16_f32(hi)).astype(np.float32)
    mid = _bf16_rn(r)
    r = (r - _bf16_f32(mid)).astype(np.float32)
    return hi, mid, _bf16_rn(r)


def _expected_image(sd, D, skip):
    """[k32 step][16-row out tile][plane][lane][8 bf16] per layer; element j of lane group g in step u of a part is input
    channel 32u + 4g + (j & 3) + 16 (j >> 2) of a hidden part, and encoding k-step 16u + 4(g >> 1) + 8(j >> 2) + (j & 3)
    of half g & 1 of an encoding part."""
    lane = np.arange(64)
    g, row16 = lane >> 4, lane & 15
    out = []
    for l in range(D + 2):
        if l < D:
            w = sd['pts_linears.%d.weight' % l]
        elif l == D:
            w = sd['feature_linear.weight']
        else:
            w = sd['views_linears.0.weight']
        parts = []                                     # (kind, first input column of the part)
        if l == 0:
            parts.append(('emb', 0))
        elif skip >= 0 and l == skip + 1 and l < D:
            parts += [('emb', 0), ('hid', 63)]
        else:
            parts.append(('hid', 0))
        if l == D + 1:
            parts.append(('dir', 256))
        OT = w.shape[0] // 16
        for kind, c0 in parts:
            steps = {'emb': 2, 'hid': 8, 'dir': 1}[kind]
            for u in range(steps):
                cols = np.zeros((64, 8), np.int64)
                for j in range(8):
                    if kind == 'hid':
                        cols[:, j] = c0 + 32 * u + 4 * g + (j & 3) + 16 * (j >> 2)
                    else:
                        st = 16 * u + 4 * (g >> 1) + 8 * (j >> 2) + (j & 3)
                        bands = 10 if kind == 'emb' else 4
                        ch = np.array([_enc_channel(int(s), int(h), bands) for s, h in zip(st, g & 1)])
                        cols[:, j] = np.where(ch >= 0, c0 + ch, -1)
                for t in range(OT):
                    rows = 16 * t + row16
                    vals = np.where(cols >= 0, w[rows[:, None], np.maximum(cols, 0)], 0.).astype(np.float32)
                    for plane in _split3(vals):
                        out.append(plane.reshape(-1))
    return np.concatenate(out)


@pytest.mark.parametrize('D,skips', [(8, [4]), (2, [])])
def test_x3_image_is_the_split_with_the_k_permutation(D, skips):
    sd, net = _net(D, skips, seed=41 + D)
    img = net.packed_x3()
    assert img is not None
    got = N(img).view(np.uint16)
    exp = _expected_image(sd, D, net._skip())
    assert got.shape == exp.shape
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (bad.size, bad[:8])


def _run_embedded(net, x, M, rows):
    """nerfail_mlp_fwd_embedded_x3 over the first M rows of x into a NaN-filled [rows, 4] buffer."""
    from nerfail_amd import _lib
    lib = _lib.load()
    raw = torch.full((rows, 4), float('nan'), dtype=torch.float32, device=dev())
    _lib.check(lib.nerfail_mlp_fwd_embedded_x3(_lib.dev(net.packed()), _lib.dev(net.packed_x3()), 8, 256, net._skip(),
                                               _lib.dev(x), M, _lib.dev(raw), _lib.stream()))
    torch.cuda.synchronize()
    return N(raw)


def _embedded(rs, M):
    from nerfail_amd.run_nerf_helpers import get_embedder
    pts = torch.from_numpy(rs.uniform(-3, 3, size=(M, 3)).astype(np.float32))
    vd = rs.normal(size=(M, 3)).astype(np.float32)
    vd = torch.from_numpy(vd / np.linalg.norm(vd, axis=1, keepdims=True))
    ep, _ = get_embedder(10, 0)
    ed, _ = get_embedder(4, 0)
    return T(N(torch.cat([ep(pts), ed(vd)], -1).float().contiguous()))


@pytest.mark.parametrize('last', [1, 15, 16, 17, 31])
def test_x3_ragged_last_tile_stores_only_its_rows(last):
    """Last tile with `last` valid samples (up to 16: its second half has none): the stored rows equal those of a run
    over whole tiles, and nothing past M is written."""
    _, net = _net(8, [4], seed=51)
    rs = np.random.RandomState(last)
    full = 32 * 37
    x = _embedded(rs, full)
    M = 32 * 36 + last
    ref = _run_embedded(net, x, full, full)
    got = _run_embedded(net, x, M, full)
    assert np.isfinite(ref).all()
    assert np.array_equal(got[:M].view(np.int32), ref[:M].view(np.int32))
    assert np.isnan(got[M:]).all()


def test_x3_multi_round_grid_is_run_to_run_identical():
    _, net = _net(8, [4], seed=53)
    rs = np.random.RandomState(4)
    M = 2 * 1024 * 32 + 1000                          # more than two rounds of a 256-CU persistent grid, ragged end
    x = _embedded(rs, M)
    a = _run_embedded(net, x, M, M + 32)
    b = _run_embedded(net, x, M, M + 32)
    assert np.isfinite(a[:M]).all() and np.isnan(a[M:]).all()
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
