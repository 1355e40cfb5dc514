"""-m gpu: the attack-evaluation kernels (csrc/eval_metrics.hip), ops and nerfail_amd.model_test against the numpy restatement
tests/eval_ref.py and fixture g25 (the reference's test_for_inception). Shapes are the smallest that reach every path: one
pixel, U8C3 views whose byte count is and is not a multiple of 4 (the last pixels then take byte loads), one and two workgroups
per view (128 at g25's 800 x 800), more views than one launch's table carries."""
import numpy as np
import pytest
import torch

import cnn_inputs as CI
import eval_ref as R
import synth
from hiputil import T, N, dev, hip_nerf

pytestmark = pytest.mark.gpu

IMAGE_FORMATS = (R.U8C4, R.U8C3, R.F32C4)


def _ops():
    from nerfail_amd import ops  # noqa: F401
    return torch.ops.nerfail_mi


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def embed(arr):
    """The array on the device INSIDE a larger buffer whose other bytes are 0xFF (255 as uint8, a NaN as float32): a read
    beyond the view changes a maximum or a sum. 16 bytes in front keep every format's alignment."""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = torch.full((16 + raw.size + 64,), 255, dtype=torch.uint8, device=dev())
    buf[16:16 + raw.size] = torch.from_numpy(raw.copy()).to(dev())
    return buf[16:16 + raw.size].view(torch.from_numpy(np.zeros(0, arr.dtype)).dtype).reshape(arr.shape)


def as_format(img8, fmt):
    """uint8 [P,4] -> the same image on white in `fmt` (numpy)."""
    if fmt == R.U8C4:
        return img8
    if fmt == R.F32C4:
        return img8.astype(np.float32)
    if fmt == R.U8C3:
        return R.white(img8, R.U8C4).astype(np.uint8)
    return R.white(img8, R.U8C4).reshape(-1)


def rgba8(rs, B, P):
    x = rs.randint(0, 256, size=(B, P, 4)).astype(np.uint8)
    x[..., 3] = np.where(rs.uniform(size=(B, P)) < 0.3, 0, x[..., 3])
    return x


def run_rows(a_list, fa, o_list, fo, cla=False):
    rows, c = _ops().eval_view_metrics([embed(a) for a in a_list], fa, [embed(o) for o in o_list], fo, cla)
    return N(rows), N(c)


@pytest.mark.parametrize('B,P', [(1, 1), (3, 1), (1, 1023), (3, 1023), (1, 1024), (1, 33 * 33), (17, 5)])
def test_view_metrics_uint8_values_every_format_pair(B, P):
    rs = np.random.RandomState(B * 10000 + P)
    a8, o8 = rgba8(rs, B, P), rgba8(rs, B, P)
    o8[0, : (P + 1) // 2] = a8[0, : (P + 1) // 2]                                     # zeros among the differences
    want = R.view_rows(a8, R.U8C4, o8, R.U8C4)
    want_cla = np.stack([R.cla_in(a, R.U8C4) for a in a8])
    assert (want[:, 5] == 3 * P).all() and (want[:, 2:5] < 2.0 ** 53).all()
    for fa in IMAGE_FORMATS:
        for fo in IMAGE_FORMATS:
            rows, cla = run_rows([as_format(a, fa) for a in a8], fa, [as_format(o, fo) for o in o8], fo, True)
            assert rows.tobytes() == want.tobytes(), (fa, fo, rows, want)                # sums of integers: bitwise, every format
            assert cla.shape == (B, 3, P) and cla.tobytes() == want_cla.tobytes(), (fa, fo)
    flat, _ = run_rows([as_format(a, R.FLAT) for a in a8], R.FLAT, [as_format(o, R.FLAT) for o in o8], R.FLAT)
    assert flat.tobytes() == want.tobytes()
    again, _ = run_rows([as_format(a, R.FLAT) for a in a8], R.FLAT, [as_format(o, R.FLAT) for o in o8], R.FLAT)
    assert again.tobytes() == flat.tobytes()
    if P % 4:                                                                            # FLAT with n no multiple of 12 either
        n = 3 * P - 1
        f, _ = run_rows([as_format(a, R.FLAT)[:n] for a in a8], R.FLAT, [as_format(o, R.FLAT)[:n] for o in o8], R.FLAT)
        assert f.tobytes() == R.view_rows([as_format(a, R.FLAT)[:n] for a in a8], R.FLAT, [as_format(o, R.FLAT)[:n] for o in o8], R.FLAT).tobytes()


@pytest.mark.parametrize('B,P', [(1, 1), (3, 1023), (1, 33 * 33), (17, 5)])
def test_view_metrics_unrounded_floats(B, P):
    rs = np.random.RandomState(B * 777 + P)
    a = rs.uniform(-20, 280, size=(B, P, 4)).astype(np.float32)
    a[..., 3] = np.where(rs.uniform(size=(B, P)) < 0.3, -1., 255.)
    o8 = rgba8(rs, B, P)
    for fo, o in ((R.U8C4, o8), (R.F32C4, o8.astype(np.float32) + rs.uniform(0, 1, size=o8.shape).astype(np.float32))):
        want = R.view_rows(a, R.F32C4, o, fo)
        rows, cla = run_rows(list(a), R.F32C4, list(o), fo, True)
        rows2, _ = run_rows(list(a), R.F32C4, list(o), fo, False)
        assert rows.tobytes() == rows2.tobytes()                                         # two runs: the same bits
        assert np.array_equal(rows[:, [0, 1, 4, 5]], want[:, [0, 1, 4, 5]])              # max, min, count, n: exact
        for v in range(B):
            for k in (2, 3):                                                             # a float64 sum in another order
                assert _rel(rows[v, k], want[v, k]) <= 1e-13, (v, k, rows[v, k], want[v, k])
        assert cla.tobytes() == np.stack([R.cla_in(x, R.F32C4) for x in a]).tobytes()
    fa, fo_ = R.white(a[0], R.F32C4).reshape(-1), R.white(o8[0], R.U8C4).reshape(-1) + np.float32(0.25)
    rows, _ = run_rows([fa], R.FLAT, [fo_], R.FLAT)
    want = R.view_rows([fa], R.FLAT, [fo_], R.FLAT)
    assert np.array_equal(rows[:, [0, 1, 4, 5]], want[:, [0, 1, 4, 5]]) and _rel(rows[0, 2], want[0, 2]) <= 1e-13 and _rel(rows[0, 3], want[0, 3]) <= 1e-13


def test_view_metrics_slices_and_separate_allocations_and_batch_independence():
    rs = np.random.RandomState(5)
    B, P = 5, 1023
    a8, o8 = rgba8(rs, B, P), rgba8(rs, B, P)
    for fmt in (R.U8C4, R.F32C4):
        a, o = np.stack([as_format(x, fmt) for x in a8]), np.stack([as_format(x, fmt) for x in o8])
        stacked = _ops().eval_view_metrics(list(T(a).unbind(0)), fmt, list(T(o).unbind(0)), fmt, False)[0]
        separate = _ops().eval_view_metrics([T(x) for x in a], fmt, [T(x) for x in o], fmt, False)[0]
        alone = torch.cat([_ops().eval_view_metrics([T(a[v])], fmt, [T(o[v])], fmt, False)[0] for v in range(B)])
        assert N(stacked).tobytes() == N(separate).tobytes() == N(alone).tobytes() == R.view_rows(a8, R.U8C4, o8, R.U8C4).tobytes()


def test_nan_rules():
    rs = np.random.RandomState(9)
    B, P = 3, 300
    a = rgba8(rs, B, P).astype(np.float32)
    o = rgba8(rs, B, P).astype(np.float32)
    a[..., 3] = np.maximum(a[..., 3], 1.)
    clean = R.view_rows(a, R.F32C4, o, R.F32C4)
    a[1, 77, 2] = np.nan                                                                 # one NaN element in view 1
    rows, _ = run_rows(list(a), R.F32C4, list(o), R.F32C4)
    assert np.isnan(rows[1, :4]).all() and rows[1, 4] == R.view_row(a[1], R.F32C4, o[1], R.F32C4)[4] and rows[1, 5] == 3 * P
    assert rows[[0, 2]].tobytes() == clean[[0, 2]].tobytes()                             # the others untouched
    a[1, 77, 2] = 5.
    a[1, 78, 3] = np.nan                                                                 # a NaN alpha: white
    rows, cla = run_rows(list(a), R.F32C4, list(o), R.F32C4, True)
    assert rows.tobytes() == R.view_rows(a, R.F32C4, o, R.F32C4).tobytes() and not np.isnan(rows).any()
    assert (cla[1, :, 78] == 255).all() and not np.isnan(cla).any()


def test_logit_stats():
    z = np.array([[1., 7., 7., 0.], [7., 7., 1., 0.], [np.nan, 9., 0., 0.], [0., 9., np.nan, 0.], [2., 9., 1., 0.]], np.float32)
    pred, ce = _ops().eval_logit_stats(T(z), 2)
    assert N(pred).dtype == np.int32 and N(pred).tolist() == [1, 0, -1, -1, 1]            # the first maximum; NaN rows: -1
    wp, wc = R.logit_stats(z, 2)
    assert np.isnan(N(ce)[2:4]).all() and all(_rel(N(ce)[i], wc[i]) <= 1e-12 for i in (0, 1, 4))
    rs = np.random.RandomState(7)                                                        # more views than lanes
    for C, label in ((8, 3), (32, 31), (1, 0)):
        lg = (rs.normal(size=(130, C)) * 10).astype(np.float32)
        pred, ce = _ops().eval_logit_stats(T(lg), label)
        wp, wc = R.logit_stats(lg, label)
        assert N(pred).tolist() == wp.tolist()
        assert all(_rel(g, w) <= 1e-12 or abs(g - w) <= 1e-15 for g, w in zip(N(ce), wc))


def test_fold_two_batches():
    rs = np.random.RandomState(11)
    C, label, P = 8, 4, 100
    a8, o8 = rgba8(rs, 7, P), rgba8(rs, 7, P)
    a8[2] = o8[2]                                                                        # an identical pair: the PSNR epsilon branch
    lg = rs.normal(size=(7, C)).astype(np.float32)
    lg[5, 0] = np.nan                                                                    # a view without a prediction
    rows = R.view_rows(a8, R.U8C4, o8, R.U8C4)
    wp, wc = R.logit_stats(lg, label)
    rec = torch.zeros(R.RECORD, dtype=torch.float64, device=dev())
    want = np.zeros(R.RECORD)
    for sl in (slice(0, 3), slice(3, 7)):
        r, _ = _ops().eval_view_metrics([T(x) for x in a8[sl]], R.U8C4, [T(x) for x in o8[sl]], R.U8C4, False)
        p, c = _ops().eval_logit_stats(T(lg[sl]), label)
        _ops().eval_fold(r, p, c, C, rec)
        want = R.fold(want, rows[sl], wp[sl], wc[sl], C)
    got = N(rec)
    exact = [0, 1, 2, 5, 7, 10, 11, 12, 13, 14, 15] + list(range(16, R.RECORD))          # counts, e max, e min, d l0, PSNR max
    assert got[exact].tolist() == want[exact].tolist(), (got, want)
    assert got[7] == R.PSNR_IDENTICAL and got[0] == 7 and got[10] == 1 and got[16:].sum() == 6
    assert np.isnan(got[9]) and np.isnan(want[9])                                        # the NaN row's CE
    for k in (3, 4, 6, 8):                                                               # device sqrt / log10 against libm
        assert _rel(got[k], want[k]) <= 1e-12, (k, got[k], want[k])
    first = torch.zeros(R.RECORD, dtype=torch.float64, device=dev())                     # a first call initialises the minima
    r, _ = _ops().eval_view_metrics([T(a8[0])], R.U8C4, [T(o8[0])], R.U8C4, False)
    p, c = _ops().eval_logit_stats(T(lg[:1]), label)
    _ops().eval_fold(r, p, c, C, first)
    assert N(first)[2] == rows[0, 1] and N(first)[6] == N(first)[7] > 0


# ---------------------------------------------------------------------------------------------------------- end to end
def native8(seed):
    from nerfail_amd.MyModel import MyCNN
    m = MyCNN(8)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CI.state_dict(seed, 8).items()}, strict=True)
    return m.to(dev()).requires_grad_(False).eval()


def test_evaluate_views_native_cnn_against_reference(golden):
    from nerfail_amd import model_test as MT
    g = golden('g25_eval')
    originals, attacked = R.g25_pairs(g)
    m = native8(int(g['weight_seed']))
    side = int(g['side'])
    a, o = [T(x) for x in attacked], [T(x) for x in originals]
    _, cla = _ops().eval_view_metrics(a, R.U8C4, o, R.U8C4, True)
    lg = N(m(cla.view(len(a), 3, side, side))).astype(np.float64)
    r32, r64 = g['logits'].astype(np.float64), g['logits_f64']
    bound = 2 * np.linalg.norm(r32 - r64) + 1e-6 * np.linalg.norm(r64)                   # the bound of tests/test_hip_cnn.py against g23
    print('logits |got - f64| %.3e bound %.3e' % (np.linalg.norm(lg - r64), bound))
    assert np.linalg.norm(lg - r64) <= bound
    assert lg.argmax(1).tolist() == g['logits'].argmax(1).tolist()
    msg = MT.evaluate_views(m, 'my_model', a, o, int(g['label']), batch=4, num_classes=int(g['num_classes']))
    R.check_msg(msg, g, 'evaluate_views', logit_slack=bound + float(np.abs(r32 - r64).max()))
    f32 = MT.evaluate_views(m, 'my_model', torch.stack(a).float(), o, int(g['label']), batch=4, num_classes=int(g['num_classes']))
    assert f32 == msg                                                                    # x_rgba-like float input: the same numbers


class StandIn(torch.nn.Module):
    """A stock classifier: 4 x 4 average pool and one linear layer."""

    def __init__(self, C=8, seed=3):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(4), torch.nn.Flatten(), torch.nn.Linear(48, C))
        with torch.no_grad():
            rs = np.random.RandomState(seed)
            self.net[2].weight.copy_(torch.from_numpy(rs.normal(size=(C, 48)).astype(np.float32) / 255.))
            self.net[2].bias.zero_()

    def forward(self, x):
        return self.net(x)


def _msg_close(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, v in want.items():
        if isinstance(v, str) or k in ('e min', 'e max', 'd l0 norm', 'acc'):
            assert got[k] == v, (k, got[k], v)
        else:
            assert _rel(got[k], v) <= 1e-12, (k, got[k], v)


def test_evaluate_views_stock_classifier_after_resize():
    from nerfail_amd import model_test as MT
    from nerfail_amd._resize import resize
    rs = np.random.RandomState(21)
    n, side, size, C, label, batch = 5, 32, 16, 8, 1, 2
    a8, o8 = rgba8(rs, n, side * side).reshape(n, side, side, 4), rgba8(rs, n, side * side).reshape(n, side, side, 4)
    a8[4] = o8[4]
    m = StandIn(C).to(dev()).eval()
    got = MT.evaluate_views(m, 'vgg16', [T(x) for x in a8], T(o8), label, batch=batch, num_classes=C, resize_to=size)
    ar, orr, lg = [], [], []
    with torch.no_grad():
        for b0 in range(0, n, batch):                                                    # torch's own resize of the white images
            ta = resize(T(np.stack([R.cla_in(x, R.U8C4).reshape(3, side, side) for x in a8[b0:b0 + batch]])), size).contiguous()
            to = resize(T(np.stack([R.cla_in(x, R.U8C4).reshape(3, side, side) for x in o8[b0:b0 + batch]])), size).contiguous()
            lg.append(N(m(ta)))
            ar += list(N(ta))
            orr += list(N(to))
    assert ar[0].shape == (3, size, size)
    _, want = R.evaluate(ar, R.FLAT, orr, R.FLAT, np.concatenate(lg), label, C, batch=batch)
    _msg_close(got, want)
    assert got['psnr max'] == R.PSNR_IDENTICAL and got['e min'] == 0


def test_no_host_wait_before_the_record_is_read():
    """evaluate_record (= evaluate_views up to its one read) with host waits forbidden by torch's sync debug mode, where this
    build honours it; and evaluate_views reads exactly one device tensor, the 48-double record."""
    from nerfail_amd import model_test as MT
    rs = np.random.RandomState(33)
    side, C = 32, 8
    a = [T(x) for x in rgba8(rs, 5, side * side).reshape(5, side, side, 4)]
    o = [T(x) for x in rgba8(rs, 5, side * side).reshape(5, side, side, 4)]
    big_a, big_o = [T(x) for x in rgba8(rs, 3, 766 * 766).reshape(3, 766, 766, 4)], [T(x) for x in rgba8(rs, 3, 766 * 766).reshape(3, 766, 766, 4)]
    cases = ((StandIn(C).to(dev()).eval(), 'vgg16', a, o, dict(batch=2, num_classes=C, resize_to=16)),
             (native8(5), 'my_model', big_a, big_o, dict(batch=2, num_classes=C)))
    for m, name, av, ov, kw in cases:
        MT.evaluate_views(m, name, av, ov, 1, **kw)                                      # first pass: weight image, allocations
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            torch.ones(1, device=dev()).item()
            native = False
        except RuntimeError:
            native = True
        print('set_sync_debug_mode("error") catches a host wait on this build:', native)
        records = [MT.evaluate_record(m, name, av, ov, 1, **kw) for m, name, av, ov, kw in cases]
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    reads = []
    orig = {n: getattr(torch.Tensor, n) for n in ('cpu', 'item', 'tolist', 'numpy')}

    def spy(n):
        def f(self, *a_, **k):
            if self.is_cuda:
                reads.append((n, tuple(self.shape)))
            return orig[n](self, *a_, **k)
        return f
    for n in orig:
        setattr(torch.Tensor, n, spy(n))
    try:
        msgs = [MT.evaluate_views(m, name, av, ov, 1, **kw) for m, name, av, ov, kw in cases]
    finally:
        for n, f in orig.items():
            setattr(torch.Tensor, n, f)
    assert reads == [('cpu', (R.RECORD,))] * 2, reads
    for rec, msg in zip(records, msgs):
        assert MT.report(N(rec), 1, C) == msg


def test_evaluate_render_equals_views_of_render_path():
    from nerfail_amd import model_test as MT, run_nerf as RN
    side, C, label = 32, 8, 2
    _, coarse = hip_nerf(4, 64, 31)
    _, fine = hip_nerf(4, 64, 32)
    q = RN.FusedNetworkQuery(RN.get_embedder(10, 0)[0], RN.get_embedder(4, 0)[0])
    kw = dict(network_query_fn=q, perturb=0., N_importance=8, network_fine=fine, N_samples=8, network_fn=coarse, use_viewdirs=True,
              white_bkgd=True, raw_noise_std=0., ndc=False, lindisp=False, near=2., far=6.)
    focal, K = synth.lego_intrinsics(side, side)
    poses = torch.from_numpy(np.stack([synth.pose_spherical(t, -30., 4.) for t in (-117., 10., 95.)]).astype(np.float32))
    rs = np.random.RandomState(2)
    originals = T(rgba8(rs, 3, side * side).reshape(3, side, side, 4))
    m = StandIn(C).to(dev()).eval()
    got = MT.evaluate_render(kw, poses, [side, side, focal], K, 1024, originals, m, 'vgg16', label, num_classes=C, resize_to=16, batch=2)
    rgbs, _ = RN.render_path(poses, [side, side, focal], K, 1024, kw)
    files = [np.ascontiguousarray(RN.to8b(x)[..., ::-1]) for x in rgbs]                  # what render_path writes, as cv2 reads it back
    assert files[0].shape == (side, side, 3) and files[0].dtype == np.uint8
    want = MT.evaluate_views(m, 'vgg16', [T(x) for x in files], originals, label, num_classes=C, resize_to=16, batch=2)
    assert got == want and got['e max'] > 0


def test_eval_ops_pass_opcheck():
    from nerfail_amd import ops as O
    assert set(O.EVAL_OPS) == {'eval_view_metrics', 'eval_logit_stats', 'eval_fold'}
    rs = np.random.RandomState(0)
    a, o = T(rgba8(rs, 2, 9)), T(rgba8(rs, 2, 9).astype(np.float32))
    rows = torch.zeros(2, 6, dtype=torch.float64, device=dev())
    rows[:, 5] = 27.
    samples = {'eval_view_metrics': (list(a.unbind(0)), R.U8C4, list(o.unbind(0)), R.F32C4, True),
               'eval_logit_stats': (T(rs.normal(size=(3, 8)).astype(np.float32)), 2),
               'eval_fold': (rows, torch.zeros(2, dtype=torch.int32, device=dev()), torch.ones(2, dtype=torch.float64, device=dev()), 8,
                             torch.zeros(R.RECORD, dtype=torch.float64, device=dev()))}
    for name in O.EVAL_OPS:
        torch.library.opcheck(getattr(torch.ops.nerfail_mi, name).default, samples[name],
                              test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_dynamic'))
