"""-m gpu: nerfail_uap2d_step (norms through the pass mask, the choice, the apply) and nerfail_uap2d_accumulate against
tests/uap2d_ref.py, the numpy restatement written from the header.

norms2: against the float64 restatement within (T + 3) * 2^-24 relative, T = NERFAIL_UAP2D_NORM_TERMS: the sum is of
non-negative terms; each term costs a rounded subtract (two roundings' worth on its square), a rounded multiply, and the lane adds
T of them in float32 (T - 1 roundings) before the double stages, whose own error is far below one float32 ulp; the last
rounding is the double sum's conversion to float32. Choice, scale, trace, rot and r_out: bit for bit against the restatement fed
the kernel's own norms2. nerfail_uap2d_accumulate: bit for bit. Shapes: the smallest at which a path changes - fewer pixels than
a quad, a quad +- 1, one norm workgroup's pixels +- 1, two workgroups + 5 - with every table and mask alignment."""
import itertools

import numpy as np
import pytest
import torch

import nerfail_ref as NR
import uap2d_ref as UR
from hiputil import N, T, dev

pytestmark = pytest.mark.gpu

GROUP = UR.NORM_PIXELS                       # pixels of one norm workgroup
SHAPES = (1, 3, 4, 5, 7, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 5)
TABLE_OFFSETS = ((0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 2), (3, 0, 1), (2, 3, 0), (1, 2, 3))   # r0, rot, r_out: floats
PAD = 8                                       # guard floats / bytes on either side of every view
SENTINEL = np.float32(-12345.5)
NORM_TOL = (UR.NORM_TERMS + 3) * 2. ** -24


def bits_equal(a, b):
    """Equal bit patterns; two NaNs count as equal whatever their payload."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def record(fabs, cls=None, targeted=0, n_comp=None):
    fabs = np.asarray(fabs, np.float32)
    rec = dict(done=0, argmax=0, n_comp=len(fabs) if n_comp is None else n_comp, targeted=targeted,
               cls=np.full(8, -1, np.int32), fabs=np.zeros(8, np.float32))
    rec['fabs'][:len(fabs)] = fabs
    rec['cls'][:len(fabs)] = np.arange(1, len(fabs) + 1) if cls is None else cls
    return rec


def in_buffer(a, off, fill):
    """`a` flattened at element `off` + PAD of a larger device buffer filled with `fill`. Returns (buffer, first element)."""
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = np.full(flat.size + 2 * PAD + 4, fill, flat.dtype)
    buf[PAD + off:PAD + off + flat.size] = flat
    return T(buf), PAD + off


def run_step(G, mask, rec, overshoot, r0, rot, offs=(0, 0, 0), mask_off=0):
    """One nerfail_uap2d_step with the three tables `offs` floats and the mask `mask_off` bytes into larger buffers (whose
    guard elements must come back untouched). Returns (norms2, best, scale, trace, rot', r_out) as numpy."""
    from nerfail_amd import _lib
    lib = _lib.load()
    n_rhs, P = G.shape[0], mask.size
    Gd = T(np.ascontiguousarray(G, np.float32))
    (b0, s0), (b1, s1), (bm, sm) = in_buffer(r0, offs[0], SENTINEL), in_buffer(rot, offs[1], SENTINEL), in_buffer(mask, mask_off, 7)
    b2, s2 = in_buffer(np.full((P, 3), SENTINEL, np.float32), offs[2], SENTINEL)
    recd = T(NR.record_words(rec))
    nb = lib.nerfail_uap2d_step_scratch_bytes(n_rhs, P)
    scratch = torch.zeros((nb // 8,), dtype=torch.float64, device=dev())
    trace = torch.full((1,), -7, dtype=torch.int32, device=dev())
    ptr = lambda t, first: _lib.c_p(t.data_ptr() + first * t.element_size())  # noqa: E731
    _lib.check(lib.nerfail_uap2d_step(_lib.dev(Gd), n_rhs, P, ptr(bm, sm), _lib.dev(recd), _lib.c_p(scratch.data_ptr()), nb, float(overshoot),
                                      ptr(b0, s0), ptr(b1, s1), ptr(b2, s2), _lib.dev(trace), _lib.stream()))
    torch.cuda.synchronize()
    tail = N(scratch).view(np.uint8)[nb - 64:]
    norms2, best, scale = tail[:32].view(np.float32)[:n_rhs - 1].copy(), int(tail[32:36].view(np.int32)[0]), tail[36:40].view(np.float32)[0]
    h0, h1, h2 = N(b0), N(b1), N(b2)
    assert bits_equal(h0[s0:s0 + 3 * P], np.asarray(r0, np.float32).reshape(-1))                 # r0 is read only
    for h, s in ((h0, s0), (h1, s1), (h2, s2)):
        assert (h[:s] == SENTINEL).all() and (h[s + 3 * P:] == SENTINEL).all(), 'a table was written outside its view'
    return norms2, best, scale, int(trace[0]), h1[s1:s1 + 3 * P].reshape(P, 3), h2[s2:s2 + 3 * P].reshape(P, 3)


def check_step(G, mask, rec, overshoot, r0, rot, **where):
    """Runs the step and holds it to the restatement. Returns the kernel's outputs."""
    got = run_step(G, mask, rec, overshoot, r0, rot, **where)
    norms2, best, scale, trace, rot1, out = got
    ref64 = UR.norms2(G, mask)
    with np.errstate(invalid='ignore'):
        ok = np.where(np.isnan(ref64), np.isnan(norms2), np.abs(norms2.astype(np.float64) - ref64) <= NORM_TOL * ref64)
    assert ok.all(), ('norms2', norms2, ref64, np.abs(norms2 - ref64) / ref64 / NORM_TOL)
    _, wbest, wscale, wtrace, wrot, wout = UR.step(G, mask, rec, overshoot, r0, rot, norms2_f32=norms2)
    assert (best, trace) == (wbest, wtrace), (best, trace, wbest, wtrace)
    assert bits_equal(scale, wscale), (scale, wscale)
    assert bits_equal(rot1, wrot) and bits_equal(out, wout)
    return got


def scene(P, n_rhs, seed, spread=1.):
    """Gradients [n_rhs,3,P] of different sizes per class, a mixed mask, tables."""
    rs = np.random.RandomState(seed)
    G = (rs.standard_normal((n_rhs, 3, P)) * (1e-3 * (1 + np.arange(n_rhs)).reshape(-1, 1, 1)) * spread).astype(np.float32)
    mask = rs.randint(0, 8, size=P).astype(np.uint8)
    r0 = rs.uniform(-8, 8, size=(P, 3)).astype(np.float32)
    rot = rs.uniform(-30, 30, size=(P, 3)).astype(np.float32)
    fabs = rs.uniform(50, 120, size=n_rhs - 1).astype(np.float32)
    return G, mask, r0, rot, fabs


@pytest.mark.parametrize('P', SHAPES)
def test_mixed_mask_bits_at_every_alignment(P):
    for n_rhs in (2, 3, 8):
        G, mask, r0, rot, fabs = scene(P, n_rhs, 100 * P + n_rhs)
        for (k, offs), mask_off in itertools.product(enumerate(TABLE_OFFSETS), range(4)):
            if k >= 4 and mask_off != k - 4:                                # mixed table offsets: one mask offset each
                continue
            _, best, scale, trace, rot1, _ = check_step(G, mask, record(fabs), 0.02, r0, rot, offs=offs, mask_off=mask_off)
            assert 1 <= best < n_rhs and trace == best and scale > 0
            assert not UR.mask_bits(mask).any() or not np.array_equal(rot1, rot)


@pytest.mark.parametrize('P', (5, GROUP + 1))
def test_targeted_record_takes_competitor_zero(P):
    G, mask, r0, rot, fabs = scene(P, 2, 7)
    _, best, _, trace, _, _ = check_step(G, mask, record(fabs[:1], cls=[6], targeted=1), 1.0, r0, rot, offs=(1, 1, 1), mask_off=3)
    assert (best, trace) == (1, 6)


@pytest.mark.parametrize('P', (7, 2 * GROUP + 5))
def test_all_bits_cleared(P):
    G, _, r0, rot, fabs = scene(P, 3, 11)
    G[1, 0, 0] = np.nan                                                    # (a NaN under a cleared bit as well)
    norms2, best, scale, trace, rot1, out = check_step(G, np.zeros(P, np.uint8), record(fabs), 0.5, r0, rot, offs=(2, 2, 2))
    assert (norms2 == 0).all() and bits_equal(rot1, rot)
    assert best == 1 + int(np.argmin(fabs)) and scale > 0                  # value_r = |f'| / 1e-4 is finite: a class IS chosen
    assert bits_equal(out, np.clip((r0 + (np.float32(0.5) * rot).astype(np.float32)).astype(np.float32), -255, 255))


@pytest.mark.parametrize('P', (5, GROUP - 1))
def test_nan_under_a_cleared_bit_contributes_nothing(P):
    G, mask, r0, rot, fabs = scene(P, 3, 13)
    clean = check_step(G, mask, record(fabs), 0.02, r0, rot)
    p = P // 2
    mask[p] = 0b101
    base = check_step(G, mask, record(fabs), 0.02, r0, rot)
    G2 = G.copy()
    G2[:, 1, p] = (np.nan, np.inf, -np.inf)                                # channel 1 of pixel p: its bit is cleared
    got = check_step(G2, mask, record(fabs), 0.02, r0, rot)
    assert bits_equal(got[0], base[0]) and got[1:4] == base[1:4] and bits_equal(got[4], base[4]) and bits_equal(got[5], base[5])
    assert np.isfinite(got[4]).all() and np.isfinite(clean[0]).all()


@pytest.mark.parametrize('P', (4, GROUP + 1))
def test_nan_under_a_set_bit_is_never_chosen(P):
    n_rhs = 4
    G, mask, r0, rot, fabs = scene(P, n_rhs, 17)
    mask[P - 1] = 0b111
    fabs[:] = (60, 1, 70)                                                  # competitor 1 would win by far
    G[2, 2, P - 1] = np.nan
    norms2, best, _, trace, rot1, _ = check_step(G, mask, record(fabs, cls=[0, 2, 5]), 0.02, r0, rot, offs=(3, 0, 1), mask_off=1)
    assert np.isnan(norms2[1]) and not np.isnan(norms2[[0, 2]]).any()
    assert best != 2 and trace in (0, 5) and np.isfinite(rot1).all()


@pytest.mark.parametrize('P', (3, GROUP))
def test_every_competitor_nan(P):
    G, mask, r0, rot, fabs = scene(P, 3, 19)
    mask[0] = 0b111
    G[1:, 0, 0] = np.nan
    norms2, best, scale, trace, rot1, out = check_step(G, mask, record(fabs), 0.25, r0, rot, offs=(1, 2, 3), mask_off=2)
    assert np.isnan(norms2).all() and trace == -1 and scale == 0
    assert bits_equal(rot1, rot)                                           # nothing chosen: rot is left alone ...
    assert bits_equal(out, (r0 + (np.float32(0.25) * rot).astype(np.float32)).astype(np.float32))   # ... and r_out still written


@pytest.mark.parametrize('P', (5, GROUP + 1))
def test_two_identical_competitors_the_first_wins(P):
    G, mask, r0, rot, fabs = scene(P, 4, 23)
    G[3] = G[2]
    fabs[:] = (90, 3, 3)
    _, best, _, trace, _, _ = check_step(G, mask, record(fabs, cls=[1, 4, 6]), 0.02, r0, rot)
    assert (best, trace) == (2, 4)


@pytest.mark.parametrize('P', (7, GROUP + 1))
def test_a_record_of_another_shape_moves_nothing(P):
    G, mask, r0, rot, fabs = scene(P, 3, 29)
    rec = record(np.r_[fabs, 5., 5.], n_comp=4)                            # n_comp 4 with n_rhs - 1 = 2
    _, best, scale, trace, rot1, out = check_step(G, mask, rec, 0.02, r0, rot, offs=(0, 1, 2))
    assert scale == 0 and trace == -1 and bits_equal(rot1, rot)
    assert bits_equal(out, (r0 + (np.float32(0.02) * rot).astype(np.float32)).astype(np.float32))


@pytest.mark.parametrize('P', (5, 2 * GROUP + 5))
def test_the_255_clamp_is_reached(P):
    G, mask, r0, rot, fabs = scene(P, 3, 31)
    mask[:] = 0b111
    r0 = (r0 * 30).astype(np.float32)
    mask[0], r0[0], rot[0] = 0, (250., -250., 0.), (100., -100., 0.)        # pixel 0 does not move: 280 -> 255, -280 -> -255, 0
    _, _, _, _, _, out = check_step(G, mask, record(fabs), 0.3, r0, rot, offs=(2, 3, 0), mask_off=1)
    assert tuple(out[0]) == (255., -255., 0.) and np.abs(out).max() == 255


def test_two_runs_give_equal_bits():
    P, n_rhs = 2 * GROUP + 5, 8
    G, mask, r0, rot, fabs = scene(P, n_rhs, 37)
    a = run_step(G, mask, record(fabs), 0.02, r0, rot, offs=(1, 1, 1), mask_off=1)
    b = run_step(G, mask, record(fabs), 0.02, r0, rot, offs=(1, 1, 1), mask_off=1)
    assert bits_equal(a[0], b[0]) and a[1] == b[1] and bits_equal(a[2], b[2]) and a[3] == b[3]
    assert bits_equal(a[4], b[4]) and bits_equal(a[5], b[5])


def test_norms_bound_holds_for_terms_of_very_different_size():
    """Gradients spanning six decades: the float32 part of the sum is the lane's NERFAIL_UAP2D_NORM_TERMS terms, whatever P."""
    P = 2 * GROUP + 5
    rs = np.random.RandomState(41)
    G = (rs.standard_normal((3, 3, P)) * 10. ** rs.uniform(-6, 0, size=(1, 1, P))).astype(np.float32)
    mask = np.full(P, 0b111, np.uint8)
    r0, rot = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32)
    check_step(G, mask, record([80., 90.]), 0.02, r0, rot)


# ------------------------------------------------------------------------------------------------ nerfail_uap2d_accumulate
def run_accumulate(table, r_final, epsilon, offs):
    from nerfail_amd import _lib
    lib = _lib.load()
    n = table.size
    (bt, st), (br, sr) = in_buffer(table, offs[0], SENTINEL), in_buffer(r_final, offs[1], SENTINEL)
    _lib.check(lib.nerfail_uap2d_accumulate(_lib.c_p(bt.data_ptr() + 4 * st), _lib.c_p(br.data_ptr() + 4 * sr), float(epsilon), n,
                                            _lib.stream()))
    torch.cuda.synchronize()
    ht, hr = N(bt), N(br)
    assert (ht[:st] == SENTINEL).all() and (ht[st + n:] == SENTINEL).all(), 'the table was written outside its view'
    assert bits_equal(hr[sr:sr + n], r_final.reshape(-1))
    return ht[st:st + n]


@pytest.mark.parametrize('n', (1, 3, 4, 5, 4099))
@pytest.mark.parametrize('epsilon', (0., 8.))
def test_accumulate_bit_for_bit(n, epsilon):
    rs = np.random.RandomState(n)
    for ot, orf in itertools.product(range(4), range(4)):
        table = rs.uniform(-8, 8, size=n).astype(np.float32)
        r_final = (table + rs.uniform(-12, 12, size=n)).astype(np.float32)
        k = rs.randint(0, n, size=4)
        table[k[0]], r_final[k[0]] = 0., epsilon                           # lands exactly on +epsilon ...
        if n > 1:
            table[k[1]], r_final[k[1]] = 0., -epsilon                       # ... and on -epsilon
        if n > 3:
            table[k[2]] = np.nan                                           # torch.clamp: a NaN stays
            r_final[k[3]] = np.nan
        got = run_accumulate(table, r_final, epsilon, (ot, orf))
        want = UR.accumulate(table, r_final, epsilon)
        assert bits_equal(got, want), (n, epsilon, ot, orf)
        assert np.nanmax(np.abs(got)) <= epsilon
        assert np.array_equal(np.isnan(got), np.isnan(table) | np.isnan(r_final))
        if n > 3:
            assert np.isnan(got).any()


def test_accumulate_twice_equal_bits():
    rs = np.random.RandomState(5)
    table, r_final = rs.uniform(-8, 8, size=4099).astype(np.float32), rs.uniform(-20, 20, size=4099).astype(np.float32)
    assert bits_equal(run_accumulate(table, r_final, 8., (1, 2)), run_accumulate(table, r_final, 8., (1, 2)))
