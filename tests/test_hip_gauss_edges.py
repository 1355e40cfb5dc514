"""-m gpu: the Gauss map's per-pixel DECISIONS at their boundaries (tests/gauss_edge_inputs.py; what those inputs reach is
counted on the oracle in tests/test_gauss_edge_inputs.py).

The clip / where / clip chain of GN:85-119 and its backward is written out in finish_pixel (which also leaves the 3-bit pass
mask), gauss_bwd_kernel, gauss_pixel_grad_kernel, gauss_pixel_grad_multi_kernel and - through the mask -
gauss_pixel_grad_rgb_kernel; the sign step AS:352-392 in igsm_step_kernel, igsm_step_rgb_kernel and gauss_rows_sum3_kernel<true>;
the float -> row conversion in the forward, the atomic backward and the inverted index. On the exact map (one slot of weight 1
per pixel, a row of its own) x == s[row] and grad_s[row] == the pixel's gradient, so every copy is compared with the oracle
WITHOUT a tolerance: an inclusive comparison turned strict, a lost `ori alpha > 0` gate or flushed denormals change a value
from g to 0 (or a step from a to 0), never a last bit.

What "equal" means below: forward outputs (x, x_rgba, alpha, mask), the sign step's result and the epsilon bookkeeping are
compared bit for bit. Gradients are compared as IEEE values (np.array_equal): every non-zero value has identical bits; the
sign of a ZERO is not compared - a blocked channel's 0 * alpha is -0 in a copy that stores the product (alpha < 0) and +0 in
one that adds it to a zero accumulator, and the sign step treats both alike (tested in D).
"""
import ctypes

import numpy as np
import pytest
import torch

import gauss_edge_inputs as E
from conftest import rel_err
from hiputil import T, N, dev
from oracle import gauss as OG

pytestmark = pytest.mark.gpu

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def assert_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(bits(got) != bits(ref))
    assert bad.size == 0, '%s: %d of %d elements differ, first at %s: got %r, reference %r' % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])


def assert_values(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    assert bad.size == 0, '%s: %d of %d elements differ, first at %s: got %r, reference %r' % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])


def _clear():
    from nerfail_amd import GaussNet as G
    G._VIEW_CACHE.clear(); G._BATCH_KEYS.clear(); G._CSR_CACHE.clear()


@pytest.fixture(scope='module')
def table():
    """The table of cases and its oracle results, computed once; nothing below writes into it."""
    t = E.table_inputs()
    t['G3'] = np.random.RandomState(11).normal(size=(3,) + t['shape'] + (4,)).astype(F32)    # three right-hand sides
    for eps in (E.EPS, None):
        x, xr, _ = OG.gauss_forward(t['s'], t['wi'], t['ori'], eps)
        alpha, mask, _ = OG.pixel_decisions(x, t['ori'], None, np.zeros_like(x), eps)
        t[eps] = dict(x=x, x_rgba=xr, alpha=alpha, mask=mask,
                      gs_full=OG.gauss_backward(t['s'], t['wi'], t['ori'], t['grad_x'], t['grad_x_rgba'], eps),
                      gs_rgba=[OG.gauss_backward(t['s'], t['wi'], t['ori'], np.zeros_like(x), t['G3'][c], eps) for c in range(3)])
    return t


# ------------------------------------------------------------------------------------------------ A. forward
@pytest.mark.parametrize('eps', [E.EPS, None])
def test_forward_at_the_boundaries(table, eps):
    """finish_pixel on every class of decision: x, x_rgba, alpha and the pass mask equal the oracle bit for bit, from the float
    image, from its uint8 form (same bits) and through gauss_gather; the float form also with ori alphas -3 and 300."""
    from nerfail_amd import GaussNet as G
    t, ref = table, table[eps]
    s, wi = T(t['s']), T(t['wi'])
    outs = {}
    for form, ori in (('float', T(t['ori'])), ('u8', torch.from_numpy(t['ori_u8'].copy()).to(dev()))):
        views = G.resolve_views(s, wi, ori)
        assert views.ori_u8 == (form == 'u8')
        x, xr, (aa, am) = G.hot_forward(s, views, eps, None, need_x=True, need_aux=True)
        outs[form] = [N(x), N(xr), N(aa), N(am)]
        assert_bits(N(x), ref['x'], 'x ' + form)
        assert_bits(N(xr), ref['x_rgba'], 'x_rgba ' + form)
        assert_bits(N(aa), ref['alpha'], 'aux_alpha ' + form)
        assert np.array_equal(N(am), ref['mask']), ('aux_mask ' + form, np.argwhere(N(am) != ref['mask'])[:4])
    for a, b in zip(outs['float'], outs['u8']):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    x, xr = G.gauss_gather(s, wi, T(t['ori']), eps)
    assert_bits(N(x), ref['x'], 'gauss_gather x')
    assert_bits(N(xr), ref['x_rgba'], 'gauss_gather x_rgba')
    # ori alphas that only a float image holds: -3 (transparent: rgb 0, alpha clipped to 0), 300 (opaque, alpha clipped to 255)
    tf = E.table_inputs(True)
    rx, rxr, _ = OG.gauss_forward(tf['s'], tf['wi'], tf['ori'], eps)
    ra, rm, _ = OG.pixel_decisions(rx, tf['ori'], None, np.zeros_like(rx), eps)
    sf = T(tf['s'])
    views = G.resolve_views(sf, T(tf['wi']), T(tf['ori']))
    x, xr, (aa, am) = G.hot_forward(sf, views, eps, None, need_x=True, need_aux=True)
    assert_bits(N(x), rx, 'x, float-only alphas')
    assert_bits(N(xr), rxr, 'x_rgba, float-only alphas')
    assert_bits(N(aa), ra, 'aux_alpha, float-only alphas')
    assert np.array_equal(N(am), rm)
    assert set(np.unique(rxr[..., 3]).tolist()) == {0.0, 255.0}


# ------------------------------------------------------------------------------------------------ B. epsilon bookkeeping
def _bookkeep(k, mm, eps=None, batch_call=False):
    from nerfail_amd import GaussNet as G, _lib
    s, wi, ori = T(k['s']), T(k['wi']), T(k['ori'])
    if not batch_call:
        G.gauss_gather(s, wi, ori, eps, mm)
        return
    B, H, W = k['shape']
    x = torch.full((B, H, W, 4), float('nan'), device=dev())
    xr = torch.full((B, H, W, 4), float('nan'), device=dev())
    _lib.check(_lib.load().nerfail_gauss_fwd(_lib.dev(s), s.shape[0], _lib.dev(wi), _lib.dev(ori), B, H * W, -1.0 if eps is None else eps,
                                             _lib.dev(x), _lib.dev(xr), _lib.dev(mm), _lib.stream()))
    assert not bool(torch.isnan(x).any()) and not bool(torch.isnan(xr).any())


@pytest.mark.parametrize('batch_call', [False, True])
@pytest.mark.parametrize('kind,B', [('mixed', 3), ('positive', 3), ('negative', 3), ('mixed', 17)])
def test_epsilon_bookkeeping_is_exact(kind, B, batch_call):
    """The running [min, max] of where(alpha > 0, x_rgb, 0) * alpha (GN:89-103; wave reduction, stale-read filter, sign-aware
    integer atomics) from [0, 0]: EXACTLY [min(0, oracle min), max(0, oracle max)] - min and max round nothing. All-positive
    deltas leave the minimum at 0, all-negative ones the maximum; B = 17 folds two launches into the same pair (the maximum
    lies in the first launch's views, the minimum in the second's). Values behind alpha <= 0 (+-1e6) must not count. The
    epsilon clip comes after the bookkeeping: the same values with epsilon = 32."""
    k = E.bookkeeping_inputs(kind, B)
    _, _, (emax, emin) = OG.gauss_forward(k['s'], k['wi'], k['ori'], None)
    want = np.array([min(0.0, emin), max(0.0, emax)], F32)
    assert want.tolist() == [k['emin'], k['emax']]
    for eps in (None, E.EPS):
        mm = torch.zeros(2, device=dev())
        _bookkeep(k, mm, eps, batch_call)
        assert_bits(N(mm), want, 'eps_minmax %s B=%d eps=%r' % (kind, B, eps))


def test_epsilon_bookkeeping_only_moves_outwards():
    """From [-5, 7]: inputs whose extrema (-3.25, 3.5) lie inside leave both values as they are; a second call with larger
    extrema (-57.5, 61.25) moves both outwards; a third call with the small inputs changes nothing again."""
    small, large = E.bookkeeping_inputs('small', 3), E.bookkeeping_inputs('large', 3, seed=4)
    assert -5 < small['emin'] < 0 < small['emax'] < 7 and large['emin'] < -5 and large['emax'] > 7
    mm = T(np.array([-5.0, 7.0], F32))
    _bookkeep(small, mm)
    assert_bits(N(mm), np.array([-5.0, 7.0], F32), 'inside the running range')
    _bookkeep(large, mm)
    assert_bits(N(mm), np.array([large['emin'], large['emax']], F32), 'outwards')
    _bookkeep(small, mm)
    assert_bits(N(mm), np.array([large['emin'], large['emax']], F32), 'unchanged again')


# ------------------------------------------------------------------------------------------------ C. every backward copy
@pytest.mark.parametrize('eps', [E.EPS, None])
def test_every_backward_copy_at_the_boundaries(table, eps):
    """Each row of the exact map receives ONE contribution with weight 1, so every backward path returns its kernel copy's
    per-pixel gradient itself: compared with OG.gauss_backward (float32 decisions, float64 accumulation) for EQUALITY.
    The alpha column (ga / 255: three products summed in float32 in the order c = 0, 1, 2, then one division) needed no
    allowance: all four columns are equal."""
    from nerfail_amd import GaussNet as G, _lib
    t, ref = table, table[eps]
    lib = _lib.load()
    B, H, W = t['shape']
    P, Ns = H * W, t['s'].shape[0]
    keps = -1.0 if eps is None else eps
    s_np, wi, ori = t['s'], T(t['wi']), T(t['ori'])
    Gx, Gr, G3 = T(t['grad_x']), T(t['grad_x_rgba']), T(t['G3'])
    _clear()
    full, rgba = {}, {}                                      # copy -> gradient [Ns,4] with (grad_x, grad_x_rgba) / with G3[0] alone

    # autograd through gauss_gather: gauss_pixel_grad_kernel + per-view indices (deterministic), gauss_bwd_kernel (atomics)
    for det in (True, False):
        st = T(s_np).requires_grad_(True)
        x, xr = G.gauss_gather(st, wi, ori, eps, None, det)
        ((x * Gx).sum() + (xr * Gr).sum()).backward()
        full['gather det=%s' % det] = N(st.grad)
        st = T(s_np).requires_grad_(True)
        x, xr = G.gauss_gather(st, wi, ori, eps, None, det)
        (xr * G3[0]).sum().backward()
        rgba['gather det=%s' % det] = N(st.grad)
    xs = x.detach().contiguous()
    assert_bits(N(xs), ref['x'], 'x')

    # gauss_pixel_grad_kernel over the batch index, with and without grad_x
    csr = G.csr_for(wi, Ns)
    sc1 = torch.empty((lib.nerfail_gauss_bwd_scratch_floats(B, P, 1),), device=dev())
    for name, gx, gr, store in (('csr', Gx, Gr, full), ('csr', None, G3[0].contiguous(), rgba)):
        out = torch.full((Ns, 4), float('nan'), device=dev())
        _lib.check(lib.nerfail_gauss_bwd_csr(_lib.dev(ori), _lib.dev(xs), _lib.dev(gx), _lib.dev(gr), _lib.dev(csr.row_ptr),
                                             _lib.dev(csr.contrib), _lib.dev(csr.w_sorted), _lib.dev(csr.row_of), Ns, B, P, keps,
                                             _lib.dev(sc1), 0, _lib.dev(out), _lib.stream()))
        store[name] = N(out)

    # gauss_pixel_grad_multi_kernel, 3 right-hand sides: over the batch index ...
    J = G3.reshape(3, B * P, 4).contiguous()
    out3 = torch.full((3, Ns, 4), float('nan'), device=dev())
    sc3 = torch.empty((lib.nerfail_gauss_bwd_scratch_floats(B, P, 3),), device=dev())
    _lib.check(lib.nerfail_gauss_bwd_csr_multi(_lib.dev(ori), _lib.dev(xs), _lib.dev(J), 3, _lib.dev(csr.row_ptr), _lib.dev(csr.contrib),
                                               _lib.dev(csr.w_sorted), _lib.dev(csr.row_of), Ns, B, P, keps, _lib.dev(sc3),
                                               _lib.dev(out3), _lib.stream()))
    multi = N(out3)
    # ... and view by view over the per-view indices (a row belongs to one pixel, so the views' tables add up exactly)
    vis = G.view_indices(wi, Ns)
    view_multi = np.zeros((3, Ns, 4), F32)
    for b in range(B):
        stt = _lib.ViewIndexStruct()
        vis[b].fill(stt)
        Jb = G3[:, b].reshape(3, P, 4).contiguous()
        ob, xb = ori[b].contiguous(), xs[b].contiguous()
        outb = torch.full((3, Ns, 4), float('nan'), device=dev())
        scb = torch.empty((lib.nerfail_gauss_bwd_views_scratch_floats(ctypes.byref(stt), 1, P, 3),), device=dev())
        _lib.check(lib.nerfail_gauss_bwd_view_multi(_lib.dev(ob), _lib.dev(xb), _lib.dev(Jb), 3, ctypes.byref(stt), Ns, P, keps,
                                                    _lib.dev(scb), _lib.dev(outb), _lib.stream()))
        assert vis[b].n_entries == P and vis[b].n_rows == P
        view_multi += N(outb)
    rgba['csr_multi'], rgba['view_multi'] = multi[0], view_multi[0]

    # gauss_pixel_grad_rgb_kernel: alpha + the forward's pass mask instead of x and ori
    views = G.resolve_views(T(s_np), wi, ori)
    _, _, aux = G.hot_forward(T(s_np), views, eps, None, need_x=False, need_aux=True)
    rgb = N(G.hot_backward_rgb(aux, G3[0].contiguous(), views)).reshape(Ns, 3)

    for name, g in full.items():
        assert_values(g.reshape(Ns, 4), ref['gs_full'], name + ' (grad_x and grad_x_rgba)')
    for name, g in rgba.items():
        assert_values(g.reshape(Ns, 4), ref['gs_rgba'][0], name + ' (grad_x_rgba)')
    for c in range(3):
        assert_values(multi[c], ref['gs_rgba'][c], 'csr_multi rhs %d' % c)
        assert_values(view_multi[c], ref['gs_rgba'][c], 'view_multi rhs %d' % c)
    assert_values(rgb, ref['gs_rgba'][0][:, :3], 'hot_backward_rgb')
    # the copies among each other: the rgb columns, value for value
    first = next(iter(rgba.values())).reshape(Ns, 4)
    for name, g in rgba.items():
        assert_values(g.reshape(Ns, 4)[:, :3], first[:, :3], name)
    assert_values(rgb, first[:, :3], 'hot_backward_rgb vs the x / ori copies')
    # the comparison is not vacuous: passing and blocked channels both occur among the opaque pixels, with a gradient to block
    passed = (ref['mask'][..., None] >> np.arange(3)) & 1
    assert passed.sum() > 100 and (1 - passed)[t['ori'][..., 3] > 0].sum() > 100
    _clear()


def test_backward_with_float_only_ori_alpha():
    """ori alpha -3 (blocks) and 300 (passes) through the copies that read the float image."""
    from nerfail_amd import GaussNet as G
    tf = E.table_inputs(True)
    _clear()
    for eps in (E.EPS, None):
        ref = OG.gauss_backward(tf['s'], tf['wi'], tf['ori'], tf['grad_x'], tf['grad_x_rgba'], eps)
        for det in (True, False):
            st = T(tf['s']).requires_grad_(True)
            x, xr = G.gauss_gather(st, T(tf['wi']), T(tf['ori']), eps, None, det)
            ((x * T(tf['grad_x'])).sum() + (xr * T(tf['grad_x_rgba'])).sum()).backward()
            assert_values(N(st.grad), ref, 'det=%s eps=%r' % (det, eps))
    _clear()


# ------------------------------------------------------------------------------------------------ D. sign step
@pytest.mark.parametrize('targeted', [False, True])
def test_sign_step_kernels_at_the_boundaries(targeted):
    """igsm_step_kernel and igsm_step_rgb_kernel: gradients +-0, denormal (torch.sign is +-1 there: they must step), tiny and
    ordinary; row alpha 255, 0 and -1; s +- a exactly on s_init +- epsilon, one float step inside and beyond. Equal to
    OG.igsm_step bit for bit. On a NaN gradient the reference would write NaN (sign(NaN) = NaN) while the kernels' comparisons
    are both false and leave the value where it is: those entries are NOT compared with the oracle - what is pinned is that
    the copies agree with each other there, bit for bit."""
    from nerfail_amd import attack as A
    s, g, s0 = E.sign_step_rows(with_nan=True)
    g4 = np.concatenate([g, np.random.RandomState(2).normal(size=(len(g), 1)).astype(F32)], 1)
    ref = OG.igsm_step(s, g4, s0, E.A, E.SIGN_EPS, targeted)
    a = N(A.igsm_step(T(s), T(g4), T(s0), E.A, E.SIGN_EPS, targeted))
    b = N(A.igsm_step_rgb(T(s), T(g), T(s0), E.A, E.SIGN_EPS, targeted))
    assert_bits(a, b, 'igsm_step vs igsm_step_rgb')
    ok = np.concatenate([~np.isnan(g), np.ones((len(g), 1), bool)], 1)
    assert (~ok).sum() == 6 and not np.isnan(a).any()
    assert_bits(np.where(ok, a, 0), np.where(ok, ref, 0), 'igsm_step vs the oracle')
    # the denormal gradients stepped (on the kernel's output, not only on the oracle's)
    tiny = (np.abs(g) > 0) & (np.abs(g) < 1e-35) & (s[:, 3:4] > 0) & (np.abs(s[:, :3]) < 10)
    assert tiny.sum() >= 6 and (np.abs(a[:, :3] - s[:, :3])[tiny] == F32(E.A)).all()


@pytest.mark.parametrize('targeted', [False, True])
def test_fused_sign_step_at_the_boundaries(targeted):
    """gauss_rows_sum3_kernel<true>: the same rows as the perturbation table of an exact map with ONE view, so that the summed
    gradient of a row is its pixel's value (alpha = 1 rows: the upstream gradient itself, denormals included). Equal to the
    oracle's backward + sign step bit for bit, and to both separate kernels on the gradient the fused call wrote out (also on
    the NaN gradients, which are not compared with the oracle)."""
    from nerfail_amd import GaussNet as G, attack as A
    rows, g, _ = E.sign_step_rows(with_nan=True)
    n = len(rows)
    shape = (1, 9, n // 9)
    assert 9 * (n // 9) == n
    s, wi, row, _ = E.exact_map(rows, shape, seed=3)
    Ns = s.shape[0]
    s_init = np.zeros_like(s)
    s_init[:, 3] = s[:, 3]
    ori = np.empty(shape + (4,), F32)
    ori[..., :3], ori[..., 3] = 128.0, 255.0                 # every channel passes: pre = 128 + s_c * alpha lies inside
    Gr = np.zeros(shape + (4,), F32)
    Gr.reshape(-1, 4)[:, :3] = g
    Gr[..., 3] = 1.0
    # (the oracle multiplies a NaN gradient by the seven zero weights too and scatters 0 * NaN = NaN into those rows; the
    # kernels leave zero-weight entries out. NaN entries are not the oracle's to judge: it gets 0 there, NaN put back after)
    g_or = OG.gauss_backward(s, wi, ori, np.zeros_like(Gr), np.nan_to_num(Gr, nan=0.0), None)
    g_or[row[:, None], np.arange(3)[None, :]] = np.where(np.isnan(g), F32(np.nan), g_or[row, :3])
    opaque_row = rows[:, 3] == 255.0
    assert_values(g_or[row][opaque_row][:, :3], g[opaque_row], 'oracle')              # the table's gradients arrive as they are
    ok = np.concatenate([~np.isnan(g_or[:, :3]), np.ones((Ns, 1), bool)], 1)
    ref = OG.igsm_step(s, g_or, s_init, E.A, E.SIGN_EPS, targeted)
    _clear()
    st, s0t = T(s), T(s_init)
    views = G.resolve_views(st, T(wi), T(ori))
    _, _, aux = G.hot_forward(st, views, None, None, need_x=False, need_aux=True)
    gout = torch.full((3 * Ns,), 7.0, device=dev())
    fused = N(G.hot_backward_rgb_step(aux, T(Gr), views, st, s0t, E.A, E.SIGN_EPS, targeted, grad_out=gout))
    assert_values(N(gout).reshape(Ns, 3), g_or[:, :3], 'the gradient the fused step saw')
    assert not np.isnan(fused).any() and (~ok).sum() >= 2
    assert_bits(np.where(ok, fused, 0), np.where(ok, ref, 0), 'fused step vs the oracle')
    assert_bits(N(A.igsm_step_rgb(st, gout, s0t, E.A, E.SIGN_EPS, targeted)), fused, 'igsm_step_rgb vs fused')
    g4 = torch.cat([gout.view(Ns, 3), torch.zeros((Ns, 1), device=dev())], 1).contiguous()
    assert_bits(N(A.igsm_step(st, g4, s0t, E.A, E.SIGN_EPS, targeted)), fused, 'igsm_step vs fused')
    assert_bits(N(G.hot_backward_rgb_step(aux, T(Gr), views, st, s0t, E.A, E.SIGN_EPS, targeted)), fused, 'fused, no grad_out')
    _clear()


# ------------------------------------------------------------------------------------------------ E. index conversion
def _probe_map(Ns, probes, seed=5):
    """One pixel per probed index in the live slot (weight 1; the dead slots carry probed indices too, with weight 0)."""
    rs = np.random.RandomState(seed)
    n = len(probes)
    idx = np.stack([np.roll(probes, k + 1) for k in range(8)], 1).astype(F32)      # dead slots: other probes
    w = np.zeros((n, 8), F32)
    slot = np.arange(n) % 8
    w[np.arange(n), slot] = 1.0
    idx[np.arange(n), slot] = probes
    wi = np.stack([w.reshape(1, 1, n, 8), idx.reshape(1, 1, n, 8)], 1)
    gx = rs.randint(1, 64, (1, 1, n, 4)).astype(F32)              # small integers: their sums are exact in any order
    return wi, gx


def test_index_conversion_follows_one_rule_everywhere():
    """A float index resolves to the row `clamp as a float to [0, Ns-1] (NaN -> 0), then truncate` (index_row, common.h) in the
    forward's gather, in the atomic backward's scatter and in the inverted index: -1, -0.5, -0.0, 0.5, Ns-1, Ns-0.5, Ns, Ns+0.5,
    3e9, 1e20, +-inf and NaN. (Before the shared helper the two backward copies converted through int64 FIRST and clamped
    afterwards - an out-of-range conversion: a pixel with index 1e20 gathered from the last row in the forward while both
    backward forms added its gradient to row 0. This test and the next one failed on those kernels.) Every copy clamps before
    its first memory access, so no probe leaves the table."""
    from nerfail_amd import GaussNet as G
    Ns = 61
    probes = E.probe_indices(Ns)
    want = E.expected_row(probes, Ns)
    assert want.tolist() == [0, 0, 0, 0, Ns - 1, Ns - 1, Ns - 1, Ns - 1, Ns - 1, Ns - 1, Ns - 1, 0, 0]
    wi, gx = _probe_map(Ns, probes)
    rs = np.random.RandomState(6)
    s = rs.uniform(-40, 40, (Ns, 4)).astype(F32)
    ori = np.zeros((1, 1, len(probes), 4), F32)
    _clear()
    grads = {}
    for det in (True, False):
        st = T(s).requires_grad_(True)
        x, _ = G.gauss_gather(st, T(wi), T(ori), None, None, det)
        assert_values(N(x).reshape(-1, 4), s[want], 'forward rows')
        (x * T(gx)).sum().backward()
        grads[det] = N(st.grad)
    ref = np.zeros((Ns, 4), F32)
    np.add.at(ref, want, gx.reshape(-1, 4))
    assert_values(grads[False], ref, 'atomic backward rows')
    assert_values(grads[True], ref, 'inverted-index backward rows')
    assert G.view_indices(T(wi), Ns)[0].n_rows == 2
    _clear()


def test_index_conversion_where_float_of_the_last_row_rounds_up():
    """Ns = 2^24 + 4: float32(Ns - 1) rounds UP to Ns, so the float clamp alone lets the index float(Ns) through and the integer
    clamp behind it has to hold. Zero table on the device, only the probed rows set, five pixels."""
    from nerfail_amd import GaussNet as G
    Ns = 2 ** 24 + 4
    assert float(F32(Ns - 1)) > Ns - 1 and float(F32(Ns)) == Ns
    probes = np.array([Ns, Ns - 2, 0, 2 ** 24, 1e20], F32)
    want = np.array([Ns - 1, Ns - 2, 0, 2 ** 24, Ns - 1])
    assert E.expected_row(probes, Ns).tolist() == want.tolist()
    wi, gx = _probe_map(Ns, probes)
    ori = np.zeros((1, 1, len(probes), 4), F32)
    rows = sorted(set(want.tolist()))
    vals = np.random.RandomState(8).uniform(1, 40, (len(rows), 4)).astype(F32)
    s = torch.zeros((Ns, 4), device=dev())
    s[torch.tensor(rows, device=dev())] = T(vals)
    expect_x = vals[[rows.index(r) for r in want.tolist()]]
    ref = np.zeros((len(rows), 4), F32)
    np.add.at(ref, [rows.index(r) for r in want.tolist()], gx.reshape(-1, 4))
    _clear()
    for det in (True, False):
        st = s.clone().requires_grad_(True)
        x, _ = G.gauss_gather(st, T(wi), T(ori), None, None, det)
        assert_values(N(x).reshape(-1, 4), expect_x, 'forward rows')
        (x * T(gx)).sum().backward()
        hit = torch.nonzero(st.grad.abs().sum(1)).flatten()
        assert hit.cpu().tolist() == rows, det
        assert_values(N(st.grad[hit]), ref, 'backward rows det=%s' % det)
        del st, x
    _clear()


# ------------------------------------------------------------------------------------------------ F. launch geometry
@pytest.mark.parametrize('B', [1, 3, 16, 17, 33])
@pytest.mark.parametrize('H,W', [(5, 7), (16, 17)])
def test_forward_launch_geometry(H, W, B):
    """gauss_fwd_views_kernel's launch: kFwdViews = 16 views per launch (B = 16 | 17 | 33: one full launch, a second one with a
    single view, a third), the grid padded to a multiple of 8 workgroups (`v >= nv` guard) and the XCD remap of the virtual
    block, with P = 35 (one workgroup per view) and 272 (two, the second nearly empty). Through nerfail_gauss_fwd on the batch
    tensor and through nerfail_gauss_fwd_views / gauss_gather on per-view tensors; every output pre-filled with NaN: no
    pixel may be left unwritten, and none written twice with another view's data."""
    from nerfail_amd import GaussNet as G, _lib
    lib = _lib.load()
    rs = np.random.RandomState(100 * B + H)
    P = H * W
    Ns = 3 * P
    s = rs.uniform(-40, 40, (Ns, 4)).astype(F32)
    s[:, 3] = rs.choice(np.array([255.0, 127.5, 0.0], F32), Ns)
    dist = np.sort(np.abs(rs.normal(scale=0.02, size=(B, H, W, 8))).astype(F32), -1)
    idx = rs.randint(0, Ns, (B, H, W, 8)).astype(F32)
    wi_np, _ = OG.create_gauss_w(np.stack([dist, idx], 1))
    ori = np.zeros((B, H, W, 4), F32)
    ori[..., :3] = rs.randint(0, 256, (B, H, W, 3))
    ori[..., 3] = rs.choice(np.array([0.0, 255.0], F32), (B, H, W), p=[0.3, 0.7])
    Gx, Gr = rs.normal(size=(B, H, W, 4)).astype(F32), rs.normal(size=(B, H, W, 4)).astype(F32)
    rx, rxr, _ = OG.gauss_forward(s, wi_np, ori, E.EPS)
    rg = OG.gauss_backward(s, wi_np, ori, Gx, Gr, E.EPS)
    st, wi, orit = T(s), T(wi_np), T(ori)

    def nan(*shape, dtype=torch.float32):
        return torch.full(shape, float('nan'), dtype=dtype, device=dev())
    x, xr = nan(B, H, W, 4), nan(B, H, W, 4)
    _lib.check(lib.nerfail_gauss_fwd(_lib.dev(st), Ns, _lib.dev(wi), _lib.dev(orit), B, P, E.EPS, _lib.dev(x), _lib.dev(xr), None, _lib.stream()))
    assert rel_err(N(x), rx) < 1e-5 and rel_err(N(xr), rxr) < 1e-5          # (rel_err also refuses a NaN the reference has not)
    # per-view tensors: every view its own allocation
    wl, ol = [wi[b].clone() for b in range(B)], [orit[b].clone() for b in range(B)]
    views = G.resolve_views(st, wl, ol)
    x2, xr2, aa = nan(B, H, W, 4), nan(B, H, W, 4), nan(B, H, W)
    am = torch.full((B, H, W), 255, dtype=torch.uint8, device=dev())
    _lib.check(lib.nerfail_gauss_fwd_views(_lib.dev(st), Ns, views.table(), B, P, 0, E.EPS, _lib.dev(x2), _lib.dev(xr2), _lib.dev(aa),
                                           _lib.dev(am), None, _lib.stream()))
    assert torch.equal(x2, x) and torch.equal(xr2, xr)
    assert not bool(torch.isnan(aa).any()) and int(am.max()) <= 7
    _clear()
    sg = T(s).requires_grad_(True)
    x3, xr3 = G.gauss_gather(sg, wl, ol, E.EPS)
    assert torch.equal(x3, x) and torch.equal(xr3, xr)
    ((x3 * T(Gx)).sum() + (xr3 * T(Gr)).sum()).backward()
    assert np.abs(N(sg.grad) - rg).max() <= 2e-5 * np.abs(rg).max()
    _clear()


# ------------------------------------------------------------------------------------------------ G. Gaussian weights
def test_gaussian_weights_normal_denormal_and_underflowed():
    """K9 with c = 0.02 at d / c = 0, 1, 13 (normal Gaussians), 13.5, 14, 14.3 (denormal: exp(-91) .. exp(-102)), 14.6, 20, inf
    (underflowed to 0) - away from the flush threshold near 14.42 -, in mixed rows, all-underflowed rows (GN:181: weights 0)
    and all-denormal rows (sum g > 0: the weights are g / 0.001, not 0). The zero pattern equals the oracle's exactly, the
    values to 1e-5 of the maximum. A denormal weight is a weight: the forward's "any weight non-zero" test and the inverted
    index's "weight == 0" drop must both keep it (n_entries; forward / backward adjointness on the all-denormal pixels)."""
    from nerfail_amd import GaussNet as G
    rs = np.random.RandomState(9)
    c = 0.02
    ratios = np.array([0, 1, 13.0, 13.5, 14.0, 14.3, 14.6, 20, np.inf], np.float64)
    H, W = 6, 8
    Ns = 3 * H * W
    r = np.empty((1, H, W, 8))
    r[0, :2] = rs.choice(ratios, (2, W, 8))                                   # mixed
    r[0, 0, 0] = ratios[:8]
    r[0, 2:4] = rs.choice(ratios[6:], (2, W, 8))                              # all underflowed
    r[0, 4:] = rs.choice(ratios[3:6], (2, W, 8))                              # all denormal
    dist = (r * c).astype(F32)
    idx = rs.randint(0, Ns, (1, H, W, 8)).astype(F32)
    dai = np.stack([dist, idx], 1)
    ref, _ = OG.create_gauss_w(dai, c)
    wi, _ = G.create_gauss_w(dev(), c)(T(dai))
    w, rw = N(wi)[:, 0], ref[:, 0]
    assert np.array_equal(w == 0, rw == 0)
    assert rel_err(w, rw) < 1e-5 and np.array_equal(N(wi)[:, 1], idx)
    tiny = np.finfo(F32).tiny
    assert (rw[0, 2:4] == 0).all() and (rw[0, 4:] > 0).all() and (rw[0, 4:] < tiny * 1e4).all()
    assert ((rw[0, :2] > 0) & (rw[0, :2] < tiny)).any() and (rw[0, :2] > 0.01).any()
    # the denormal Gaussians themselves (before the division by 0.001) and the weights of the 14.3 slots are not flushed
    assert (w[0, 4:][r[0, 4:] == 14.3] > 0).all() and (w[0, 4:][r[0, 4:] == 14.3] < tiny).all()
    _clear()
    vi = G.ViewIndex(wi[0], Ns)
    assert vi.n_entries == int(np.count_nonzero(rw)) and vi.n_entries > 16 * 8
    # adjointness on the all-denormal pixels alone: <G, J s> == <J^T G, s> with G, s > 0 of magnitude 1e30 (so that w * s and
    # w * G are ordinary numbers and no term cancels). Each side is a sum of positive products: one rounding per product and
    # per addition, at most 8 additions per pixel in the forward and 128 (every entry in one row) in the backward - a relative
    # error below 130 * 2^-24 = 7.8e-6 each. A dropped pixel or entry would leave one side short by a whole term (>= 1/128).
    s2 = (rs.uniform(0.5, 1.0, (Ns, 4)) * 1e30).astype(F32)
    Gm = np.zeros((1, H, W, 4), F32)
    Gm[0, 4:] = (rs.uniform(0.5, 1.0, (2, W, 4)) * 1e30).astype(F32)
    ori = np.zeros((1, H, W, 4), F32)
    for det in (True, False):
        st = T(s2).requires_grad_(True)
        x, _ = G.gauss_gather(st, wi, T(ori), None, None, det)
        assert (N(x)[0, 4:] > 0).all() and (N(x)[0, 2:4] == 0).all()
        (x * T(Gm)).sum().backward()
        lhs = float((N(x).astype(np.float64) * Gm).sum())
        rhs = float((N(st.grad).astype(np.float64) * s2).sum())
        assert lhs > 0 and abs(lhs - rhs) <= 2 * 130 * 2.0 ** -24 * lhs, (det, lhs, rhs)
    _clear()
