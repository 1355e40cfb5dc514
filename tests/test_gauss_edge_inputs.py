"""The boundary inputs of tests/gauss_edge_inputs.py really reach every class of per-pixel decision - counted on the oracle
alone (no GPU): the kernel tests in test_hip_gauss_edges.py compare against the oracle on these inputs, so what the inputs
cover is what those tests cover."""
import numpy as np
import pytest

import gauss_edge_inputs as E
from oracle import gauss as OG

F32 = np.float32


@pytest.mark.parametrize('float_only_alpha', [False, True])
def test_exact_map_gathers_the_row_itself(float_only_alpha):
    t = E.table_inputs(float_only_alpha)
    for eps in (E.EPS, None):
        x, x_rgba, _ = OG.gauss_forward(t['s'], t['wi'], t['ori'], eps)
        assert np.array_equal(x.reshape(-1, 4), t['s'][t['row']])            # x == s[row] exactly (-0.0 == 0.0: the sum starts at +0)
        assert np.array_equal(x, t['x'])
    assert sorted(set(t['slot'].tolist())) == list(range(8))                 # the live slot takes every position
    assert len(set(t['row'].tolist())) == t['row'].size                      # a row of its own
    if not float_only_alpha:
        assert np.array_equal(t['ori_u8'].astype(F32), t['ori'])


@pytest.mark.parametrize('eps', [E.EPS, None])
def test_every_decision_class_occurs_in_every_channel(eps):
    t = E.table_inputs()
    cls = E.classify(t['x'], t['ori'], eps)
    alpha, mask, g = OG.pixel_decisions(t['x'], t['ori'], None, np.ones_like(t['x']), eps)
    # the classifier and the oracle agree on what passes
    assert np.array_equal(E.passes(cls), (mask[..., None] >> np.arange(3)) & 1 == 1)
    want = [c for c in E.CLASSES if eps is not None or 'eps' not in c]
    for c in range(3):
        for name in want:
            n = int((cls[..., c] == E.CLASSES.index(name)).sum())
            assert n >= 2, (name, c, n)
    # ... and with alpha = 1, 0.5 and -1 each (delta is ON the bound through a product, not only through x_c itself)
    for x3 in (255.0, 127.5, -255.0):
        sel = t['x'][..., 3] == F32(x3)
        for name in want:
            assert int((cls[sel] == E.CLASSES.index(name)).sum()) >= 2, (name, x3)
    # the float-only ori alphas: -3 blocks, 300 passes
    tf = E.table_inputs(True)
    _, mf, _ = OG.pixel_decisions(tf['x'], tf['ori'], None, np.ones_like(tf['x']), eps)
    assert (mf[tf['ori'][..., 3] < 0] == 0).all() and (mf[tf['ori'][..., 3] > 255] != 0).any()
    # alpha: zero, negative zero, negative and denormal all occur, and the denormal one is not flushed by the oracle
    a = alpha[t['x'][..., 3] == F32(1e-40)]
    assert (a > 0).all() and (a < np.finfo(F32).tiny).all()


def test_backward_through_the_exact_map_is_the_pixel_gradient():
    t = E.table_inputs()
    for eps in (E.EPS, None):
        _, _, g = OG.pixel_decisions(t['x'], t['ori'], t['grad_x'], t['grad_x_rgba'], eps)
        gs = OG.gauss_backward(t['s'], t['wi'], t['ori'], t['grad_x'], t['grad_x_rgba'], eps)
        assert np.array_equal(gs[t['row']], g.reshape(-1, 4))
        spare = np.setdiff1d(np.arange(gs.shape[0]), t['row'])
        assert spare.size > 0 and (gs[spare] == 0).all()


@pytest.mark.parametrize('kind,B', [('mixed', 3), ('positive', 3), ('negative', 3), ('small', 3), ('large', 3), ('mixed', 17)])
def test_bookkeeping_extrema_are_attained_at_a_known_pixel(kind, B):
    k = E.bookkeeping_inputs(kind, B)
    x, _, (emax, emin) = OG.gauss_forward(k['s'], k['wi'], k['ori'], None)
    assert (emax, emin) == (k['emax'], k['emin'])
    alpha = x[..., 3:4] / F32(255)
    e = (np.where(alpha > 0, x[..., :3], F32(0)) * alpha).reshape(-1, 3)
    if kind != 'negative':
        assert np.flatnonzero((e == F32(emax)).any(1)).tolist() == [k['at_max']]
    if kind != 'positive':
        assert np.flatnonzero((e == F32(emin)).any(1)).tolist() == [k['at_min']]
    assert (np.abs(x[..., :3]) > 1e5).any()                                   # huge values behind alpha <= 0 that must not count
    if B == 17:                                                               # the extrema lie in different launches of 16 views
        P = k['shape'][1] * k['shape'][2]
        assert k['at_max'] // P < 16 <= k['at_min'] // P


def test_sign_step_rows_reach_every_bound():
    s, g, s0 = E.sign_step_rows()
    for targeted in (False, True):
        out = OG.igsm_step(s, g, s0, E.A, E.SIGN_EPS, targeted)
        opaque = s[:, 3] > 0
        moved = out[opaque, :3] - s[opaque, :3]
        tiny = (np.abs(g[opaque]) > 0) & (np.abs(g[opaque]) < 1e-35)
        assert tiny.any() and (np.abs(moved[tiny]) > 0).any()                 # a denormal gradient steps
        assert (moved[(g[opaque] == 0) & (np.abs(s[opaque, :3]) < 10)] == 0).all()      # sign(+-0) = 0: no step
        assert ((out[:, :3] == F32(32)).sum() >= 2) and ((out[:, :3] == F32(-32)).sum() >= 2)
        inside = E._na(32, 0)
        assert (out[:, :3] == inside).any() and (out[:, :3] == -inside).any()
        assert (out[~opaque, :3] == 0).all() and np.array_equal(out[:, 3], s[:, 3])


def test_index_rule():
    Ns = 100
    fi = E.probe_indices(Ns)
    assert E.expected_row(fi, Ns).tolist() == [0, 0, 0, 0, 99, 99, 99, 99, 99, 99, 99, 0, 0]
    big = 2 ** 24 + 4
    assert float(F32(big - 1)) > big - 1 and E.expected_row([F32(big)], big).tolist() == [big - 1]
