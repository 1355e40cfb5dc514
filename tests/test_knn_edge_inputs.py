"""The inputs of tests/knn_edge_inputs.py really reach what they are built for - counted on the oracle and on the float32
emulation of the grid build alone (no GPU): the kernel tests in test_hip_knn_edges.py compare against the oracle on these
inputs, so what the inputs cover is what those tests cover. Conditions, not measurements."""
import numpy as np
import pytest

import knn_edge_inputs as E
from oracle import knn as OK

F32 = np.float32
ALL_LADDERS = dict(E.LADDER_FAMILIES, **E.FAR_FAMILIES)


@pytest.fixture(scope='module')
def families():
    """Every ladder family once: name -> (Q, P, info). Nothing below writes into them."""
    out = {}
    for name, make in ALL_LADDERS.items():
        info = {}
        Q, P = make(info=info)
        out[name] = (Q, P, info)
    return out


def test_emulated_build_formulas():
    assert [E.grid_dim_for(n) for n in (8, 63, 100, 4095, 4096, 4166, 5359, 5360, 6000, 6331, 6332, 1920000, 1 << 24)] == \
        [4, 4, 5, 16, 16, 16, 17, 18, 18, 18, 19, 124, 256]
    # float steps: a round trip through the ordered integers, across 0 and across a binade
    v = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -149, -16384.0, 1e-11], F32)
    assert np.array_equal(E.o2f(E.f2o(v)), v)
    assert E.step(F32(1), -1) == np.nextafter(F32(1), F32(0)) and E.step(F32(-16384), -1) == np.nextafter(F32(-16384), F32(-np.inf))
    assert E.step(F32(2.0 ** -149), -2) == -F32(2.0 ** -149)
    # the transition is where cell_coord changes, whatever the drawn face says; both face forms stay within a few steps of
    # |o| + extent of it (the slack a fix of the kernel has to cover): 8 steps of 2.9 * 2^-24 here
    g = E.Grid(E.face_ladders(16)[1])
    assert g.G == 16 and g.Gc == 4 and g.Gs == 1 and E.Grid(E.face_ladders(18)[1]).Gs == 2
    for axis in range(3):
        for k in range(1, g.G):
            T = g.transition(axis, k)
            assert g.raw_coord(T, axis) == k and g.raw_coord(E.step(T, -1), axis) == k - 1
            for fused in (False, True):
                assert abs(float(T) - float(g.face(axis, k, fused))) <= 8 * 2.9 * 2.0 ** -24
    assert E.ladder_offsets((1,)).tolist() == list(range(-48, 49))
    o23 = E.ladder_offsets((2, 3))
    assert o23.min() <= -48 and o23.max() >= 48 and 0 in o23 and set(np.diff(o23).tolist()) == {2, 3}


@pytest.mark.parametrize('name', sorted(ALL_LADDERS))
def test_every_ladder_holds_points_of_both_cells_and_points_the_drawn_box_misplaces(families, name):
    Q, P, info = families[name]
    g = info['grid']
    assert np.array_equal(np.unique(P, axis=0), np.unique(np.concatenate([P, Q]), axis=0))      # every query is a point of the set
    if 'ladders' in info:
        reach = np.abs(info['offsets']).max()
        assert reach >= 48
        for axis, k, first, n in info['ladders']:
            v = Q[first:first + n, axis]
            c = g.coord(v, axis)
            assert {k - 1, k} <= set(c.tolist()), (name, axis, k)
            assert np.array_equal(E.f2o(v) - E.f2o(g.transition(axis, k)), info['offsets'])        # centred on the transition
            other = [b for b in range(3) if b != axis]
            assert (Q[first:first + n][:, other] == Q[first, other]).all()
    else:
        assert {c[2] for c in info['clusters']} == {'lower', 'upper'}
        assert {c[0] for c in info['clusters']} == {0, 1, 2} or len(info['clusters']) >= 4
    # binned cell != the cell whose drawn box contains the point: under BOTH face forms, in every family
    for fused in (False, True):
        wrong = 0
        for axis in range(3):
            wrong += int((g.coord(P[:, axis], axis) != E.box_cell(g, P[:, axis], axis, fused)).sum())
        assert wrong >= 1, (name, fused)


@pytest.mark.parametrize('name', sorted(E.LADDER_FAMILIES))
def test_the_stopping_rule_as_written_loses_neighbours_on_every_ladder_family(families, name):
    """The shell walk's rule `d8 < (0.999 bound)^2`, bound taken from the DRAWN faces, on the binned cells: at least one query of
    every family (under either face form) gets another answer than oracle.knn.knn8 - the inputs can fail. The hand-built
    clusters fail at every cluster: that is their construction. (The sets far from the origin are not in this list: there
    v - o is exact, the transition is the first float at or above the true face, the drawn face is at most one step below
    it, and a point ON the drawn face is exactly `bound` away - the strict rule cannot lose it. They are inputs for the
    kernel's other box expressions and for the bbox atomics.)"""
    Q, P, info = families[name]
    _, exact = OK.knn8(Q, P)
    for fused in (False, True):
        got, stopped = E.emulated_shell_rule(Q, P, fused)
        bad = (got != exact).any(1)
        print('%s, %s faces: %d of %d queries stop in the shells, %d answered wrongly' % (name, 'fused' if fused else 'unfused', stopped.sum(), len(Q), bad.sum()))
        assert bad.sum() >= 1, (name, fused)
        assert not bad[~stopped].any()
        if 'clusters' in info:
            assert bad.all()
        # ... and with the slack the kernel takes off the bound, the same rule answers every query: the slack covers the
        # distance between binning and drawn face at every face of the family
        mended, _ = E.emulated_shell_rule(Q, P, fused, slack=True)
        assert np.array_equal(mended, exact), (name, fused)
    g = info['grid']
    for axis in range(3):
        for k in range(1, g.G):
            for fused in (False, True):
                assert abs(float(g.transition(axis, k)) - float(g.face(axis, k, fused))) < 0.5 * float(E.bin_slack(g))


def test_lattice_ties_cross_cells_and_the_index_decides():
    info = {}
    Q, P = E.tie_lattice(info=info)
    g = info['grid']
    h2 = float(E.LATTICE_H) ** 2
    d2 = OK.d2_f32(Q[:, None, :], P[None, :, :])
    exact64 = ((Q[:, None, :].astype(np.float64) - P[None]) ** 2).sum(-1)
    on_lattice = (P * 8 == np.round(P * 8)).all(1)
    assert on_lattice.sum() == 1000
    assert np.array_equal(d2.astype(np.float64)[:, on_lattice], exact64[:, on_lattice])      # every d2 to a lattice point is exact
    order = np.lexsort((np.broadcast_to(np.arange(len(P)), d2.shape), d2), axis=-1)[:, :9]
    od, oi = OK.knn8(Q, P)
    assert np.array_equal(order[:, :8], oi) and on_lattice[order].all()           # the clump stays out of every answer
    ds = np.take_along_axis(d2, order, -1)
    # the multiplicities the four kinds of query are built for: 1 + 6 (lattice point: itself, then its 6 neighbours), 2, 4, 8
    inner = np.all(Q >= -1 + float(E.LATTICE_H), axis=1)                          # (the queries stay 2 h inside the far hull)
    first = (ds[:, :8] == ds[:, :1]).sum(1)
    second = (ds[:, 1:9] == ds[:, 1:2]).sum(1)                # (after the lattice point itself)
    for kind, want in ((1, 2), (2, 4), (3, 8)):
        assert (first[inner & (info['kind'] == kind)] == want).all() and (inner & (info['kind'] == kind)).sum() >= 10
    assert (second[inner & (info['kind'] == 0)] == 6).all()
    pc, qc = g.cells(P), g.cells(Q)
    tied = ds[:, 7] == ds[:, 8]
    c8, c9 = pc[order[:, 7]], pc[order[:, 8]]
    cross = tied & (c8 != c9).any(1)
    ring8, ring9 = np.abs(c8 - qc).max(1), np.abs(c9 - qc).max(1)
    farther = cross & (ring8 > ring9)                        # the winner (lower index) sits in a later shell than the loser
    print('lattice: %d of %d queries tie 8th / 9th, %d across cells, %d with the lower index in the farther cell' % (tied.sum(), len(Q), cross.sum(), farther.sum()))
    assert cross.sum() >= 32 and farther.sum() >= 8
    assert h2 == 2.0 ** -6


@pytest.mark.parametrize('kind', E.WAVE_KINDS)
def test_wave_compositions_have_the_lanes_they_claim(kind):
    info = {}
    Q, P = E.wave_composition(kind, info=info)
    g, group = info['grid'], info['group']
    assert len(group) == len(Q) == {'last_1': 65, 'last_63': 63}.get(kind, 64)
    qc = g.cells(Q)
    reach = 0.5 * E.K_COHERENT * float(g.cs)                  # the kernel's grouping distance (coordinates, not cells)
    cheb = np.abs(Q[:, None, :].astype(np.float64) - Q[None]).max(-1)
    if kind in ('one_ladder', 'last_1', 'last_63'):
        assert cheb.max() < 1e-6 and set(qc[:, 0].tolist()) == {7, 8} and (qc[:, 1:] == 3).all()
        assert info['searched'] == len(Q)
        return
    sizes = {'g7': [7], 'g8': [8], 'g9': [9], 'g8_late': [8], 'five_groups': [12] * 5}[kind]
    assert [int((group == i).sum()) for i in range(len(sizes))] == sizes and (group == -1).sum() == 64 - sum(sizes)
    assert len(sizes) <= E.K_GROUP_PASSES or kind == 'five_groups'
    for i in range(len(sizes)):
        m = group == i
        assert (qc[m] == qc[m][0]).all()                                         # one emulated cell per group
        assert cheb[m][:, m].max() <= 0.1 * float(g.cs) and cheb[m][:, ~m].min() > reach + float(g.cs) * 0.5
        assert len(np.unique(Q[m], axis=0)) == m.sum()
    s = group == -1
    apart = cheb[s][:, s] + np.eye(s.sum()) * 1e9
    assert apart.min() > reach and (np.abs(qc[s][:, None] - qc[s][None]).max(-1) + np.eye(s.sum(), dtype=int) * 99).min() > 3
    assert (group[0] == 0) == (kind != 'g8_late')                                 # who names the first group
    assert info['searched'] == {'g7': 0, 'g8': 8, 'g9': 9, 'g8_late': 0, 'five_groups': 48}[kind]
    # every lane that walks the shells finishes in them (so the counter is what the grouping alone makes it): exact answer,
    # stopped, under both face forms
    _, exact = OK.knn8(Q, P)
    for fused in (False, True):
        got, stopped = E.emulated_shell_rule(Q, P, fused)
        assert stopped.all() and np.array_equal(got, exact)


def test_tiled_view_cuts_the_ladder():
    info = {}
    Q, P = E.tiled_view(info=info)
    assert Q.shape == (9, 17, 3) and Q.dtype == F32
    on_ladder = (np.arange(9 * 17) < info['n_ladder']).reshape(9, 17)
    tiles = [on_ladder[r:r + 8, c:c + 8] for r in (0, 8) for c in (0, 8, 16)]
    assert [t.size for t in tiles] == [64, 64, 8, 8, 8, 1]
    assert sum(1 for t in tiles if t.any()) >= 3 and sum(1 for t in tiles if t.any() and not t.all()) >= 1
    qc = info['grid'].cells(Q.reshape(-1, 3))[:info['n_ladder'], 0]
    assert set(qc.tolist()) == {7, 8}


@pytest.mark.parametrize('kind', E.DEGENERATE_KINDS)
def test_degenerate_sets(kind):
    Q, P = E.degenerate(kind)
    g = E.Grid(P)
    n_places = len(np.unique(P, axis=0))
    assert n_places == {'same_8': 1, 'same_100': 1, 'two_places': 2, 'eight_points': 8}[kind]
    if n_places == 1:
        assert g.cs == F32(F32(1.0001) / F32(g.G))                                # extent 0 -> 1
    if kind == 'eight_points':
        lo, hi = P.min(0), P.max(0)
        out = np.maximum(lo - Q, Q - hi).max(1) / float(g.cs)
        assert (out > 9.99).sum() == 8 and (out <= 0).sum() >= 30
