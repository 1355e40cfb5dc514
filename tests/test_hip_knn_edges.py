"""-m gpu: the grid 8-NN search at cell faces, exact ties and wave groupings (tests/knn_edge_inputs.py; what those inputs reach
is counted on the oracle and on a float32 emulation of the build in tests/test_knn_edge_inputs.py).

knn_grid.hip promises the bits of the brute-force scan and of oracle/knn.py. The promise rests on pruning: a cell, a coarse
cell, a block or the unvisited rest of the grid is skipped when a lower bound of its distance lies strictly above the current
8th distance, and every bound comes from a box DRAWN at o + x * cs while a point is BINNED by floorf((v - o) * inv_cs). The
inputs here sit where the two disagree (ladders of points one float step apart across the binning transition of a face, near 0
where a float step is a thousandth of the binning's own error, and far from the origin), where keys tie exactly across cells,
and where a wave's grouping decisions fall on their thresholds. Every comparison is for EQUALITY of distances and indices,
every query, against oracle.knn.knn8; `method='brute'` is held to the same.
"""
import numpy as np
import pytest
import torch

import knn_edge_inputs as E
from hiputil import T, N, dev
from oracle import knn as OK

pytestmark = pytest.mark.gpu

_REF = {}


def case(name, make):
    """(Q, P, info, oracle dist, oracle idx) of one input set, computed once per run; nothing writes into it."""
    if name not in _REF:
        info = {}
        Q, P = make(info=info)
        od, oi = OK.knn8(Q.reshape(-1, 3), P)
        _REF[name] = (Q, P, info, od, oi)
    return _REF[name]


def knn(Q, P, method):
    from nerfail_amd.create_index_and_dist import knn8
    d, i = knn8(Q if torch.is_tensor(Q) else T(Q), P if torch.is_tensor(P) else T(P), want_int=True, method=method)
    return N(d).reshape(-1, 8), N(i).reshape(-1, 8)


def assert_same(got, ref, what, info=None, order=None):
    """Distances (as bits) and indices equal for every query; the message counts the queries that differ (per ladder where the
    input has ladders)."""
    (d, i), (od, oi) = got, ref
    assert d.shape == od.shape and i.shape == oi.shape, what
    bad = (i != oi).any(1) | (d.view(np.uint32) != od.view(np.uint32)).any(1)
    if not bad.any():
        return
    msg = '%s: %d of %d queries differ from the oracle' % (what, bad.sum(), len(bad))
    where = np.flatnonzero(bad) if order is None else np.sort(order[np.flatnonzero(bad)])
    if info and 'ladders' in info:
        msg += '; per ladder (axis, face): ' + ', '.join(
            '(%d, %d): %d' % (a, k, ((where >= f) & (where < f + n)).sum()) for a, k, f, n in info['ladders'] if ((where >= f) & (where < f + n)).any())
    n0 = int(np.flatnonzero(bad)[0])
    raise AssertionError('%s; first at query %d: idx %s, oracle %s; dist %s, oracle %s' % (msg, n0, i[n0], oi[n0], d[n0], od[n0]))


# ------------------------------------------------------------------------------------------------ A. faces
LADDERS = dict(E.LADDER_FAMILIES, **E.FAR_FAMILIES)


@pytest.mark.parametrize('name', sorted(LADDERS))
def test_ladders_across_cell_faces(name):
    """Every ladder point as a query, ladder by ladder (64 consecutive queries lie on one ladder: the wave searches them as one
    group, pruning by wave_box_d2 / box_d2 / axis_d / the per-point bound) and in a shuffled order (a wave holds a few lanes of
    every ladder: no group forms, each lane walks the shells and stops by the rule the emulation shows failing when the bound
    is taken from the drawn face), and as 8 x 8 pixel tiles. Before the kernel grew its boxes by kBinSlack it answered 91 / 22 /
    89 of the 1164 queries of ladders_G16 wrongly in the three orders, 105 / 11 / 106 of ladders_G18, 46 / 22 / 51 and 49 / 11 / 49
    of the 492 of the 2/3-step ladders and 10 / 10 and 7 / 5 of the hand-built clusters; the four sets far
    from the origin passed."""
    Q, P, info, od, oi = case(name, LADDERS[name])
    Pt = T(P)
    assert_same(knn(Q, Pt, 'brute'), (od, oi), name + ' brute', info)
    assert_same(knn(Q, Pt, 'grid'), (od, oi), name + ' grid, ladder by ladder', info)
    order = np.random.RandomState(1).permutation(len(Q))
    assert_same(knn(Q[order], Pt, 'grid'), (od[order], oi[order]), name + ' grid, shuffled', info, order)
    if len(Q) >= 64:
        # 8 x 8 pixel tiles over the same queries (the view entry): rows of 20 pixels, the last tile column 4 pixels wide
        H = len(Q) // 20
        Qv = Q[:H * 20].reshape(H, 20, 3)
        assert_same(knn(Qv, Pt, 'grid'), (od[:H * 20], oi[:H * 20]), name + ' grid, view tiles', info)


# ------------------------------------------------------------------------------------------------ B. exact ties
def test_exact_ties_across_cells():
    """Lattice queries whose 8th and 9th keys have EQUAL d2 in different cells (224 of 320 queries; in 35 the winner sits in a
    later shell than the loser): a bound that excludes a box must be strict, and the index alone decides."""
    Q, P, info, od, oi = case('lattice', E.tie_lattice)
    Pt = T(P)
    assert_same(knn(Q, Pt, 'brute'), (od, oi), 'lattice brute')
    assert_same(knn(Q, Pt, 'grid'), (od, oi), 'lattice grid')
    order = np.random.RandomState(2).permutation(len(Q))
    assert_same(knn(Q[order], Pt, 'grid'), (od[order], oi[order]), 'lattice grid, shuffled')


# ------------------------------------------------------------------------------------------------ C. wave compositions
@pytest.mark.parametrize('kind', E.WAVE_KINDS)
def test_wave_compositions_and_work_counter(kind):
    """One launch of the flat entry per composition, with the kernel's work counters on: the result equals the oracle and the
    second counter - valid lanes that took part in a wave search - has the value the grouping rules imply (kMinGroup = 8: a
    group of 7 is not searched as a wave, 8 and 9 are; a scattered lane 0 ends the grouping for the whole wave; kGroupPasses = 4:
    the fifth group walks the shells; a last wave's repeated lanes are not counted). The inputs are built so that every lane
    that walks the shells finishes in shell 0, which test_knn_edge_inputs.py checks on the emulation."""
    from nerfail_amd import _lib
    lib = _lib.load()
    Q, P, info, od, oi = case('wave_' + kind, lambda info=None: E.wave_composition(kind, info=info))
    Pt = T(P)
    knn(Q, Pt, 'grid')                                        # (builds the grid: the counted launch is the search alone)
    stats = torch.zeros((2,), dtype=torch.int64, device=dev())
    try:
        _lib.check(lib.nerfail_knn8_grid_stats(_lib.dev(stats)))
        got = knn(Q, Pt, 'grid')
        torch.cuda.synchronize()
    finally:
        lib.nerfail_knn8_grid_stats(None)
    examined, searched = stats.cpu().tolist()
    assert_same(got, (od, oi), 'wave ' + kind)
    assert_same(knn(Q, Pt, 'brute'), (od, oi), 'wave %s brute' % kind)
    assert searched == info['searched'], (kind, searched, info['searched'])
    assert examined >= 8 * len(Q)                             # every valid query measured at least its 8 neighbours
    stats.zero_()                                             # the pointer is off again: nothing is counted
    knn(Q, Pt, 'grid')
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [0, 0]


def test_view_tiles_cut_a_ladder():
    """9 x 17 pixels through the view entry (8 x 8 tiles, a last row and a last column one pixel wide: repeated lanes), the flat
    entry and brute force."""
    Q, P, info, od, oi = case('view', E.tiled_view)
    assert Q.shape == (9, 17, 3)
    Pt = T(P)
    assert_same(knn(Q, Pt, 'grid'), (od, oi), 'view entry')
    assert_same(knn(Q.reshape(-1, 3), Pt, 'grid'), (od, oi), 'flat entry')
    assert_same(knn(Q, Pt, 'brute'), (od, oi), 'brute')


# ------------------------------------------------------------------------------------------------ D. degenerate sets
@pytest.mark.parametrize('kind', E.DEGENERATE_KINDS)
def test_degenerate_sets(kind):
    Q, P, info, od, oi = case('degenerate_' + kind, lambda info=None: E.degenerate(kind))
    Pt = T(P)
    assert_same(knn(Q, Pt, 'brute'), (od, oi), kind + ' brute')
    assert_same(knn(Q, Pt, 'grid'), (od, oi), kind + ' grid')


# ------------------------------------------------------------------------------------------------ E. both index outputs
def test_both_index_outputs_in_one_call():
    """nerfail_knn8_grid_search with idx_f32 AND idx_i32 (the wrapper only ever passes one): both are written, agree with each
    other and with the oracle."""
    from nerfail_amd import _lib, create_index_and_dist as CI
    lib = _lib.load()
    Q, P, info, od, oi = case('ladders_G16', E.LADDER_FAMILIES['ladders_G16'])
    q, p = T(Q), T(P)
    nq = len(Q)
    ws, nbytes = CI._grid_for(p)
    dist = torch.full((nq, 8), float('nan'), device=dev())
    idx_f = torch.full((nq, 8), float('nan'), device=dev())
    idx_i = torch.full((nq, 8), -1, dtype=torch.int32, device=dev())
    _lib.check(lib.nerfail_knn8_grid_search(_lib.dev(q), nq, len(P), _lib.dev(dist), _lib.dev(idx_f), _lib.dev(idx_i), _lib.dev(ws), nbytes,
                                            _lib.stream()))
    assert np.array_equal(N(idx_f), N(idx_i).astype(np.float32)) and N(idx_i).min() >= 0
    assert_same((N(dist), N(idx_i)), (od, oi), 'both outputs', info)
    H = nq // 20
    dist.fill_(float('nan')); idx_f.fill_(float('nan')); idx_i.fill_(-1)
    _lib.check(lib.nerfail_knn8_grid_search_view(_lib.dev(q), H, 20, len(P), _lib.dev(dist), _lib.dev(idx_f), _lib.dev(idx_i), _lib.dev(ws),
                                                 nbytes, _lib.stream()))
    assert np.array_equal(N(idx_f)[:H * 20], N(idx_i)[:H * 20].astype(np.float32))
    assert_same((N(dist)[:H * 20], N(idx_i)[:H * 20]), (od[:H * 20], oi[:H * 20]), 'both outputs, view entry', info)
    assert np.isnan(N(dist)[H * 20:]).all() and (N(idx_i)[H * 20:] == -1).all()      # nothing written past the view
    CI._GRID.clear()


# ------------------------------------------------------------------------------------------------ F. grid cache
def test_grid_cache_hits_rebuilds_and_evicts(monkeypatch):
    """create_index_and_dist._grid_for: a second call on the same tensor does not rebuild; writing into the tensor in place bumps
    its version and the next answer comes from the NEW set; a fifth set evicts the first, which is rebuilt on its next use and
    still answers correctly."""
    from nerfail_amd import _lib, create_index_and_dist as CI
    lib = _lib.load()
    builds = []
    real = lib.nerfail_knn8_grid_build

    def counting(*a):
        builds.append(a[1])
        return real(*a)
    monkeypatch.setattr(lib, 'nerfail_knn8_grid_build', counting)
    rs = np.random.RandomState(3)
    Q = rs.uniform(-1, 1, (200, 3)).astype(np.float32)
    sets = [rs.uniform(-1, 1, (n, 3)).astype(np.float32) for n in (700, 701, 702, 703, 704)]
    refs = [OK.knn8(Q, S) for S in sets]
    q = T(Q)
    CI._GRID.clear()
    try:
        p0 = T(sets[0])
        assert_same(knn(q, p0, 'grid'), refs[0], 'first call')
        assert builds == [700] and len(CI._GRID) == 1
        assert_same(knn(q, p0, 'grid'), refs[0], 'second call')
        assert builds == [700] and len(CI._GRID) == 1                              # no rebuild
        # in place: the same address and size, another version - and another answer (the points in reverse order)
        flipped = sets[0][::-1].copy()
        ref_flipped = OK.knn8(Q, flipped)
        assert not np.array_equal(ref_flipped[1], refs[0][1])
        v = p0._version
        p0.copy_(T(flipped))
        assert p0._version > v
        assert_same(knn(q, p0, 'grid'), ref_flipped, 'after the in-place change')
        assert builds == [700, 700]
        # five sets: the fifth evicts the first
        CI._GRID.clear()
        del builds[:]
        ps = [T(S) for S in sets]
        for k in range(4):
            assert_same(knn(q, ps[k], 'grid'), refs[k], 'set %d' % k)
        assert builds == [700, 701, 702, 703] and len(CI._GRID) == 4
        key0 = (ps[0].data_ptr(), ps[0]._version, 700)
        assert key0 in CI._GRID
        assert_same(knn(q, ps[4], 'grid'), refs[4], 'set 4')
        assert len(CI._GRID) == 4 and key0 not in CI._GRID
        assert_same(knn(q, ps[1], 'grid'), refs[1], 'set 1 again')                # still cached
        assert builds == [700, 701, 702, 703, 704]
        assert_same(knn(q, ps[0], 'grid'), refs[0], 'set 0 after its eviction')   # rebuilt, and right
        assert builds == [700, 701, 702, 703, 704, 700] and key0 in CI._GRID
    finally:
        CI._GRID.clear()
