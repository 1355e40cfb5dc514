"""Inputs that put the grid 8-NN search (nerfail_amd/csrc/knn_grid.hip) ON its decisions: points a float step either side of a
cell face, exact ties between points of different cells, waves whose group sizes sit on the grouping thresholds, degenerate
sets (numpy only; shared by tests/test_knn_edge_inputs.py, which counts on the oracle and on the emulation below what the
inputs reach, and by tests/test_hip_knn_edges.py, which compares the kernels with oracle/knn.py bit for bit).

The module holds a float32 emulation of the build's own formulas: grid_dim_for, the bounding box with cs = ext * 1.0001f / G
and inv_cs = 1 / cs, cell_coord (exact: a subtract followed by a multiply cannot fuse), and the face a box is drawn from,
o + x * cs, in both forms a compiler may emit: two roundings (unfused) and one (fused: float32 of the float64 value, the
product of two float32 being exact in float64). A point is BINNED by cell_coord and PRUNED by the drawn box; the two disagree
near a face by the rounding of (v - o) and of inv_cs, a few float steps of |o| + extent - thousands of steps of v itself
where a face lies next to 0. `transition` finds where the binning really changes cell; every ladder is centred there.

Every generator returns (Q, P) float32 with the order of the points permuted, and asserts that the final point count gives the
grid size it planned for. A generator that takes `info` fills that dict with what the tests count on (ladders, lanes ...).
"""
import numpy as np

from oracle import knn as OK

F32 = np.float32

K_SHELL_CAP = 3           # knn_grid.hip: kShellCap, kCoarse, kCoherentCells, kGroupPasses, kMinGroup
K_COARSE = 4
K_COHERENT = 6
K_GROUP_PASSES = 4
K_MIN_GROUP = 8


# ---------------------------------------------------------------------------------------------- float steps
def f2o(v):
    """float32 -> an integer that orders like the float and moves by 1 per float step (-0 and +0 share 0)."""
    i = np.asarray(v, F32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7fffffff))


def o2f(o):
    o = np.asarray(o, np.int64)
    bits = np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32)
    return bits.view(F32)


def step(v, n):
    """v moved by n float steps (n an integer or an array of integers)."""
    return o2f(f2o(v) + np.asarray(n, np.int64))


# ---------------------------------------------------------------------------------------------- the build's formulas
def grid_dim_for(n):
    G = int(np.floor(np.cbrt(float(n)) + 0.5))                    # lround of a positive value
    return min(max(G, 4), 256)


class Grid(object):
    """bbox_kernel + grid_params_kernel: origin o[3], cs, inv_cs, G - float32 throughout."""

    def __init__(self, P):
        P = np.asarray(P, F32).reshape(-1, 3)
        self.G = grid_dim_for(P.shape[0])
        lo, hi = P.min(0), P.max(0)
        ext = F32((hi - lo).max())
        if not ext > 0:
            ext = F32(1)
        self.o = lo.astype(F32)
        self.cs = F32(F32(ext * F32(1.0001)) / F32(self.G))
        self.inv_cs = F32(F32(1) / self.cs)
        self.Gc = (self.G + K_COARSE - 1) // K_COARSE
        self.Gs = (self.Gc + K_COARSE - 1) // K_COARSE

    def raw_coord(self, v, axis):
        """floorf((v - o) * inv_cs) before the clamp."""
        t = ((np.asarray(v, F32) - self.o[axis]).astype(F32) * self.inv_cs).astype(F32)
        return np.floor(t).astype(np.int64)

    def coord(self, v, axis):
        return np.clip(self.raw_coord(v, axis), 0, self.G - 1)

    def cells(self, X):
        X = np.asarray(X, F32).reshape(-1, 3)
        return np.stack([self.coord(X[:, a], a) for a in range(3)], 1)

    def face(self, axis, x, fused):
        """o + (float)x * cs as the search computes the low face of cell x (and the high face of cell x - 1)."""
        if fused:
            return F32(np.float64(self.o[axis]) + np.float64(x) * np.float64(self.cs))
        return F32(self.o[axis] + F32(F32(x) * self.cs))

    def centre(self, axis, j):
        return F32(np.float64(self.o[axis]) + (j + 0.5) * np.float64(self.cs))

    def transition(self, axis, k):
        """The first float32 that is binned into cell k or above on `axis` (0 < k < G): cell_coord is monotonic in v."""
        f = np.float64(self.face(axis, k, True))
        lo, hi = int(f2o(F32(f - 0.5 * self.cs))), int(f2o(F32(f + 0.5 * self.cs)))
        assert self.raw_coord(o2f(lo), axis) < k <= self.raw_coord(o2f(hi), axis)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if self.raw_coord(o2f(mid), axis) >= k:
                hi = mid
            else:
                lo = mid
        return F32(o2f(hi))

    def face_offset(self, axis, k, fused):
        """M: float steps from the computed face k up to the binning transition (M > 0: the M values below the transition that
        the drawn box of cell k contains are binned into cell k - 1; M < 0: -M values binned into k lie in the box of k - 1)."""
        return int(f2o(self.transition(axis, k)) - f2o(self.face(axis, k, fused)))


def box_cell(g, v, axis, fused):
    """The cell whose DRAWN box [face(x), face(x + 1)) contains v (clamped like the binning)."""
    faces = np.array([g.face(axis, x, fused) for x in range(1, g.G)], F32)
    return np.searchsorted(faces, np.asarray(v, F32), side='right')


# ---------------------------------------------------------------------------------------------- the shell walk's stopping rule
def bin_slack(g):
    """kBinSlack of knn_grid.hip: the absolute amount every drawn box grows by before a distance to it is taken,
    2^-21 (max |o_a| + cs * 16 * Gs) in float32 (derivation next to the constant and in DESIGN.md section 2)."""
    return F32(F32(2.0 ** -21) * F32(np.abs(g.o).max() + F32(g.cs * F32(g.Gs * K_COARSE * K_COARSE))))


def emulated_shell_rule(Q, P, fused, slack=False):
    """shell_walk of knn8_grid_kernel as written, in float32: the block [c - R, c + R]^3 of BINNED cells is scanned exhaustively
    (the per-cell pruning inside the block is left out: it can only lose more), then the lower bound to everything unvisited is
    taken from the drawn faces and the walk stops when d8 < (0.999f * bound)^2 - the rule before the slack; slack=True takes
    bin_slack off the bound first, as the kernel does now. A query that does not stop within kShellCap
    shells, lies far outside the grid or has an empty coarse neighbourhood goes to the wave search: it gets the exact answer.
    Returns (idx [nq,8] int32, stopped [nq] bool)."""
    Q, P = np.asarray(Q, F32).reshape(-1, 3), np.asarray(P, F32).reshape(-1, 3)
    g = Grid(P)
    G, cs = g.G, g.cs
    pc, qc = g.cells(P), g.cells(Q)
    _, exact = OK.knn8(Q, P)
    out, stopped = exact.copy(), np.zeros(len(Q), bool)
    ext = F32(cs * F32(G))
    coarse_pop = np.zeros((g.Gc,) * 3, np.int64)
    np.add.at(coarse_pop, tuple((pc // K_COARSE).T), 1)
    for n in range(len(Q)):
        q, c = Q[n], qc[n]
        outside = max(max(F32(g.o[a] - q[a]), F32(q[a] - F32(g.o[a] + ext))) for a in range(3))
        if outside > F32(F32(K_SHELL_CAP + 1) * cs):
            continue
        C = c // K_COARSE
        sl = tuple(slice(max(C[a] - 1, 0), min(C[a] + 1, g.Gc - 1) + 1) for a in range(3))
        if coarse_pop[sl].sum() == 0:
            continue
        cheb = np.abs(pc - c).max(1)
        near = np.flatnonzero(cheb <= K_SHELL_CAP)
        d2 = OK.d2_f32(q[None, :], P[near])
        order = np.lexsort((near, d2))
        near, d2, ring = near[order], d2[order], cheb[near[order]]
        for R in range(0, min(K_SHELL_CAP, G - 1) + 1):
            keep = np.flatnonzero(ring <= R)[:8]
            d8 = d2[keep[7]] if len(keep) == 8 else F32(np.inf)
            bound = F32(np.inf)
            for a in range(3):
                if c[a] - R > 0:
                    bound = min(bound, F32(q[a] - g.face(a, c[a] - R, fused)))
                if c[a] + R < G - 1:
                    bound = min(bound, F32(g.face(a, c[a] + R + 1, fused) - q[a]))
            done = bound == np.inf
            if slack and not done:
                bound = F32(bound - bin_slack(g))
            if not done and bound > 0:
                sb = F32(F32(0.999) * bound)
                done = d8 < F32(sb * sb)
            if done:
                out[n, :len(keep)] = near[keep]
                stopped[n] = True
                break
    return out, stopped


# ---------------------------------------------------------------------------------------------- face ladders
ORIGIN = (-1.3712, -0.7301, -1.4507)      # no power of two; x and z put a face next to 0 at G = 16 and 18 (see _origin)
EXTENT = 2.9


def _origin(G, offset, extent=EXTENT):
    """Origin per axis: on x and z the corner is moved so that one face of the middle of the grid falls within a few 1e-4 of
    0 (there a float step of v is ~1e-11 while the binning works on v - o ~ 1.4: transition and drawn face lie thousands of steps
    apart); y stays ordinary (a face is a few steps off at most). With an offset every coordinate has one sign and a float step
    is a visible fraction of a cell."""
    cs = extent * 1.0001 / G
    o = np.array(ORIGIN, np.float64)
    o[0] = -(round(-o[0] / cs)) * cs - 3.1e-4
    o[2] = -(round(-o[2] / cs)) * cs + 2.3e-4
    return (o + offset).astype(F32)


def _cloud(G, offset, n_fill, rs, extent=EXTENT):
    """Two corner points that pin the bbox (extent EXTENT on every axis) and a uniform filler between them."""
    o = _origin(G, offset, extent)
    hi = (o.astype(np.float64) + extent).astype(F32)
    fill = (o.astype(np.float64) + rs.uniform(0.02, 0.98, (n_fill, 3)) * extent).astype(F32)
    return np.concatenate([o[None], hi[None], fill]).astype(F32)


def _plan_grid(G, offset, n_total, extent=EXTENT):
    """The grid that a set of n_total points with the corners of _cloud will get (the ladders are placed on ITS transitions)."""
    assert grid_dim_for(n_total) == G, (n_total, G)
    o = _origin(G, offset, extent)
    hi = (o.astype(np.float64) + extent).astype(F32)
    g = Grid(np.concatenate([np.stack([o, hi])] * ((n_total + 1) // 2))[:n_total])
    assert g.G == G
    return g


def ladder_offsets(steps, reach=48):
    """Offsets (float steps from the transition) of a ladder with the given step pattern, 0 included, at least `reach` each way."""
    up, k = [0], 0
    while up[-1] < reach:
        up.append(up[-1] + steps[k % len(steps)])
        k += 1
    up = np.array(up, np.int64)
    return np.concatenate([-up[:0:-1], up])


def _finish(Q, P, g, rs):
    """Permute the points, check the plan, return float32 copies."""
    P = np.ascontiguousarray(P[rs.permutation(len(P))], F32)
    got = Grid(P)
    assert got.G == g.G and got.cs == g.cs and np.array_equal(got.o, g.o), 'the set does not give the planned grid'
    return np.ascontiguousarray(Q, F32), P


def ladder_faces(G):
    """Faces near both ends and in the middle of the grid; at G = 18 face 16 also separates two blocks of coarse cells."""
    return (1, G // 2 - 1, G // 2, G - 1) if G == 16 else (1, G // 2, 16, G - 1)


def face_ladders(G=16, offset=0.0, steps=(1,), seed=0, info=None):
    """Twelve ladders - three axes x four faces - of points `steps` float steps apart along one axis, centred on the emulated
    binning transition of the face, the other two coordinates at a cell centre; the queries are every ladder point, ladder by
    ladder. G = 16: 4166 points with one-step ladders (one block of coarse cells); G = 18: about 6000 (ragged coarse cells,
    2^3 blocks). info: grid, ladders = [(axis, face, first query, query count)]."""
    rs = np.random.RandomState(seed)
    offs = ladder_offsets(steps)
    n_total = 4166 if G == 16 else 6000
    assert G in (16, 18)
    n_ladder = 12 * len(offs)
    g = _plan_grid(G, offset, n_total)
    ladders, pts = [], []
    for axis in range(3):
        for k in ladder_faces(G):
            T = g.transition(axis, k)
            line = np.empty((len(offs), 3), F32)
            line[:, axis] = step(T, offs)
            for b in range(3):
                if b != axis:
                    line[:, b] = g.centre(b, rs.randint(1, G - 1))
            ladders.append((axis, k, len(pts) * len(offs), len(offs)))
            pts.append(line)
    L = np.concatenate(pts)
    assert len(np.unique(L, axis=0)) == len(L)
    P = np.concatenate([_cloud(G, offset, n_total - 2 - n_ladder, rs), L])
    if info is not None:
        info.update(grid=g, ladders=ladders, offsets=offs)
    return _finish(L.copy(), P, g, rs)


def hand_clusters(G=16, extent=3.3, seed=0, info=None):
    """The construction that needs no luck. Lower face (transition T of face k, drawn face M >= 3 steps below it): query q = T + 1
    step, seven copies of q and q + 3 steps in cell k, p = q - 2 steps still binned into cell k - 1: shell 0 finds eight keys with
    d8 = 9 u^2, the bound to the drawn face is (M + 1) u > 3 u / 0.999, the walk stops and p - the true 8th neighbour - is lost.
    Mirrored for the upper face (drawn face M' >= 2 steps above T): q = T - 2 steps, seven copies, q - 3 steps, p = q + 2 steps = T.
    Up to four faces of each kind per axis, chosen where BOTH face forms are that far off (which way a face is off follows the
    rounding of inv_cs and of v - o: the extent is one that gives both kinds at this G). info: grid, clusters = [(axis, face,
    'lower' | 'upper', query index)]."""
    rs = np.random.RandomState(seed + 100)
    n_total = 4166 if G == 16 else 6000
    g = _plan_grid(G, 0.0, n_total, extent)
    clusters, pts, qs = [], [], []
    for axis in range(3):
        taken = {'lower': 0, 'upper': 0}
        for k in range(1, G):
            M = [g.face_offset(axis, k, fused) for fused in (False, True)]
            kind = 'lower' if min(M) >= 3 else ('upper' if max(M) <= -2 else None)
            if kind is None or taken[kind] == 4:
                continue
            taken[kind] += 1
            T = g.transition(axis, k)
            s = 1 if kind == 'lower' else -1
            q = step(T, 1) if kind == 'lower' else step(T, -2)
            xs = [q] * 7 + [step(q, 3 * s), step(q, -2 * s)]
            c = np.empty((9, 3), F32)
            c[:, axis] = xs
            for b in range(3):
                if b != axis:
                    c[:, b] = g.centre(b, rs.randint(1, G - 1))
            clusters.append((axis, k, kind, len(qs)))
            qs.append(c[0])
            pts.append(c)
    assert len([c for c in clusters if c[2] == 'lower']) >= 2 and len([c for c in clusters if c[2] == 'upper']) >= 2
    C = np.concatenate(pts)
    P = np.concatenate([_cloud(G, 0.0, n_total - 2 - len(C), rs, extent), C])
    if info is not None:
        info.update(grid=g, clusters=clusters)
    return _finish(np.array(qs, F32), P, g, rs)


# name -> generator of the ladder families (each must fail under the emulated stopping rule, see test_knn_edge_inputs.py)
LADDER_FAMILIES = {
    'ladders_G16': lambda info=None: face_ladders(16, info=info),
    'ladders_G18': lambda info=None: face_ladders(18, seed=1, info=info),
    'steps23_G16': lambda info=None: face_ladders(16, steps=(2, 3), seed=2, info=info),
    'steps23_G18': lambda info=None: face_ladders(18, steps=(2, 3), seed=3, info=info),
    'clusters_G16': lambda info=None: hand_clusters(16, 3.3, info=info),
    'clusters_G18': lambda info=None: hand_clusters(18, 3.5, info=info),
}
# the same ladder sets built far from the origin: every coordinate positive / negative (the bbox atomics take the other
# branch), a float step is 2^-13 (+1024) or 2^-10 / 2^-9 (-16384, the sets straddle the binade) - up to 1 / 90 of a cell
FAR_FAMILIES = {
    'ladders_G16_at_+1024': lambda info=None: face_ladders(16, 1024.0, seed=4, info=info),
    'ladders_G18_at_+1024': lambda info=None: face_ladders(18, 1024.0, seed=5, info=info),
    'ladders_G16_at_-16384': lambda info=None: face_ladders(16, -16384.0, seed=6, info=info),
    'ladders_G18_at_-16384': lambda info=None: face_ladders(18, -16384.0, seed=7, info=info),
}


# ---------------------------------------------------------------------------------------------- exact ties across cells
LATTICE_H = F32(0.125)


def tie_lattice(seed=0, info=None):
    """10^3 points on a cubic lattice of spacing h = 2^-3 from -1, plus a tight clump of 3096 points in the middle of the last
    lattice cube (4096 points, G = 16: a cell is 0.5626 h, so the members of a tie lie one or two cells from the query, in
    different shells). Queries at lattice points, edge midpoints, face centres and cube centres, on the hull and inside, at least
    2 h from the clump: every coordinate is a multiple of 2^-4 below 1, every d2 exact, and the nearest keys come in 6-, 2-, 4-
    and 8-fold ties (then 12-, 8-, 8- and 24-fold ones) whose members lie in different cells; which of the tied 8th / 9th keys
    wins is decided by the permuted index alone. info: grid, kind [nq] (0 lattice point, 1 edge, 2 face, 3 cube)."""
    rs = np.random.RandomState(seed + 200)
    n = 10
    ax = (F32(-1) + np.arange(n).astype(F32) * LATTICE_H).astype(F32)
    lattice = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)
    clump = (float(ax[n - 2]) + 0.0625 + rs.normal(scale=1e-3, size=(4096 - n ** 3, 3))).astype(F32)
    P = np.concatenate([lattice, clump])
    half = LATTICE_H / F32(2)
    shifts = {0: [(0, 0, 0)], 1: [(1, 0, 0), (0, 1, 0), (0, 0, 1)], 2: [(1, 1, 0), (1, 0, 1), (0, 1, 1)], 3: [(1, 1, 1)]}
    qs, kinds = [], []
    for kind, ss in shifts.items():
        for s in ss:
            base = rs.randint(0, n - 3, (40, 3))
            base[:5] = [(0, 0, 0), (n - 4, n - 4, n - 4), (0, 3, n - 4), (3, 3, 3), (4, 0, 2)]               # hull + inside
            qs.append(ax[base] + np.array(s, F32) * half)
            kinds += [kind] * len(base)
    Q = np.concatenate(qs).astype(F32)
    g = Grid(P)
    assert g.G == 16
    if info is not None:
        info.update(grid=g, kind=np.array(kinds))
    return _finish(Q, P, g, rs)


# ---------------------------------------------------------------------------------------------- wave compositions
def _wave_points(rs):
    """The point set of the wave compositions (4166 points, G = 16): cloud, 8 copies of the centre of each anchor cell
    (coordinates 1, 5, 9, 13 on every axis: 64 cells, 4 cells apart) and one ladder across face 8 of x in the row (y, z) = (3, 3)."""
    G, n_total = 16, 4166
    g = _plan_grid(G, 0.0, n_total)
    anchors = np.array([(x, y, z) for z in (1, 5, 9, 13) for y in (1, 5, 9, 13) for x in (1, 5, 9, 13)])
    A = np.stack([[g.centre(a, c[a]) for a in range(3)] for c in anchors]).astype(F32)
    offs = ladder_offsets((1,))
    L = np.empty((len(offs), 3), F32)
    L[:, 0] = step(g.transition(0, 8), offs)
    L[:, 1], L[:, 2] = g.centre(1, 3), g.centre(2, 3)
    P = np.concatenate([_cloud(G, 0.0, n_total - 2 - 8 * len(A) - len(L), rs), np.repeat(A, 8, axis=0), L])
    return g, anchors, A, L, P


def _in_cell(g, centre, n, rs):
    """n distinct queries within 0.05 cells of a cell centre (the 8 copies there are their 8 neighbours or close to it)."""
    return (centre.astype(np.float64) + rs.uniform(-0.05, 0.05, (n, 3)) * float(g.cs)).astype(F32)


WAVE_KINDS = ('g7', 'g8', 'g9', 'g8_late', 'five_groups', 'one_ladder', 'last_1', 'last_63')


def wave_composition(kind, seed=0, info=None):
    """Queries for the flat entry (64 consecutive queries = one wave) on the point set of _wave_points.
      g7 | g8 | g9   lanes 0 .. g-1 inside one anchor cell, the other 64 - g lanes on anchor centres of their own (more than 3 cells
                     from each other and from the group);
      g8_late        the same 8 + 56 lanes with the group in lanes 56 .. 63 (a scattered lane names the first group);
      five_groups    lanes 12 i .. 12 i + 11 inside anchor cell i (i = 0 .. 4) - one group more than kGroupPasses - and 4 scattered;
      one_ladder     64 consecutive points of the ladder;
      last_1         one_ladder plus a 65th query (a last wave with 1 valid lane); last_63: 63 ladder points (63 valid lanes).
    info: grid, group [nq] (-1 scattered, else the number of the lane's group), searched = what the kernel's second work
    counter must read for this launch (None where the kernel's rules do not fix it)."""
    rs = np.random.RandomState(seed + 300)
    g, anchors, A, L, P = _wave_points(rs)
    pick = rs.permutation(len(A))
    searched = None
    if kind in ('g7', 'g8', 'g9', 'g8_late'):
        n = int(kind[1])
        grp = _in_cell(g, A[pick[0]], n, rs)
        rest = A[pick[1:65 - n]]
        Q = np.concatenate([rest, grp] if kind == 'g8_late' else [grp, rest])
        group = np.array([-1] * (64 - n) + [0] * n if kind == 'g8_late' else [0] * n + [-1] * (64 - n))
        # lane 0 names the first group. In the group and >= kMinGroup lanes: those lanes search as a wave, everything else
        # finishes in shell 0 (8 copies of a cell centre: d8 <= (0.087 cs)^2 against a bound of ~0.45 cs). Fewer lanes, or a
        # scattered lane 0 (a group of 1): the grouping ends and EVERY lane takes the shell walk - no wave search at all.
        searched = n if (n >= K_MIN_GROUP and kind != 'g8_late') else 0
    elif kind == 'five_groups':
        Q = np.concatenate([_in_cell(g, A[pick[i]], 12, rs) for i in range(5)] + [A[pick[5:9]]])
        group = np.array(sum([[i] * 12 for i in range(5)], []) + [-1] * 4)
        searched = 12 * K_GROUP_PASSES                           # the fifth group walks the shells lane by lane
    else:
        nq = {'one_ladder': 64, 'last_1': 65, 'last_63': 63}[kind]
        Q = L[10:10 + nq].copy()
        group = np.zeros(nq, np.int64)
        searched = nq                                             # every valid lane is in the one group of its wave
    if info is not None:
        info.update(grid=g, group=group, searched=searched, anchors=anchors)
    return _finish(Q, P, g, rs)


def tiled_view(seed=0, info=None):
    """A view of 9 x 17 pixels (8 x 8 tiles: 2 x 3 of them, the last row and column 1 pixel wide) whose pixels, row by row, walk
    up the ladder of _wave_points and then over anchor cells: every tile holds several pieces of the ladder. Q is [9, 17, 3]."""
    rs = np.random.RandomState(seed + 400)
    g, anchors, A, L, P = _wave_points(rs)
    extra = np.concatenate([_in_cell(g, A[i], 8, rs) for i in range(7)])
    Q = np.concatenate([L, extra])[:9 * 17].reshape(9, 17, 3)
    if info is not None:
        info.update(grid=g, n_ladder=len(L))
    Qf, P = _finish(Q.reshape(-1, 3), P, g, rs)
    return Qf.reshape(9, 17, 3), P


# ---------------------------------------------------------------------------------------------- degenerate sets
DEGENERATE_KINDS = ('same_8', 'same_100', 'two_places', 'eight_points')


def degenerate(kind, seed=0):
    """same_8 | same_100: identical points (extent 0: the build falls back to extent 1); two_places: 50 + 50 copies of two
    locations; eight_points: exactly 8 distinct points, the queries 10 cells outside the box on every side as well as inside."""
    rs = np.random.RandomState(seed + 500)
    a = np.array([0.37, -1.21, 2.05], F32)
    if kind in ('same_8', 'same_100'):
        P = np.repeat(a[None], 8 if kind == 'same_8' else 100, axis=0)
        Q = np.concatenate([a[None], a[None] + rs.uniform(-3, 3, (40, 3)).astype(F32), step(a, 1)[None], step(a, -1)[None]])
    elif kind == 'two_places':
        b = np.array([0.41, -1.21, 2.05], F32)
        P = np.concatenate([np.repeat(a[None], 50, axis=0), np.repeat(b[None], 50, axis=0)])
        mid = ((a.astype(np.float64) + b) / 2).astype(F32)
        Q = np.concatenate([a[None], b[None], mid[None], step(mid, 1)[None], step(mid, -1)[None], a[None] + rs.uniform(-1, 1, (40, 3)).astype(F32)])
    else:
        P = (a + rs.uniform(0, 1, (8, 3))).astype(F32)
        g = Grid(P)
        far = 10.0 * float(g.cs)
        lo, hi = P.min(0).astype(np.float64), P.max(0).astype(np.float64)
        out = [np.where(np.arange(3) == ax, (lo - far) if side == 0 else (hi + far), (lo + hi) / 2) for ax in range(3) for side in (0, 1)]
        out += [lo - far, hi + far]
        Q = np.concatenate([np.array(out), P, rs.uniform(lo, hi, (30, 3))]).astype(F32)
    P = np.ascontiguousarray(P[rs.permutation(len(P))], F32)
    assert Grid(P).G == (5 if kind in ('same_100', 'two_places') else 4)
    return np.ascontiguousarray(Q, F32), P
