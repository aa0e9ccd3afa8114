"""The improvement pipeline of csrc/dcr_sdrf.hip (k_imp_insert, k_imp_rows_count, k_imp_bc, k_imp_emit, imp_enqueue and the
two readers of its result) against the C oracle's literal add / recompute / subtract / remove, value by value: float64
compared with ==, candidates as integers.  The inputs come from tests/improvements_ref.py, which also says — from the
adjacency alone — which strides and which branches of the bookkeeping they reach; those statements are asserted first."""
import ctypes

import numpy as np
import pytest

import improvements_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


@pytest.fixture(scope='module')
def oracle():
    from oracle import c_oracle
    return c_oracle


def check_edge(G, C, x, y, ct):
    """One orientation of one edge: candidates, every improvement, the first arg-max, single candidates, the count."""
    imp, ci, cj = G.improvements(x, y, ct, want_candidates=True)
    imp, ci, cj = np.array(imp), np.array(ci), np.array(cj)   # (views of buffers the next call overwrites)
    oi, oj = C.candidates(x, y)
    assert np.array_equal(ci, oi) and np.array_equal(cj, oj), (x, y, ct, len(ci), len(oi))
    if len(oi) == 0:
        assert imp.shape == (0,) and ci.shape == (0,) and cj.shape == (0,)
        return 0
    want = C.improvements(x, y, oi, oj, ct, nthreads=8)
    bad = np.nonzero(~(imp == want))[0]
    assert np.array_equal(imp, want), \
        (ct, x, y, bad.size, [(int(oi[k]), int(oj[k]), float(imp[k]).hex(), float(want[k]).hex()) for k in bad[:8]])
    k_max = int(np.argmax(want))
    assert G.improvements_argmax() == k_max, (x, y, ct)
    for k in (0, k_max, len(oi) - 1):
        assert G.candidate_at(k) == (int(oi[k]), int(oj[k])), (x, y, ct, k)
    assert G.improvements_count(x, y, ct) == len(oi), (x, y, ct)
    return len(oi)


def check_both(G, C, x, y, ct):
    return check_edge(G, C, x, y, ct) + check_edge(G, C, y, x, ct)


# ---- 1. shaped edges at the kernels' strides -------------------------------------------------------------------------------
@pytest.mark.parametrize('dx,dy,big', R.SHAPES)
def test_shaped_edges_at_the_strides(dcr, oracle, dx, dy, big):
    a = R.shape_args(dx, dy, big)
    ei, n, info = R.shaped(**a)
    R.check_shaped(ei, n, info, dx, dy, big, a['n_tri'])
    G, C = dcr(ei, n), oracle.CGraph(ei, n)
    x, y = info['x'], info['y']
    assert (G.degree(x), G.degree(y)) == (dx, dy) == (C.degree(x), C.degree(y))
    if big:
        assert G.degree(info['big_node']) == C.degree(info['big_node']) > max(big, R.STRIDE)
    kinds = ('bfc', 'augmented') if (dx, dy, big) in R.LARGE_SHAPES else R.KINDS
    total = sum(check_both(G, C, x, y, ct) for ct in kinds)
    print(f'shaped {dx, dy, big}: n = {n}, {total} candidate values over {len(kinds)} kinds and both orientations')
    assert total > 0 or (dx, dy) == (1, 1)


# ---- 2. the maximum bookkeeping, on many small graphs ----------------------------------------------------------------------
def test_maximum_bookkeeping_on_many_small_graphs(dcr, oracle):
    graphs = list(R.small_graphs())
    census = R.census_of(graphs)
    print(f'{census["graphs"]} graphs, {census["edges"]} edges; candidates per branch: '
          + ', '.join(f'{b} {census[b]}' for b in R.BRANCHES))
    for b in R.BRANCHES:   # a condition on the inputs, from the host model alone
        assert census[b] >= R.CENSUS_CAP, (b, census[b])
    values = 0
    for g, (ei, n, edges) in enumerate(graphs):
        G, C = dcr(ei, n), oracle.CGraph(ei, n)
        for ct in (R.KINDS if g % 5 == 0 else ('bfc',)):
            for x, y in edges:
                values += check_edge(G, C, x, y, ct)
    print(f'{values} improvement values identical')


# ---- 3. one handle, many shapes, edits in between --------------------------------------------------------------------------
def _table_size(dx, dy):
    ts = 64
    while ts < 4 * (dx + dy):
        ts <<= 1
    return ts


def test_one_handle_across_sizes_and_edits(dcr, oracle):
    from dcr import synthetic
    a = R.shape_args(513, 512, 0, seed=3)
    ei_a, n_a, info = R.shaped(**a)
    R.check_shaped(ei_a, n_a, info, 513, 512, 0, a['n_tri'])
    ei_b, n_b = synthetic.powerlaw_graph(300, 3, seed=5)
    ei, n = R.disjoint_union(ei_a, n_a, ei_b, n_b)
    G, C = dcr(ei, n), oracle.CGraph(ei, n)
    bx, by = info['x'], info['y']
    eu, ev = C.edges()
    deg = np.array([C.degree(u) for u in range(n)])
    small = min(((int(u), int(v)) for u, v in zip(eu, ev) if u >= n_a), key=lambda e: deg[e[0]] + deg[e[1]])
    assert min(deg[small[0]], deg[small[1]]) == 3
    # the edge of the power-law part whose table lies between the two, with the lighter end first: the edits below outgrow
    # that row's slack (max(8, deg / 4) free places behind a row when the graph is laid out)
    mid = max(((int(u), int(v)) for u, v in zip(eu, ev) if u >= n_a), key=lambda e: deg[e[0]] + deg[e[1]])
    mx, my = mid if deg[mid[0]] <= deg[mid[1]] else mid[::-1]
    ts = [_table_size(deg[p], deg[q]) for p, q in (small, mid, (bx, by))]
    assert ts[0] < ts[1] < ts[2], ts
    print(f'table sizes {ts}; degrees {[(int(deg[p]), int(deg[q])) for p, q in (small, (mx, my), (bx, by))]}')
    for (x, y) in (small, (bx, by), small, (by, bx), (mx, my)):
        assert check_edge(G, C, x, y, 'bfc') > 0

    def both(op, u, v):
        getattr(G, op)(u, v)
        assert getattr(C, op)(u, v) == 0

    rng = np.random.Generator(np.random.PCG64(17))
    slack = max(8, int(deg[mx]) // 4)
    appended = 0
    for step in range(30):
        if step % 2 == 0:   # add: at mx until its row has overflowed, then anywhere (both parts, neighbours of my included)
            pool = C_neighbours(C, my) + rng.integers(0, n, 8).tolist()
            u = mx if appended <= slack + 1 else int(rng.integers(0, n))
            v = next(int(w) for w in rng.permutation(pool + list(range(n))) if w != u and not C.has_edge(u, int(w)))
            both('add_edge', u, v)
            appended += u == mx
        else:               # remove: an edge at my, at a neighbour of mx, or any live edge (never at mx: its row keeps growing)
            pick = step % 6
            if pick == 1:
                u, v = my, next(w for w in C_neighbours(C, my) if w != mx)
            elif pick == 3:
                u = next(w for w in C_neighbours(C, mx) if w != my and C.degree(w) > 1)
                v = next(w for w in C_neighbours(C, u) if w != mx)
            else:
                lu, lv = C.edges()
                k = next(int(k) for k in rng.permutation(len(lu)) if mx not in (lu[k], lv[k]) and (lu[k], lv[k]) != (bx, by)
                         and (lv[k], lu[k]) != (bx, by))
                u, v = int(lu[k]), int(lv[k])
            both('remove_edge', u, v)
        if step % 3 == 2:
            check_edge(G, C, mx, my, 'bfc')
            lu, lv = C.edges()
            k = int(rng.integers(0, len(lu)))
            if (int(lu[k]), int(lv[k])) in ((bx, by), (by, bx)):
                k = (k + 1) % len(lu)
            check_edge(G, C, int(lu[k]), int(lv[k]), 'bfc')
    assert appended > slack, (appended, slack)   # the row of mx was laid out again on the way
    assert np.array_equal(G.to_edge_index(), C.to_edge_index())
    check_edge(G, C, bx, by, 'augmented')        # every row has moved since this edge was last asked for
    check_edge(G, C, my, mx, 'bfc')

    # the arg-min step hands its degrees to the next improvement call; an edit in between must drop them
    u, v, val = G.curvature_pass_argmin('bfc')
    ou, ov, oc = C.curv_all('bfc', nthreads=8)
    m = int(np.argmin(oc))
    assert (u, v, val) == (int(ou[m]), int(ov[m]), float(oc[m]))
    assert check_edge(G, C, u, v, 'bfc') > 0
    w = next(w for w in range(n) if w != u and not C.has_edge(u, w))
    both('add_edge', u, w)
    assert check_edge(G, C, u, v, 'bfc') > 0
    assert G.degree(u) == C.degree(u)


def C_neighbours(C, u):
    lu, lv = C.edges()
    return [int(b) for a, b in zip(lu, lv) if a == u] + [int(a) for a, b in zip(lu, lv) if b == u]


# ---- 4. families ----------------------------------------------------------------------------------------------------------
def _family(name):
    from dcr import synthetic
    if name == 'dense':
        return synthetic.erdos_renyi_graph(300, 0.5, seed=2) + ('haantjes',)
    if name == 'grid':
        return synthetic.grid_graph(12, 9) + ('1d',)
    if name == 'star':
        return R.star_with_leaf_edge(3000) + ('augmented',)
    import fuzz_parity
    seed = 58
    assert int(np.random.Generator(np.random.PCG64(seed)).integers(0, 6)) == 3   # the stars joined by random edges
    return fuzz_parity.random_graph(np.random.Generator(np.random.PCG64(seed)), 0.0) + ('augmented',)


# (the dense graph's twelve edges in four cases of three: the oracle adds and recomputes around ~150-neighbour endpoints)
@pytest.mark.parametrize('name,part,parts', [('dense', 0, 4), ('dense', 1, 4), ('dense', 2, 4), ('dense', 3, 4), ('grid', 0, 1),
                                             ('star', 0, 1), ('stars', 0, 1)])
def test_families(dcr, oracle, name, part, parts):
    ei, n, classical = _family(name)
    G, C = dcr(ei, n), oracle.CGraph(ei, n)
    eu, ev = C.edges()
    deg = np.array([C.degree(u) for u in range(n)])
    picks = R.ranked_edges(eu, ev, deg)
    assert len(picks) == 12
    picks = picks[part::parts]
    if name == 'star':
        assert (1, 2) in picks and deg[0] == 3000 and deg[1] == 2 and deg[3] == 1
    total = sum(check_both(G, C, x, y, ct) for x, y in picks for ct in ('bfc', classical))
    print(f'{name}: n = {n}, {len(picks)} edges, {total} candidate values')
    assert total > 0


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(dcr, oracle):
    from dcr import _lib
    L = _lib.lib()
    ei = R.undirected_edge_index([(0, 1), (1, 2), (2, 3), (4, 5)])
    G, C = dcr(ei, 6), oracle.CGraph(ei, 6)
    n = ctypes.c_int64(-7)
    pi, pci, pcj = _lib._f64p(), _lib._i32p(), _lib._i32p()

    def improvements(x, y, ct, n_out=ctypes.byref(n)):
        return L.dcr_improvements(G._h, x, y, ct, 1, n_out, ctypes.byref(pi), ctypes.byref(pci), ctypes.byref(pcj))

    i, j, k = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    assert check_edge(G, C, 1, 2, 'bfc') > 0
    for x, y, ct in ((1, 1, 0), (1, 6, 0), (-1, 2, 0), (1, 2, 4), (1, 2, -1)):
        assert improvements(x, y, ct) == -1 and L.dcr_last_error(), (x, y, ct)   # DCR_EINVAL
        assert n.value == -7
    assert improvements(1, 2, 0, None) == -1
    n_live = check_edge(G, C, 2, 1, 'bfc')
    assert n_live > 0
    for bad in (-1, n_live, 1 << 40):
        assert L.dcr_candidate_at(G._h, bad, ctypes.byref(i), ctypes.byref(j)) == -1, bad
    assert G.candidate_at(n_live - 1) == tuple(int(c[-1]) for c in C.candidates(2, 1))
    assert check_edge(G, C, 4, 5, 'bfc') == 0                    # an isolated edge has no candidate
    assert L.dcr_improvements_argmax(G._h, ctypes.byref(k)) == -6   # DCR_ESTATE
    assert L.dcr_candidate_at(G._h, 0, ctypes.byref(i), ctypes.byref(j)) == -1
    for ct in R.KINDS:
        assert check_both(G, C, 0, 1, ct) > 0
