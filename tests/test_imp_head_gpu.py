"""The head of the SDRF step (csrc/dcr_sdrf.hip: k_imp_insert's row descriptors, k_imp_rows_count starting from them, classes B
and C folded into k_imp_emit, the closing scan's 1,024-row step, k_draw_partial) on small hand-built graphs at the edges of what
those kernels do: candidates in order, every improvement as an exact float64, the count; the device draw against the host's
``draw_index`` on the same improvements.  The inputs' builders and the row model are tests/improvements_ref.py's; the values
come from the C oracle's literal add / recompute / subtract, as in tests/test_improvements_gpu.py."""
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


def edge_graph(dx, dy, n_tri=0, n_sq=0, big_deg=0, seed=0, ids=None):
    """An edge (x, y) with deg(x) = dx, deg(y) = dy, ``n_tri`` common neighbours and ``n_sq`` edges between the private
    neighbourhoods; with ``big_deg`` the first private neighbour of x has exactly that degree, and its LAST entries are its
    neighbours in N(y) (they lie behind every stride of its row).  ``ids``: node ids of (x, y, triangle nodes, x's private
    neighbours, y's private neighbours), the rest follow; default: a seeded permutation.  Returns (edge_index, n, x, y, big)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    px, py = dx - 1 - n_tri, dy - 1 - n_tri
    assert px >= 0 and py >= 0
    tri = list(range(2, 2 + n_tri))
    ax = list(range(2 + n_tri, 2 + n_tri + px))
    ay = list(range(2 + n_tri + px, 2 + n_tri + px + py))
    core = 2 + n_tri + px + py
    pairs = [(0, 1)] + [(0, t) for t in tri] + [(1, t) for t in tri] + [(0, a) for a in ax] + [(1, b) for b in ay]
    n_sq = min(n_sq, px * py)
    big_sq = min(3, py) if big_deg else 0
    cells = [c for c in rng.permutation(px * py).tolist() if not (big_deg and c // py == 0)][:max(n_sq - big_sq, 0)]
    pairs += [(ax[c // py], ay[c % py]) for c in cells]
    order = rng.permutation(len(pairs)).tolist()
    pairs = [pairs[k] for k in order]
    n = core
    if big_deg:
        fill = big_deg - 1 - big_sq
        assert px >= 1 and fill >= 0
        pairs += [(ax[0], core + k) for k in range(fill)] + [(ax[0], ay[k]) for k in range(big_sq)]
        n = core + fill
    if ids is None:
        perm = rng.permutation(n)
    else:
        ids = np.asarray(ids, dtype=np.int64)
        assert ids.shape[0] == core
        total = max(n, int(ids.max()) + 1)          # (ids beyond the nodes in use: the others stay isolated)
        perm = np.concatenate([ids, np.setdiff1d(np.arange(total), ids)[:n - core]])
        assert len(set(perm.tolist())) == n
        n = total
    pairs = [(int(perm[u]), int(perm[v])) for u, v in pairs]
    return R.undirected_edge_index(pairs), n, int(perm[0]), int(perm[1]), int(perm[ax[0]]) if big_deg else -1


def check_edge(G, C, x, y, ct='bfc'):
    """Candidates in order, every improvement, the count, for one orientation of one edge.  Returns (imp, ci, cj)."""
    imp, ci, cj = G.improvements(x, y, ct, want_candidates=True)
    imp, ci, cj = np.array(imp), np.array(ci), np.array(cj)
    oi, oj = C.candidates(x, y)
    assert np.array_equal(ci, oi) and np.array_equal(cj, oj), (x, y, ct, len(ci), len(oi))
    assert G.improvements_count(x, y, ct) == len(oi)
    if len(oi) == 0:
        assert imp.shape == (0,)
        return imp, ci, cj
    want = C.improvements(x, y, oi, oj, ct, nthreads=8)
    bad = np.nonzero(~(imp == want))[0]
    assert np.array_equal(imp, want), \
        (ct, x, y, bad.size, [(int(oi[k]), int(oj[k]), float(imp[k]).hex(), float(want[k]).hex()) for k in bad[:8]])
    return imp, ci, cj


def check_both(G, C, x, y, kinds=('bfc',)):
    total = 0
    for ct in kinds:
        total += len(check_edge(G, C, x, y, ct)[0]) + len(check_edge(G, C, y, x, ct)[0])
    return total


# ---- row length around the 4 x 256 look-up step ------------------------------------------------------------------------------
@pytest.mark.parametrize('deg', [1023, 1024, 1025])
def test_neighbour_row_around_the_lookup_step(dcr, oracle, deg):
    ei, n, x, y, big = edge_graph(9, 6, n_tri=1, n_sq=6, big_deg=deg, seed=deg)
    rows = R.rows_of(ei, n)
    assert len(rows[x]) == 9 and len(rows[y]) == 6 and len(rows[big]) == deg
    assert rows[big][-1] in rows[y] and rows[big][-3] in rows[y]             # found only by the row's last look-ups
    assert any(len(rows[i]) == 1 for i in rows[x])                           # a neighbour whose only entry is x itself
    G, C = dcr(ei, n), oracle.CGraph(ei, n)
    assert check_both(G, C, x, y, ('bfc', 'augmented')) > 0
    assert check_both(G, C, x, big) > 0                                      # the long row as row y and as row x


# ---- row count around the scan's steps, bitmap width around the word boundaries ------------------------------------------------
@pytest.mark.parametrize('rows', [64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_row_count_around_the_scan_steps(dcr, oracle, rows):
    ei, n, x, y, _ = edge_graph(rows - 1, 4, n_tri=1, n_sq=2 * rows, seed=rows)
    G, C = dcr(ei, n), oracle.CGraph(ei, n)
    assert (G.degree(x), G.degree(y)) == (rows - 1, 4)
    imp, _, _ = check_edge(G, C, x, y)
    assert len(imp) > rows                                                   # (every row has candidates: the offsets matter)
    check_edge(G, C, y, x)


@pytest.mark.parametrize('nb', [31, 32, 33, 64, 65])
def test_bitmap_width_around_the_word_boundaries(dcr, oracle, nb):
    ei, n, x, y, _ = edge_graph(6, nb - 1, n_tri=2, n_sq=3 * nb, seed=nb)
    G, C = dcr(ei, n), oracle.CGraph(ei, n)
    assert G.degree(y) + 1 == nb
    imp, ci, cj = check_edge(G, C, x, y, 'bfc')
    # the last position of the bitmap (j == y) and the last of row y are among the candidates: the live mask kept them
    last_y = R.rows_of(ei, n)[y][-1]
    pairs = set(zip(ci.tolist(), cj.tolist()))
    assert any(y in p for p in pairs) and (last_y == x or any(last_y in p for p in pairs))
    check_edge(G, C, x, y, 'haantjes')
    check_edge(G, C, y, x, 'bfc')


# ---- descriptor corner cases -------------------------------------------------------------------------------------------------
def test_descriptor_corner_cases(dcr, oracle):
    # triangle nodes (inserted from both rows); y at every position of row x and x at every position of row y (4 entries each)
    seen_p, seen_q, graphs = set(), set(), []
    for seed in range(40):
        ei, n, x, y, _ = edge_graph(4, 4, n_tri=2, n_sq=1, seed=seed)
        rows = R.rows_of(ei, n)
        p, q = rows[x].index(y), rows[y].index(x)
        if p not in seen_p or q not in seen_q:
            graphs.append((ei, n, x, y))
        seen_p.add(p)
        seen_q.add(q)
    assert len(seen_p) == 4 and len(seen_q) == 4 and len(graphs) <= 8
    for ei, n, x, y in graphs:
        G, C = dcr(ei, n), oracle.CGraph(ei, n)
        assert check_both(G, C, x, y, R.KINDS) > 0
    # every neighbour of x is a neighbour of y: no row of DX, classes 1 and 2 only
    ei, n, x, y, _ = edge_graph(4, 6, n_tri=3, seed=1)
    G, C = dcr(ei, n), oracle.CGraph(ei, n)
    check_both(G, C, x, y, ('bfc', '1d'))


def test_isolated_edge_has_no_candidate_and_no_draw(dcr, oracle):
    ei = R.undirected_edge_index([(0, 1), (2, 3), (3, 4)])
    G, C = dcr(ei, 5), oracle.CGraph(ei, 5)
    assert len(check_edge(G, C, 0, 1)[0]) == 0 and len(check_edge(G, C, 1, 0)[0]) == 0
    before = G.to_edge_index().copy()
    status, n_cand, added, removed, _ = G.sdrf_iteration_device_draw(0, 1, 'bfc', 163.0, 0.5, False, 0.0)
    assert (status, n_cand, tuple(added), removed) == (2, 0, (-1, -1), None)
    assert np.array_equal(G.to_edge_index(), before)
    assert len(check_edge(G, C, 3, 2)[0]) > 0                                # the handle goes on


# ---- table walks that wrap the table's end -----------------------------------------------------------------------------------
def g_hash(key, mask):
    return ((key * 0x9E3779B1 & 0xFFFFFFFF) >> 7) & mask


def test_probe_walks_wrap_the_tables_end(dcr, oracle):
    dx, dy, n_tri = 6, 6, 1
    mask = 63                                                                # 4 (dx + dy) = 48 keys -> 64 slots
    n_want = 4000
    tail = [k for k in range(2, n_want) if g_hash(k, mask) >= 62]            # ids whose walk starts in the last two slots
    rest = [k for k in range(2, n_want) if g_hash(k, mask) < 40]
    members = dx + dy - 2 - n_tri                                            # triangle node, x's and y's private neighbours
    ids = [0, 1] + tail[:7] + rest[:members - 7]
    ei, n, x, y, big = edge_graph(dx, dy, n_tri=n_tri, n_sq=8, big_deg=400, seed=3, ids=np.array(ids))
    rows = R.rows_of(ei, n)
    keys = [k for k in dict.fromkeys(rows[x] + rows[y]) if k not in (x, y)]
    table, wrapped = {}, 0
    for k in keys:                                                           # (which walks wrap does not depend on the order)
        h = g_hash(k, mask)
        while h in table:
            h = (h + 1) & mask
        table[h] = k
        wrapped += h < g_hash(k, mask)
    assert wrapped >= 3, wrapped
    # look-ups of non-members that start at the end walk over the members there and wrap too
    assert any(g_hash(w, mask) >= 62 and w not in keys for w in rows[big])
    G, C = dcr(ei, n), oracle.CGraph(ei, n)
    assert check_both(G, C, x, y, ('bfc', 'augmented')) > 0


# ---- classes B and C after the fold ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ct', R.KINDS)
def test_class_b_and_c_values(dcr, oracle, ct):
    """The candidates with x or y as a member (class B: (x, j), class C: (i, y)) on graphs whose 4-cycle counters reach the
    runner-up and maximum-minus-one branches; 40 positions of row y span two bitmap words, so two class B workgroups."""
    reached = dict.fromkeys(('reach_sec_B', 'reach_sec_C', 'reach_dec_B', 'reach_dec_C'), 0)
    for seed, (dx, dy, n_sq) in enumerate([(5, 40, 9), (40, 5, 9), (9, 8, 6), (8, 9, 30), (12, 34, 3), (6, 6, 1), (7, 7, 2)]):
        ei, n, x, y, _ = edge_graph(dx, dy, n_tri=1, n_sq=n_sq, seed=seed)
        G, C = dcr(ei, n), oracle.CGraph(ei, n)
        adj = [set(r) for r in R.rows_of(ei, n)]
        for u, v in ((x, y), (y, x)):
            m = R.edge_model(adj, u, v)
            for k in reached:
                reached[k] += m[k]
            imp, ci, cj = check_edge(G, C, u, v, ct)
            is_b = ((ci == u) | (cj == u))
            is_c = ((ci == v) | (cj == v))
            assert is_b.sum() == len(adj[v] - adj[u] - {u}) and is_c.sum() == len(adj[u] - adj[v] - {v})
            if ct != 'bfc':   # one degree grows, one triangle appears
                d = {'1d': -1.0, 'augmented': 2.0, 'haantjes': 1.0}[ct]
                assert np.all(imp[is_b | is_c] == d) and np.all(imp[~(is_b | is_c)] == 0.0)
    assert all(v > 0 for v in reached.values()), reached


# ---- the draw ----------------------------------------------------------------------------------------------------------------
DRAW_TAU = 163.0


def _draw_setup(dcr):
    ei, n, x, y, _ = edge_graph(300, 256, n_tri=3, n_sq=3000, seed=11)
    return ei, n, x, y


def test_device_draw_equals_host_draw(dcr, monkeypatch):
    from rewiring.sdrf_no_cuda import draw_index
    ei, n, x, y = _draw_setup(dcr)
    G = dcr(ei, n)
    imp, ci, cj = G.improvements(x, y, 'bfc', want_candidates=True)
    imp, ci, cj = np.array(imp), np.array(ci), np.array(cj)
    nc = len(imp)
    L = (nc + 255) // 256
    seg = (L + 255) // 256
    assert nc > 66000 and seg >= 2
    e = np.exp(imp * DRAW_TAU)
    cdf = np.cumsum(e / e.sum())
    cdf /= cdf[-1]
    start = 100 * L + 7 * seg                       # the first element of segment 7 of block 100
    targets = [nc // 3, start, nc - 1]              # anywhere; at a segment boundary; in the last segment of the last block
    assert nc - 1 >= 255 * L and all(e[k] > 0 for k in targets)
    for k in targets:
        u = float((cdf[k - 1] + cdf[k]) / 2)
        monkeypatch.setattr(np.random, 'random_sample', lambda: u)
        want = draw_index(imp, DRAW_TAU)
        monkeypatch.undo()
        assert want == k
        H = dcr(ei, n)
        status, n_cand, added, removed, _ = H.sdrf_iteration_device_draw(x, y, 'bfc', DRAW_TAU, u, False, 0.0)
        assert (status, n_cand) == (0, nc), (k, status)
        assert tuple(added) == (int(ci[want]), int(cj[want])), (k, added)
        assert H.number_of_edges() == ei.shape[1] // 2 + 1 and H.has_edge(*added)


def test_wide_margin_leaves_every_draw_undecided(dcr, monkeypatch):
    ei, n, x, y = _draw_setup(dcr)
    G = dcr(ei, n)
    before = G.to_edge_index().copy()
    monkeypatch.setenv('DCR_DRAW_MARGIN_SCALE', '1e30')
    for u in (0.0, 0.25, 0.5, 0.999):
        status, n_cand, added, removed, _ = G.sdrf_iteration_device_draw(x, y, 'bfc', DRAW_TAU, u, False, 0.0)
        assert status == 1 and n_cand > 66000 and tuple(added) == (-1, -1) and removed is None, (u, status)
    assert np.array_equal(G.to_edge_index(), before)


# ---- iterations back to back on one graph ------------------------------------------------------------------------------------
def test_iterations_back_to_back_carry_nothing_over(dcr, oracle):
    """A large edge, a small one whose rows and table are shorter (stale descriptors and slots of the large one lie behind
    them), the large one the other way round, the small one again: each equal to the oracle."""
    ei_a, n_a, xa, ya, _ = edge_graph(300, 70, n_tri=4, n_sq=500, seed=5)
    ei_b, n_b, xb, yb, _ = edge_graph(5, 9, n_tri=2, n_sq=4, seed=6)
    ei, n = R.disjoint_union(ei_a, n_a, ei_b, n_b)
    xb, yb = xb + n_a, yb + n_a
    G, C = dcr(ei, n), oracle.CGraph(ei, n)
    for x, y in ((xa, ya), (xb, yb), (ya, xa), (yb, xb), (xb, yb), (xa, ya)):
        assert len(check_edge(G, C, x, y)[0]) > 0
