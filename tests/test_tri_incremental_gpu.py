"""Incremental passes of the two triangle curvatures ('augmented': 4 - du - dv + 3 T, 'haantjes': T) behind real edits, on
every route a pass can take, against two references: the C oracle (oracle/c_oracle.py) and the numpy restatement tests/tri_ref.py.

Every pass kernel is compiled twice, MODE_BFC and MODE_TRI; the two differ in the closing expression and in who owns an edge
(nc_owns takes the kind: Balanced Forman's "an endpoint of degree 1 -> 0.0" shortcut does not exist for the triangle kinds, where
such an edge is worth 4 - du - 1 or 0).  An incremental pass recomputes only what a dirty flag reaches, so a mistake in
ownership or in the dirty test under MODE_TRI leaves a stale value in place: nothing faults, the buffer is just wrong.  Every
comparison here is np.array_equal on the edge lists and on the bits of the whole curvature buffer (all values are integers);
where the route is the point, the engine the library reports and the route dcr_pass_plan gives for the graph's facts are
asserted as well, so that no case passes by taking another path."""
import os
import re

import numpy as np
import pytest

import tri_ref
from conftest import PKG
from pass_mirror import EDGE_CENTRIC, KINDS, NC_CLASSES, NC_EDGES, Mirror

pytestmark = pytest.mark.gpu



def _source(name):
    with open(os.path.join(PKG, 'csrc', name)) as f:
        return f.read()


def _limits():
    """(nc_maxdeg(0..3), NC_MAXD, DIRTY_EDITS) as the sources spell them."""
    route = _source('dcr_pass_route.h')
    nc_maxd = int(re.search(r'constexpr\s+int\s+NC_MAXD\s*=\s*(\d+)\s*;', route).group(1))
    dirty_edits = int(re.search(r'constexpr\s+int\s+DIRTY_EDITS\s*=\s*(\d+)\s*;', route).group(1))
    m = re.search(r'nc_maxdeg\(int c\)\s*\{\s*return c == 0 \? (\d+) : c == 1 \? (\d+) : c == 2 \? (\d+) : c == 3 \? (\d+) : NC_MAXD;',
                  _source('dcr_bfc_nc.hip'))
    assert m, 'nc_maxdeg not found'
    return tuple(int(x) for x in m.groups()), nc_maxd, dirty_edits


CLASS_LIMITS, NC_MAXD, DIRTY_EDITS = _limits()


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


@pytest.fixture(scope='module')
def oracle():
    from oracle import c_oracle
    return c_oracle


def other_kind(ct):
    return KINDS[1 - KINDS.index(ct)]


def _random_edits(M, rng, count):
    done = 0
    while done < count:
        u, v = (int(t) for t in rng.integers(0, M.n, 2))
        if u != v:
            M.toggle(u, v)
            done += 1


# ------------------------------------------------------------------------------------------------ 1 and 5: routes
@pytest.mark.parametrize('ct', KINDS)
@pytest.mark.parametrize('route,every', [('edges', 3), ('rows', 3), ('classes', 3), ('edges', 7), ('edge-centric', 3)])
def test_incremental_routes_behind_random_edits(dcr, oracle, monkeypatch, route, every, ct):
    """test_gpu_parity.py::test_incremental_pass_equals_full (power-law 800 x 5, 40 random additions and removals; here ten of
    them hang an isolated node on the graph) with the first pass and every incremental pass of a triangle kind: behind at most DIRTY_EDITS edits (exact flags) edge by edge, the list from a sweep (k_nc_fine_list) or from the flagged
    nodes' rows (k_nc_fine_list_rows), or — DCR_NC_FINE=0 — by the class kernels; behind more edits (coarse flags) by the class
    kernels; under DCR_PASS=edge by the edge-centric kernels.  Then the other triangle kind, Balanced Forman and the first kind
    again, each asked for incrementally on top of the previous kind's buffer (with edits pending): none may reuse it."""
    from dcr import synthetic
    monkeypatch.setenv('DCR_NC_FINE', '0' if route == 'classes' else '1')
    monkeypatch.setenv('DCR_NC_FINE_SWEEP', '0' if route == 'rows' else '1')
    ei, nn = synthetic.powerlaw_graph(800, 5, seed=13)
    spare = list(range(nn, nn + 10))                     # isolated: every fourth edit hangs one of them on the graph, so that
    nn += len(spare)                                     # each route also meets edges with an endpoint of degree 1
    M = Mirror(dcr, oracle, ei, nn, monkeypatch, 'edge' if route == 'edge-centric' else None)
    M.run(ct, incremental=False, label='first')
    rng = np.random.Generator(np.random.PCG64(17))
    taken = []
    for step in range(40):
        u, v = (int(t) for t in rng.integers(0, nn, 2))
        if step % 4 == 2:
            u = spare[step // 4]
        if u == v:
            continue
        M.toggle(u, v)
        if step % every == 0:
            exact = M.pending <= DIRTY_EDITS
            if route == 'edge-centric':
                want = (EDGE_CENTRIC, False, False)
            elif route != 'classes' and exact:
                want = (NC_EDGES, route == 'rows', False)
            else:
                want = (NC_CLASSES, False, False)
            M.run(ct, True, want, ('step', step, route))
            taken.append((want[0], exact))
    # the route this case is about was taken, and not once
    if route == 'edge-centric':
        assert taken.count((EDGE_CENTRIC, True)) >= 10
    elif every == 7:
        assert taken.count((NC_CLASSES, False)) >= 4
    elif route == 'classes':
        assert taken.count((NC_CLASSES, True)) >= 10
    else:
        assert taken.count((NC_EDGES, True)) >= 10
    if every == 7:
        assert M.pending > 0                             # the switch of kind below finds edits pending
    M.run(other_kind(ct), True, label='other triangle kind')
    _random_edits(M, rng, 2)
    M.run('bfc', True, label='bfc behind a triangle kind')
    _random_edits(M, rng, 2)
    M.run(ct, True, label='triangle kind behind bfc')
    _random_edits(M, rng, 2)
    M.run(ct, True, (EDGE_CENTRIC, False, False) if route == 'edge-centric' else
          (NC_CLASSES, False, False) if route == 'classes' else (NC_EDGES, route == 'rows', False), label='incremental again')


# ------------------------------------------------------------------------------------------------ 2: degree one, ownership
@pytest.mark.parametrize('ct', KINDS)
@pytest.mark.parametrize('route', ['edges', 'rows'])
def test_degree_one_and_ownership_edges(dcr, oracle, monkeypatch, route, ct):
    """A star of 70 leaves, a path, two triangles sharing an edge and isolated nodes, each tied to a small body; one edit per
    incremental pass (exact flags, edge by edge): (a) two leaves of the star joined — a triangle at two endpoints going from
    degree 1 to 2; (b) that edge removed; (c) a fresh leaf attached to a leaf, the degree-1 endpoint once the larger id, once
    the smaller; (d) the shared edge of the two triangles removed; (e) an isolated node's first edge.  Under MODE_TRI an edge
    with a degree-1 endpoint is 4 - du - 1 ('augmented') or 0 ('haantjes') and is owned by its higher-degree endpoint; Balanced
    Forman's rule (0.0, owned by the smaller id) must not leak in."""
    from dcr import synthetic
    monkeypatch.setenv('DCR_NC_FINE_SWEEP', '0' if route == 'rows' else '1')
    body, nb = synthetic.powerlaw_graph(60, 3, seed=3)
    low, centre, leaves, path = 0, 61, list(range(62, 132)), list(range(132, 138))
    a, b, c, d, lonely, high, n = 138, 139, 140, 141, 142, 143, 144
    src = (body[0] + 1).tolist() + [centre] + [centre] * 70 + path[1:] + [path[0]] + [a, a, b, a, b] + [a]
    dst = (body[1] + 1).tolist() + [1] + leaves + path[:-1] + [2] + [b, c, c, d, d] + [3]
    ei = synthetic.coalesced_edge_index(np.array(src), np.array(dst), n)
    M = Mirror(dcr, oracle, ei, n)
    assert [M.C.degree(k) for k in (low, lonely, high, leaves[0], path[-1], centre)] == [0, 0, 0, 1, 1, 71]
    M.run(ct, incremental=False, label='first')
    want = (NC_EDGES, route == 'rows', False)

    def value(u, v):
        return M.C.curv_edge(u, v, ct)

    assert value(centre, leaves[5]) == (4 - 71 - 1 if ct == 'augmented' else 0)      # not Balanced Forman's 0.0
    assert value(a, b) == (4 - 4 - 3 + 3 * 2 if ct == 'augmented' else 2)
    M.add(leaves[0], leaves[1])
    M.run(ct, True, want, 'a: two leaves joined')
    assert value(leaves[0], leaves[1]) == (4 - 2 - 2 + 3 if ct == 'augmented' else 1)
    M.remove(leaves[0], leaves[1])
    M.run(ct, True, want, 'b: and parted')
    M.add(leaves[2], high)
    M.run(ct, True, want, 'c: leaf on a leaf, degree 1 at the larger id')
    assert value(leaves[2], high) == (4 - 2 - 1 if ct == 'augmented' else 0)
    M.add(leaves[3], low)
    M.run(ct, True, want, 'c: leaf on a leaf, degree 1 at the smaller id')
    assert value(low, leaves[3]) == (4 - 1 - 2 if ct == 'augmented' else 0)
    M.remove(a, b)
    M.run(ct, True, want, 'd: shared edge of two triangles removed')
    assert value(a, c) == (4 - 3 - 2 if ct == 'augmented' else 0)
    M.add(lonely, 5)
    M.run(ct, True, want, 'e: first edge of an isolated node')
    M.remove(leaves[2], high)                         # and back to an isolated node, its neighbour a leaf again
    M.run(ct, True, want, 'f: last edge of a node removed')


# ------------------------------------------------------------------------------------------------ 3: every class, dirty flags
@pytest.mark.parametrize('ct', KINDS)
def test_every_node_centric_class_under_dirty_flags(dcr, oracle, monkeypatch, ct):
    """One hub per node-centric class: nc_maxdeg(c) - 1 neighbours for c = 0..3 and 4,300 for class 4, the hubs adjacent to
    each other, with shared leaves and leaf-leaf edges (built as test_hubs_at_and_beyond_node_centric_limits builds its graph).
    (a) each hub is moved onto and across its class limit, an incremental pass behind each edit (exact flags, edge by edge);
    (b) five edits among hubs and leaves, one pass (coarse flags: the class kernels, every class launched); (c) DCR_NC_FINE=0:
    two edits and a pass (exact flags through the class kernels), then five edits and a pass; (d) a hub-hub edge removed and
    added back with a pass in between."""
    from dcr import synthetic
    n = 9000
    degrees = [CLASS_LIMITS[0] - 1, CLASS_LIMITS[1] - 1, CLASS_LIMITS[2] - 1, CLASS_LIMITS[3] - 1, 4300]
    assert degrees == [61, 253, 1021, 4093, 4300] and degrees[4] <= NC_MAXD
    rng = np.random.Generator(np.random.PCG64(99))
    src, dst = [], []
    for hub, d in enumerate(degrees):
        leaves = rng.choice(np.arange(5, n), size=d - 4, replace=False)          # + the four other hubs
        src += [hub] * len(leaves); dst += leaves.tolist()
        src += [hub] * (4 - hub); dst += list(range(hub + 1, 5))
    extra = rng.integers(5, n, size=(2, 6000))                                   # leaf-leaf edges
    src += extra[0].tolist(); dst += extra[1].tolist()
    ei = synthetic.coalesced_edge_index(np.array(src), np.array(dst), n)
    M = Mirror(dcr, oracle, ei, n)
    assert [M.G.degree(h) for h in range(5)] == degrees
    M.run(ct, incremental=False, label='first')
    fine, coarse = (NC_EDGES, False, False), (NC_CLASSES, False, False)
    # (a)
    for hub in range(4):
        for step in (0, 1):
            M.add(hub, M.free_leaf(hub, 5))
            M.run(ct, True, fine, ('a', hub, step))
        assert M.G.degree(hub) == CLASS_LIMITS[hub] + 1
    # (b) and (c)
    def five_edits(k):
        leaf4 = next(v for v in M.G.neighbors(4) if v >= 5)
        M.add(0, M.free_leaf(0, 100 + k))
        M.remove(4, leaf4)
        M.add(2, M.free_leaf(2, 200 + k))
        e = next((int(x), int(y)) for x, y in extra.T[k:] if x != y and M.C.has_edge(int(x), int(y)))
        M.remove(*e)
        M.add(leaf4, M.free_leaf(leaf4, 300 + k, forbid=(4,)))
    five_edits(0)
    assert M.pending == 5 > DIRTY_EDITS
    M.run(ct, True, coarse, 'b: coarse flags')
    monkeypatch.setenv('DCR_NC_FINE', '0')
    M.add(1, M.free_leaf(1, 400))
    M.remove(3, next(v for v in M.G.neighbors(3) if v >= 5))
    assert M.pending == 2 <= DIRTY_EDITS
    M.run(ct, True, coarse, 'c: exact flags, class kernels')
    five_edits(50)
    M.run(ct, True, coarse, 'c: coarse flags, class kernels')
    monkeypatch.delenv('DCR_NC_FINE')
    # (d)
    for x, y in ((3, 4), (0, 2)):
        M.remove(x, y)
        M.run(ct, True, fine, ('d: hub-hub edge removed', x, y))
        M.add(x, y)
        M.run(ct, True, fine, ('d: and added back', x, y))


# ------------------------------------------------------------------------------------------------ 4: beyond the tables
def _three_hubs(n, da, db, dc):
    """The graph of test_gpu_parity.py::test_hubs_at_and_beyond_node_centric_limits."""
    from dcr import synthetic
    rng = np.random.Generator(np.random.PCG64(99))
    src, dst = [0], [1]
    a = rng.choice(np.arange(3, n), size=da, replace=False)
    b = rng.choice(np.arange(3, n), size=db, replace=False)
    c = rng.choice(np.arange(3, n), size=dc, replace=False)
    for hub, leaves in ((0, a), (1, b), (2, c)):
        src += [hub] * len(leaves); dst += leaves.tolist()
    src += [0, 1]; dst += [2, 2]
    extra = rng.integers(3, n, size=(2, 6000))
    src += extra[0].tolist(); dst += extra[1].tolist()
    return synthetic.coalesced_edge_index(np.array(src), np.array(dst), n), n


def _four_giant_hubs():
    """The graph of test_gpu_parity.py::test_edges_beyond_every_lds_table."""
    from dcr import synthetic
    n = 40000
    rng = np.random.Generator(np.random.PCG64(21))
    src, dst = [], []
    for hub, d in ((0, 12000), (1, 11000), (2, 17000), (3, 9000)):
        leaves = rng.choice(np.arange(10, n), size=d, replace=False)
        src += [hub] * d; dst += leaves.tolist()
    for a in range(4):
        for b in range(a + 1, 4):
            src.append(a); dst.append(b)
    extra = rng.integers(10, n, size=(2, 30000))
    src += extra[0].tolist(); dst += extra[1].tolist()
    return synthetic.coalesced_edge_index(np.array(src), np.array(dst), n), n


@pytest.mark.parametrize('ct', KINDS)
@pytest.mark.parametrize('shape', ['hub_above_nc_maxd', 'beyond_every_lds_table'])
def test_hubs_beyond_the_node_centric_tables(dcr, oracle, shape, ct):
    """A hub above NC_MAXD (its edges owned by the other endpoint, hub 1 at the largest class's limit) and hubs whose joint
    degrees exceed every LDS table (csrc/dcr_bfc_giant.hip): the node-centric pass is followed by the hub supplement —
    run_pass<MODE_TRI>(incremental, nc_rest) and process_hub_edges — on the full pass and behind each edit: the hub-hub edge
    removed, added back, and a fresh leaf on the largest hub."""
    if shape == 'hub_above_nc_maxd':
        (ei, n), giant, first_leaf = _three_hubs(18000, 8195, 8180, 6000), 0, 3
    else:
        (ei, n), giant, first_leaf = _four_giant_hubs(), 2, 10
    M = Mirror(dcr, oracle, ei, n)
    if shape == 'hub_above_nc_maxd':
        assert M.G.degree(0) > NC_MAXD >= M.G.degree(1) > NC_MAXD - 30
    else:
        assert M.G.degree(0) + M.G.degree(1) + 2 > 16384 and M.G.degree(2) > 16382
    plan = M.run(ct, incremental=False, label='full')
    assert plan[0] in (NC_CLASSES, NC_EDGES) and plan[2]
    want = (NC_EDGES, False, True)
    M.remove(0, 1)
    M.run(ct, True, want, 'hub-hub edge removed')
    M.add(0, 1)
    M.run(ct, True, want, 'hub-hub edge added back')
    M.add(giant, M.free_leaf(giant, first_leaf))
    M.run(ct, True, want, 'fresh leaf on the largest hub')


# ------------------------------------------------------------------------------------------------ 6: fused tail and arg-min
def _first(values, want_max):
    return int(np.argmax(values)) if want_max else int(np.argmin(values))


def _graph_with_tied_minima():
    """Power-law 250 x 3 and six pairs of adjacent hubs, every hub with the same degree (above any of the body's) and leaves of
    its own: six edges share the lowest 'augmented' value, more than a thousand the lowest 'haantjes' value (0)."""
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(250, 3, seed=8)
    D = int(np.bincount(ei[0], minlength=n).max()) + 5
    keep = ei[0] > ei[1]
    src, dst = ei[0][keep].tolist(), ei[1][keep].tolist()
    nxt = n
    for i in range(6):
        a, b = nxt, nxt + 1
        nxt += 2
        src += [b, a]; dst += [a, i]                                             # the pair, and a tie to the body
        for hub, leaves in ((a, D - 2), (b, D - 1)):
            src += list(range(nxt, nxt + leaves)); dst += [hub] * leaves
            nxt += leaves
    return synthetic.coalesced_edge_index(np.array(src), np.array(dst), nxt), nxt


@pytest.mark.parametrize('ct,bound', [('augmented', -2.5), ('haantjes', 10.0)])
@pytest.mark.parametrize('incremental', [False, True])
def test_fused_tail_next_pass_and_argmin(dcr, oracle, incremental, ct, bound):
    """dcr_sdrf_tail_at_pass_argmin with a triangle kind (test_fused_tail_and_next_pass_including_row_overflow, driven call
    by call): the add, the removal of the stale first maximum above the bound, the next pass — incremental: the flags of the
    two edits, cleared by the sweep for the extrema — and the first minimum, 140 times, long enough for rows to overflow and be
    laid out again.  After every call: the edits, the returned arg-min (the oracle's FIRST minimum in G.edges() order — the
    values are integers and tie massively), the whole buffer, and argext's first maximum."""
    ei, n = _graph_with_tied_minima()
    G, C = dcr(ei, n), oracle.CGraph(ei, n)
    deg0 = np.bincount(ei[0], minlength=n)
    x, y, val = G.curvature_pass_argmin(ct, incremental=incremental)
    ou, ov, oc = C.curv_all(ct, nthreads=4)
    assert int((oc == oc.min()).sum()) >= (6 if ct == 'augmented' else 1000)     # the tie rule decides
    k = _first(oc, False)
    assert (x, y, val) == (int(ou[k]), int(ov[k]), float(oc[k]))
    tied = removals = 0
    for it in range(140):
        imp, ci, cj = G.improvements(x, y, ct, want_candidates=True)
        oi, oj = C.candidates(x, y)
        assert np.array_equal(ci, oi) and np.array_equal(cj, oj), it
        want_imp = C.improvements(x, y, oi, oj, ct)
        assert np.array_equal(np.array(imp), want_imp), it
        # an edge at x where there is one (x's row keeps growing: it overflows), else the first best improvement
        idx = next((j for j in range(len(oi)) if x in (int(oi[j]), int(oj[j]))), int(np.argmax(want_imp)))
        pair = (int(oi[idx]), int(oj[idx]))
        added, removed, (mu, mv, mval) = G.sdrf_tail_at_pass_argmin(idx, True, bound, ct, incremental=incremental)
        assert G.pass_engine() == 'node-centric'
        C.add_edge(*pair)
        top = _first(oc, True)                            # stale values, the new edge has none (sdrf_no_cuda.py:57-61)
        want_removed = (int(ou[top]), int(ov[top])) if oc[top] > bound else None
        if want_removed:
            C.remove_edge(*want_removed)
            removals += 1
        assert tuple(sorted(added)) == tuple(sorted(pair)), it
        assert (None if removed is None else tuple(sorted(removed))) == want_removed, it
        ou, ov, oc = C.curv_all(ct, nthreads=4)
        ru, rv, rc = G.curvature_read()
        assert np.array_equal(ru, ou) and np.array_equal(rv, ov), it
        bad = np.flatnonzero(rc.view(np.int64) != oc.view(np.int64))
        assert bad.size == 0, (it, pair, want_removed, [(int(ru[i]), int(rv[i]), C.degree(int(ru[i])), C.degree(int(rv[i])),
                                                         float(rc[i]), float(oc[i])) for i in bad[:6]])
        k = _first(oc, False)
        assert (mu, mv, mval) == (int(ou[k]), int(ov[k]), float(oc[k])), it
        tied += int((oc == oc.min()).sum()) >= 3
        k = _first(oc, True)
        assert G.argext(True) == (int(ou[k]), int(ov[k]), float(oc[k])), it
        x, y = mu, mv
    tu, tv, tc = tri_ref.curv_all(C.to_edge_index(), n, ct, rows=True)
    assert np.array_equal(tu, ou) and np.array_equal(tv, ov) and np.array_equal(tc.view(np.int64), oc.view(np.int64))
    deg = np.array([C.degree(u) for u in range(n)])
    assert np.any(deg > deg0 + np.maximum(8, deg0 // 4))                         # some row outgrew its slack: laid out again
    assert tied >= 50 and removals >= 5 and 140 - removals >= 5


@pytest.mark.parametrize('ct', KINDS)
@pytest.mark.parametrize('incremental', [False, True])
def test_fused_tail_replay_across_a_degree_class(dcr, oracle, monkeypatch, incremental, ct):
    """test_fused_tail_replay_when_the_add_crosses_a_degree_class at (d0, limit) = (50, 62) with a triangle kind: the hub sits at
    the largest degree of class 0 with its row full, the add inside dcr_sdrf_tail_at_pass_argmin overflows, the call lays the
    rows out again, replays the tail and redoes the pass with the hub in class 1.  Five of the hub's neighbours are given the
    same degree, above every other's, and no triangle with the hub, so that the lowest 'augmented' value is shared."""
    d0, limit = 50, CLASS_LIMITS[0]
    assert limit == 62
    monkeypatch.setenv('DCR_PASS', 'nc')
    rng = np.random.Generator(np.random.PCG64(d0))
    n = 4 * limit + 200
    a = rng.integers(1, n, size=3 * n)
    b = rng.integers(1, n, size=3 * n)
    nbr = [set() for _ in range(n)]
    for u, v in zip(a.tolist(), b.tolist()):
        if u != v:
            nbr[u].add(v); nbr[v].add(u)
    hub_side = set(range(1, limit + 1))                   # the hub's neighbours once its row is full
    tied = [v for v in range(1, d0 + 1) if not nbr[v] & hub_side][:5]
    assert len(tied) == 5
    for v in range(1, d0 + 1):
        nbr[v].add(0)
    top = max(len(s) for s in nbr) + 2                    # (+ 2: the hub's later neighbours d0 + 1 .. limit stay below it too)
    far = iter(range(limit + 1, n))
    src, dst = [0] * d0 + a.tolist(), list(range(1, d0 + 1)) + b.tolist()
    for v in tied:
        while len(nbr[v]) < top:
            w = next(far)
            if w not in nbr[v] and len(nbr[w]) < top - 1:
                nbr[v].add(w); nbr[w].add(v)
                src.append(v); dst.append(w)
    from dcr import synthetic
    ei = synthetic.coalesced_edge_index(np.array(src), np.array(dst), n)
    G = dcr(ei, n)
    C = oracle.CGraph(ei, n)
    assert G.degree(0) == d0 and max(G.degree(u) for u in range(1, n)) == top < limit
    for w in range(d0 + 1, limit + 1):                    # capacity d0 + max(8, d0 // 4) == limit: the row is now full
        G.add_edge(0, w)
        C.add_edge(0, w)
    assert G.degree(0) == limit
    G.curvature_pass(ct)
    assert G.pass_engine() == 'node-centric'
    y = next(v for v in G.neighbors(0) if any(not G.has_edge(0, j) and j != 0 for j in G.neighbors(v)))
    for attempt in (0, 1):                                # the add that crosses the class, then one into the fresh slack
        imp, ci, cj = G.improvements(0, y, ct, want_candidates=True)
        idx = next(k for k in range(len(ci)) if 0 in (int(ci[k]), int(cj[k])))
        pair = (int(ci[idx]), int(cj[idx]))
        added, removed, (mu, mv, mval) = G.sdrf_tail_at_pass_argmin(idx, False, 0.0, ct, incremental=incremental)
        assert tuple(added) == pair and removed is None and G.degree(0) == limit + 1 + attempt
        assert G.pass_engine() == 'node-centric'
        C.add_edge(*pair)
        ou, ov, oc = C.curv_all(ct, nthreads=4)
        ru, rv, rc = G.curvature_read()
        assert np.array_equal(ru, ou) and np.array_equal(rv, ov)
        bad = np.flatnonzero(rc.view(np.int64) != oc.view(np.int64))
        assert bad.size == 0, (attempt, [(int(ru[i]), int(rv[i]), C.degree(int(ru[i])), C.degree(int(rv[i])), float(rc[i]),
                                          float(oc[i])) for i in bad[:6]])
        tu, tv, tc = tri_ref.curv_all(C.to_edge_index(), n, ct, rows=True)
        assert np.array_equal(tu, ou) and np.array_equal(tv, ov) and np.array_equal(tc.view(np.int64), oc.view(np.int64))
        assert int((oc == oc.min()).sum()) >= 3, attempt  # the minimum is shared: the first in G.edges() order is wanted
        k = _first(oc, False)
        assert (mu, mv, mval) == (int(ou[k]), int(ov[k]), float(oc[k])), attempt
        k = _first(oc, True)
        assert G.argext(True) == (int(ou[k]), int(ov[k]), float(oc[k])), attempt


# ------------------------------------------------------------------------------------------------ 7: SDRF end to end
def _replay(oracle, ei, n, trace):
    """The oracle's graph behind the traced edits: adjacency rows, and so G.edges() order, as the run left them."""
    C = oracle.CGraph(ei, n)
    for rec in trace:
        if rec['added']:
            C.add_edge(*rec['added'])
        if rec['removed']:
            C.remove_edge(*rec['removed'])
    return C


# removal bounds taken once from the oracle's own runs below (numpy seed 4, tau 2): 11 / 17 of the 40 iterations remove an edge
@pytest.mark.parametrize('ct,bound', [('augmented', -6.5), ('haantjes', 12.0)])
def test_sdrf_incremental_end_to_end(oracle, ct, bound):
    """sdrf_no_cuda(..., ct, loops=40, remove_edges=True, incremental=True) on power-law 1500 x 6 against oracle.sdrf with the
    same numpy seed and against the incremental=False run: the final edge index, and the final curvature buffer (one more pass
    of the run's own kind, incremental where the run was) against the oracle's values on its own final graph."""
    from dcr import synthetic
    from dcr.data import Data
    from rewiring.sdrf_no_cuda import SdrfRun, sdrf_no_cuda
    import torch
    ei, n = synthetic.powerlaw_graph(1500, 6, seed=5)
    loops, tau = 40, 2.0
    trace = []
    np.random.seed(4)
    want = oracle.sdrf(ei, n, ct, loops, True, bound, tau, trace=trace, nthreads=8)
    removed = sum(rec['removed'] is not None for rec in trace)
    assert len(trace) == loops and removed >= 5 and loops - removed >= 5, removed
    C = _replay(oracle, ei, n, trace)
    assert np.array_equal(C.to_edge_index(), want)
    ou, ov, oc = C.curv_all(ct, nthreads=8)
    tu, tv, tc = tri_ref.curv_all(want, n, ct, rows=True)
    assert np.array_equal(tu, ou) and np.array_equal(tv, ov) and np.array_equal(tc.view(np.int64), oc.view(np.int64))
    data = Data(edge_index=torch.from_numpy(ei), num_nodes=n)
    np.random.seed(4)
    got = sdrf_no_cuda(data, ct, loops, True, bound, tau, incremental=True)
    assert np.array_equal(got.edge_index.numpy(), want)
    for inc in (False, True):                             # the same loop, the handle kept for its buffer
        np.random.seed(4)
        run = SdrfRun(data, ct, True, bound, tau, incremental=inc)
        for i in range(loops):
            assert run.step(more=i + 1 < loops)
        assert np.array_equal(run.G.to_edge_index(), want), inc
        run.G.curvature_pass(ct, incremental=inc)
        assert run.G.pass_engine() == 'node-centric'
        ru, rv, rc = run.G.curvature_read()
        assert np.array_equal(ru, ou) and np.array_equal(rv, ov), inc
        bad = np.flatnonzero(rc.view(np.int64) != oc.view(np.int64))
        assert bad.size == 0, (inc, int(bad.size), [(int(ru[i]), int(rv[i]), C.degree(int(ru[i])), C.degree(int(rv[i])),
                                                     float(rc[i]), float(oc[i])) for i in bad[:6]])
