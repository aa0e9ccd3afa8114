"""The edit kernels of the graph container (csrc/dcr_graph.hip) against the host model of tests/graph_model.py, with the edits
placed where the kernels' loops change behaviour: the 64-wide steps of wave_find, wave_erase and k_relayout, the 64- and 256-wide
walks of dev_weight_edit and dev_mark_dirty, and the last slot of a row's slack.  No tolerances: integers and float64 bit
patterns.  The model's own rules are held against networkx, and its shapes shown to bite, in tests/test_graph_model_cpu.py.

After an edit the values of the last pass are compared for the edges that existed at that pass only: an added edge has no
defined value (graph_model.py says why), and the extrema are checked over what curvature_read returns for those."""
import numpy as np
import pytest

import graph_model as gm
from graph_model import GraphModel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


@pytest.fixture(scope='module')
def oracle():
    from oracle import c_oracle
    return c_oracle


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def check(G, M, nodes, pair, absent, what=None):
    """The handle against the model after an edit."""
    for x in nodes:
        assert G.degree(x) == M.degree(x), (what, x)
        assert G.neighbors(x) == M.neighbors(x), (what, x)
    u, v = pair
    assert G.has_edge(u, v) == G.has_edge(v, u) == M.has_edge(u, v), (what, pair)
    assert not G.has_edge(*absent) and not G.has_edge(absent[1], absent[0]) and not M.has_edge(*absent), (what, absent)
    assert G.number_of_edges() == M.number_of_edges(), what
    mu, mv, mc, known = M.values()
    eu, ev = G.edges()
    assert np.array_equal(eu, mu) and np.array_equal(ev, mv), what
    assert np.array_equal(G.to_edge_index(), M.to_edge_index()), what
    if not M.has_values:
        return
    ru, rv, rc = G.curvature_read()
    assert np.array_equal(ru, mu) and np.array_equal(rv, mv), what
    bad = np.flatnonzero(known & (bits(rc) != bits(mc)))      # edge by edge: the two lists are in the same order
    assert bad.size == 0, (what, bad.size, [(int(ru[i]), int(rv[i]), rc[i], mc[i]) for i in bad[:5]])
    if rc.size:
        for want_max, k in ((True, int(np.argmax(rc))), (False, int(np.argmin(rc)))):
            a, b, val = G.argext(want_max)
            assert (a, b) == (int(ru[k]), int(rv[k])) and bits(val) == bits(rc[k]), (what, want_max)


def run_pass(G, M, incremental=False):
    G.curvature_pass('bfc', incremental=incremental)
    M.set_values(*G.curvature_read())


def value_dict(G):
    eu, ev, cv = G.curvature_read()
    return {(int(a), int(b)): int(c) for a, b, c in zip(eu, ev, bits(cv))}


def incremental_equals_fresh_full(G, M, dcr, what=None):
    """An incremental pass of the edited handle against a full pass of a fresh handle of the same graph, edge by edge."""
    G.curvature_pass('bfc', incremental=True)
    F = dcr(M.to_edge_index(), M.n)
    F.curvature_pass('bfc')
    got, want = value_dict(G), value_dict(F)
    assert got.keys() == want.keys(), what
    bad = [(k, got[k], want[k]) for k in want if got[k] != want[k]]
    assert not bad, (what, len(bad), bad[:6])
    M.set_values(*G.curvature_read())


def hub_values(G, hub):
    eu, ev, cv = G.curvature_read()
    return cv[(eu == hub) | (ev == hub)]


# ---------------------------------------------------------------------------------------------------------------- case 1
@pytest.mark.parametrize('d', gm.ERASE_D)
def test_erase_at_the_stride_edges_through_remove_edge(dcr, oracle, d):
    """k_remove_edge: the hub edge at every listed position of a ladder hub's row, a fresh handle each; the leaf's own row holds
    the hub first, in the middle or last.  The hub edges' values are pairwise distinct, so a value that moved with the wrong
    edge shows."""
    for k, p in enumerate(gm.erase_positions(d)):
        ei, n, hub, leaf, p, lp = gm.erase_shape(d, k)
        G, M = dcr(ei, n), GraphModel(ei, n)
        assert M.neighbors(hub).index(leaf) == p and M.neighbors(leaf).index(hub) == lp
        run_pass(G, M)
        hv = hub_values(G, hub)
        assert hv.size == d and np.unique(bits(hv)).size == d
        if k == 0:
            ou, ov, oc = oracle.CGraph(ei, n).curv_all('bfc', nthreads=4)
            ru, rv, rc = G.curvature_read()
            assert np.array_equal(ru, ou) and np.array_equal(rv, ov) and np.array_equal(bits(rc), bits(oc))
        a, b = (hub, leaf) if k % 2 == 0 else (leaf, hub)
        G.remove_edge(a, b)
        M.remove_edge(a, b)
        check(G, M, [hub, leaf], (hub, leaf), (hub, n - 1), (d, p))


@pytest.mark.parametrize('d', gm.ERASE_D)
def test_erase_at_the_stride_edges_through_the_tail(dcr, oracle, d):
    """The removal inside k_sdrf_tail: the tail removes the stale arg-max, so the pendant edges (which outrank every hub edge) are
    removed first, one by one, and the hub row is ordered so that each arg-max in turn sits at a wanted position
    (graph_model.tail_erase_plan).  improvements() leaves the stale arg-max in the result block, which is what makes the next
    sdrf_tail the single launch; the tail's add goes between two nodes that never had an edge."""
    order, probes = gm.tail_erase_plan(d)
    P = gm.Parts()
    hub, leaf, pend = gm.add_ladder_hub(P, d, hub_order=order)
    q1, q2 = P.nodes(2)
    ei, n = P.edge_index(), P.n
    G, M = dcr(ei, n), GraphModel(ei, n)
    run_pass(G, M)
    ou, ov, oc = oracle.CGraph(ei, n).curv_all('bfc', nthreads=4)
    ru, rv, rc = G.curvature_read()
    assert np.array_equal(ru, ou) and np.array_equal(rv, ov) and np.array_equal(bits(rc), bits(oc))
    hv = hub_values(G, hub)
    assert hv.size == d and np.unique(bits(hv)).size == d
    for i in range(1, d + 1):
        for q in pend[i]:
            G.remove_edge(leaf[i], q)
            M.remove_edge(leaf[i], q)
    check(G, M, [hub, leaf[1], leaf[d]], (hub, leaf[d]), (leaf[1], pend[1][0]), (d, 'pendants gone'))
    for k, (p, length) in enumerate(probes):
        target = leaf[k + 1]
        assert M.degree(hub) == length and M.neighbors(hub).index(target) == p
        imp, _, _ = G.improvements(hub, leaf[d], 'bfc')
        assert imp.shape[0] > 0
        removed, mx = G.sdrf_tail((q1, q2), True, -10.0)
        want_removed, want_mx = M.sdrf_tail((q1, q2), True, -10.0)
        assert want_removed == (hub, target)
        assert removed == want_removed and bits(mx) == bits(want_mx), (d, p, length)
        G.remove_edge(q2, q1)
        M.remove_edge(q2, q1)
        check(G, M, [hub, target, q1, q2], (hub, target), (q1, q2), (d, p, length))


# ---------------------------------------------------------------------------------------------------------------- case 2
@pytest.mark.parametrize('q', gm.FIND_POS)
def test_find_beyond_the_first_stride(dcr, q):
    """wave_find of k_has_edge, dev_add_edge and dev_remove_edge with the match at position q of the shorter row: adding the
    edge again, in either order, returns 'already there' and changes nothing."""
    ei, n, s, t, spare = gm.find_shape(q, True)
    G, M = dcr(ei, n), GraphModel(ei, n)
    assert M.neighbors(s).index(t) == q and M.degree(s) == 130 and M.degree(t) == 131
    run_pass(G, M)
    for a, b in ((s, t), (t, s)):
        assert G.has_edge(a, b)
        G.add_edge(a, b)
        assert M.add_edge(a, b) == 2
        check(G, M, [s, t], (s, t), (s, spare), (q, a, b))
    incremental_equals_fresh_full(G, M, dcr, q)
    G.remove_edge(t, s)                               # and the removal finds it there too
    M.remove_edge(t, s)
    check(G, M, [s, t], (s, t), (s, spare), (q, 'removed'))
    incremental_equals_fresh_full(G, M, dcr, (q, 'removed'))


def test_find_stops_at_the_degree(dcr):
    """The key sits just past the degree, in the slack of both rows (an add and its removal leave the ids behind): it is not
    found, a second removal is a KeyError, and the add that follows is a real one."""
    ei, n, s, t, spare = gm.find_shape(64, False)
    G, M = dcr(ei, n), GraphModel(ei, n)
    assert M.degree(s) == 130 and M.degree(t) == 131 and not M.has_edge(s, t)
    run_pass(G, M)
    G.add_edge(s, t)
    M.add_edge(s, t)
    G.remove_edge(s, t)
    M.remove_edge(s, t)
    check(G, M, [s, t], (s, t), (t, spare), 'decoy in place')
    with pytest.raises(KeyError):
        G.remove_edge(t, s)
    with pytest.raises(KeyError):
        M.remove_edge(t, s)
    check(G, M, [s, t], (s, t), (t, spare), 'failed removal')
    incremental_equals_fresh_full(G, M, dcr, 'decoy')
    G.add_edge(t, s)
    assert M.add_edge(t, s) == 0
    check(G, M, [s, t], (s, t), (t, spare), 'real add')
    incremental_equals_fresh_full(G, M, dcr, 'real add')


# ---------------------------------------------------------------------------------------------------------------- case 3
@pytest.mark.parametrize('via', ['add_edge', 'sdrf_tail'])
@pytest.mark.parametrize('d0,slack', list(zip(gm.SLACK_DEG, gm.SLACK_WANT)))
def test_slack_boundaries_and_two_relayouts(dcr, d0, slack, via):
    """Exactly `slack` adds fit the row of a node of creation degree d0; the next one lays every row out again (ladder hubs of
    129 and 65 leaves with stale values among them), with twice the slack, and the row overflows a second time."""
    ei, n, z, partners = gm.slack_shape(d0)
    G, M = dcr(ei, n), GraphModel(ei, n)
    s1, s2 = gm.slack_script(d0)
    assert s1 == slack and M.cap[z] == d0 + slack
    run_pass(G, M)
    hub129, hub65 = 0, 1 + 129 + 129 * 130 // 2
    assert M.degree(hub129) == 129 and M.degree(hub65) == 65
    for k in range(s1 + s2 + 2):
        w = partners[k]
        if via == 'add_edge':
            G.add_edge(z, w) if k % 2 else G.add_edge(w, z)
            M.add_edge(z, w)
        else:
            assert G.sdrf_tail((z, w), False, 0.0)[0] is None
            M.sdrf_tail((z, w), False, 0.0)
        assert M.relayouts == (k >= s1) + (k >= s1 + s2), (k, M.relayouts)
        check(G, M, [z, w, hub129, hub65, hub65 + 33], (z, w), (z, partners[-1]), (d0, via, k))
    assert M.overflow_adds == [(z, partners[s1]), (z, partners[s1 + s2])]
    incremental_equals_fresh_full(G, M, dcr, (d0, via))


# ---------------------------------------------------------------------------------------------------------------- case 4
@pytest.mark.parametrize('op,via', [('add', 'calls'), ('add', 'tail'), ('remove', 'calls')])
@pytest.mark.parametrize('pending', [1, 3, 4])
def test_flags_at_the_walks_strides(dcr, monkeypatch, pending, op, via):
    """dev_mark_dirty from k_mark_dirty and from k_sdrf_tail (both 256 threads): the edge {a, b} with a at position 0, 63, 64, 255,
    256 or 257 of u's row and b at the same position of v's is recomputed after the edit of {u, v} only if both carry their
    flag.  With 1 and 3 edits pending the flags are exact and the pass reads its edges from the rows of the touched nodes; the
    fourth edit is the coarse one.  (The tail removes only the stale arg-max, which {u, v} with its 259 neighbours a side cannot
    be: the removal's flags go through k_mark_dirty, the same device function at the same width.)"""
    monkeypatch.setenv('DCR_NC_FINE', '1')
    monkeypatch.setenv('DCR_NC_FINE_SWEEP', '0')      # the edge list from the rows of the flagged nodes
    S = gm.flag_shape(with_uv=(op == 'remove'))
    u, v = S['u'], S['v']
    G, M = dcr(S['edge_index'], S['n']), GraphModel(S['edge_index'], S['n'])
    for k, p in enumerate(gm.FLAG_POS):
        assert M.neighbors(u)[p] == S['a'][k] and M.neighbors(v)[p] == S['b'][k] and M.has_edge(S['a'][k], S['b'][k])
    run_pass(G, M)
    for kind, x, y in gm.flag_extra_edits(S, pending - 1):
        getattr(G, kind + '_edge')(x, y)
        getattr(M, kind + '_edge')(x, y)
    if op == 'remove':
        G.remove_edge(u, v)
        M.remove_edge(u, v)
    elif via == 'calls':
        G.add_edge(v, u)
        M.add_edge(v, u)
    else:
        assert G.sdrf_tail((u, v), False, 0.0)[0] is None
        M.sdrf_tail((u, v), False, 0.0)
    assert M.pending == pending
    assert all(M.edge_is_dirty(a, b) for a, b in zip(S['a'], S['b']))
    check(G, M, [u, v, S['a'][4], S['b'][5]], (u, v), (u, S['b'][0]), (pending, op, via))
    incremental_equals_fresh_full(G, M, dcr, (pending, op, via))
    assert G.pass_engine() == 'node-centric'


# ---------------------------------------------------------------------------------------------------------------- case 5
@pytest.mark.parametrize('via', ['calls', 'tail'])
def test_kept_weights_at_the_strides(dcr, monkeypatch, via):
    """dev_weight_edit 64 wide (k_add_edge, k_remove_edge) and 256 wide (k_sdrf_tail) on rows of 259 entries with a common
    neighbour, under the forced two-hop route: the kept weights equal a recomputation from the rows after every edit, and
    after the add that overflows u's row and lays the rows out again."""
    monkeypatch.setenv('DCR_PASS', 'h2')
    S = gm.flag_shape(with_uv=False, common=True)
    u, v, n = S['u'], S['v'], S['n']
    G, M = dcr(S['edge_index'], n), GraphModel(S['edge_index'], n)
    assert G.h2_weight_check() == -1
    run_pass(G, M)
    assert G.pass_engine() == 'two-hop' and G.h2_weight_check() == 0
    M.start_weights()

    def add(x, y):
        if via == 'calls':
            G.add_edge(x, y)
            M.add_edge(x, y)
        else:
            assert G.sdrf_tail((x, y), False, 0.0)[0] is None
            M.sdrf_tail((x, y), False, 0.0)
        assert G.h2_weight_check() == 0 and M.weight_mismatches() == 0, (via, x, y)

    for _ in range(2):
        add(u, v)
        G.remove_edge(v, u)
        M.remove_edge(v, u)
        assert G.h2_weight_check() == 0 and M.weight_mismatches() == 0
    add(u, v)
    far = S['far']
    room = M.cap[u] - M.degree(u)
    targets = (far[6:] + S['b'] + S['ys'])[:room + 1]  # nodes that are not neighbours of u
    assert len(targets) == room + 1
    for w in targets:
        add(u, w)
    assert M.overflow_adds == [(u, targets[-1])]
    check(G, M, [u, v, targets[-1]], (u, v), (v, far[0]), via)
    run_pass(G, M)
    assert G.pass_engine() == 'two-hop' and G.h2_weight_check() == 0
    F = dcr(M.to_edge_index(), n)
    F.curvature_pass('bfc')
    assert value_dict(G) == value_dict(F)


# ---------------------------------------------------------------------------------------------------------------- case 6
def test_calls_that_must_leave_no_trace(dcr):
    ei, n, s, t, spare = gm.find_shape(65, True)
    ei = np.concatenate([ei, np.array([[n + 2], [n + 1]])], axis=1)
    iso1, iso2, n = n, n + 3, n + 4                   # two nodes without any edge beside the pair (n + 1, n + 2)
    G, M = dcr(ei, n), GraphModel(ei, n)
    run_pass(G, M)

    def same(what):
        check(G, M, [s, t, iso1, iso2, spare], (s, t), (iso1, iso2), what)

    for a, b in ((s, spare), (iso1, iso2), (iso2, t)):
        with pytest.raises(KeyError):
            G.remove_edge(a, b)
        with pytest.raises(KeyError):
            M.remove_edge(a, b)
        same(('absent', a, b))
    incremental_equals_fresh_full(G, M, dcr, 'failed removals')
    for call in ('add_edge', 'remove_edge'):
        for a, b in ((s, s), (-1, s), (s, n), (n, 0), (2 ** 31 - 1, 0)):
            with pytest.raises(ValueError):
                getattr(G, call)(a, b)
            with pytest.raises(ValueError):
                getattr(M, call)(a, b)
        same(call)
    for a, b in ((-1, s), (s, n)):
        with pytest.raises(ValueError):
            G.has_edge(a, b)
    assert not G.has_edge(s, s) and not M.has_edge(s, s) and not G.has_edge(iso1, iso1)
    same('has_edge')
    incremental_equals_fresh_full(G, M, dcr, 'argument errors')
    for bad_ei, bad_n in ((np.array([[1, 2], [0, 2]]), 3), (np.array([[1, 3], [0, 1]]), 3), (np.array([[1, -1], [0, 0]]), 3)):
        with pytest.raises(ValueError):
            dcr(bad_ei, bad_n)
        with pytest.raises(ValueError):
            GraphModel(bad_ei, bad_n)
    with pytest.raises(ValueError):
        dcr(np.array([[0], [0]]), 0)                  # no node to name
    E = dcr(np.zeros((2, 0), dtype=np.int64), 0)
    assert E.number_of_edges() == 0 and E.edges()[0].shape == (0,) and E.to_edge_index().shape == (2, 0)
    same('after the refused creations')


# ---------------------------------------------------------------------------------------------------------------- case 7
def test_creation_from_unsorted_duplicated_and_from_coalesced_input(dcr):
    import networkx as nx
    raw, coalesced, n = gm.creation_shape()
    rows = {}
    for name, ei in (('raw', raw), ('coalesced', coalesced)):
        G, M = dcr(ei, n), GraphModel(ei, n)
        assert M.created_sorted == (name == 'coalesced')
        assert M.degree(0) == 70
        X = nx.Graph()
        X.add_nodes_from(range(n))
        X.add_edges_from((int(a), int(b)) for a, b in ei.T if b <= a)
        for x in range(n):
            assert G.neighbors(x) == M.neighbors(x) == list(X[x]), (name, x)
        eu, ev = G.edges()
        assert list(zip(eu.tolist(), ev.tolist())) == [tuple(e) for e in X.edges]
        want = np.array(list(nx.convert_node_labels_to_integers(X).to_directed().edges), dtype=np.int64).T
        assert np.array_equal(G.to_edge_index(), want) and np.array_equal(M.to_edge_index(), want)
        check(G, M, [0, 1, n - 1], (0, 1), (0, 71), name)
        rows[name] = [M.neighbors(x) for x in range(n)]
    assert rows['raw'] != rows['coalesced']           # the same graph, other rows: the order of the input decides
    assert [sorted(r) for r in rows['raw']] == [sorted(r) for r in rows['coalesced']]
