"""The host model of the graph container (tests/graph_model.py) held against networkx, its layout bookkeeping against
hand-computed cases, and its shapes shown to bite: every shape the GPU test uses is replayed on an ``nx.Graph`` built the way
the reference builds one, and for each kernel loop a fault planted IN THE MODEL changes what the model returns on the shape built
for that loop."""
import networkx as nx
import numpy as np
import pytest

import graph_model as gm
from graph_model import GraphModel


def nx_graph(ei, n):
    """to_networkx(data, to_undirected=True): the nodes, then the pairs with dst <= src in order."""
    X = nx.Graph()
    X.add_nodes_from(range(n))
    X.add_edges_from((int(a), int(b)) for a, b in np.asarray(ei).T if b <= a)
    return X


def same_rows(X, M, nodes):
    for x in nodes:
        assert list(X[x]) == M.neighbors(x) and X.degree(x) == M.degree(x), x


def same_lists(X, M):
    eu, ev = M.edges()
    assert list(zip(eu.tolist(), ev.tolist())) == [tuple(e) for e in X.edges]
    want = np.array(list(nx.convert_node_labels_to_integers(X).to_directed().edges), dtype=np.int64).reshape(-1, 2).T
    assert np.array_equal(M.to_edge_index(), want)
    assert M.number_of_edges() == X.number_of_edges()


def replay(X, M, ops, every_step=True):
    """('add' | 'remove', u, v) on both; the touched rows after every step, the two edge lists after every step or at the end."""
    for kind, u, v in ops:
        if kind == 'add':
            X.add_edge(u, v)
            M.add_edge(u, v)
        else:
            X.remove_edge(u, v)
            M.remove_edge(u, v)
        same_rows(X, M, [u, v])
        assert M.has_edge(u, v) == M.has_edge(v, u) == X.has_edge(u, v)
        if every_step:
            same_lists(X, M)
    same_lists(X, M)


def tree_values(M):
    """Balanced Forman curvature on a forest: 0 with an end of degree one, else 2 / du + 2 / dv - 2."""
    eu, ev = M.edges()
    du, dv = np.array([M.degree(x) for x in eu]), np.array([M.degree(x) for x in ev])
    cv = np.where(np.minimum(du, dv) == 1, 0.0, 2.0 / du + 2.0 / dv - 2.0)
    M.set_values(eu, ev, cv)


# ---------------------------------------------------------------------------------------------------------------- layout
def test_slack_and_relayout_on_hand_computed_cases():
    assert [gm.slack_for(d) for d in gm.SLACK_DEG] == list(gm.SLACK_WANT) == [8, 8, 8, 8, 9, 16]
    assert gm.RELAYOUT_FACTOR == 2
    # node 0 with 36 neighbours: 9 adds fit, the tenth overflows and every row gets twice its slack
    ei = np.array([list(range(1, 37)), [0] * 36])
    M = GraphModel(ei, 120)
    assert M.cap[0] == 45 and M.cap[1] == 9 and M.cap[119] == 8
    for k in range(9):
        assert M.add_edge(0, 40 + k) == 0
    assert M.relayouts == 0 and M.degree(0) == M.cap[0] == 45
    assert M.add_edge(0, 49) == 0
    assert M.relayouts == 1 and M.overflow_adds == [(0, 49)]
    assert M.cap[0] == 45 + 2 * 11 and M.cap[1] == 1 + 16 and M.cap[119] == 16 and M.cap[40] == 1 + 16
    for k in range(21):
        M.add_edge(0, 50 + k)
    assert M.relayouts == 1 and M.degree(0) == M.cap[0] == 67
    M.add_edge(0, 71)
    assert M.relayouts == 2 and M.cap[0] == 67 + 2 * 16
    assert M.add_edge(71, 0) == 2 and M.relayouts == 2      # an existing edge never lays out again
    # a full row on the OTHER side of the add overflows too
    M2 = GraphModel(np.array([list(range(1, 9)), [0] * 8]), 30)
    for k in range(8):
        M2.add_edge(0, 10 + k)
    assert M2.relayouts == 0
    M2.add_edge(20, 0)
    assert M2.relayouts == 1 and M2.overflow_adds == [(20, 0)]


@pytest.mark.parametrize('d0', gm.SLACK_DEG)
def test_slack_script_against_the_model_and_the_fault(d0):
    ei, n, z, partners = gm.slack_shape(d0)
    s1, s2 = gm.slack_script(d0)
    assert len(partners) >= s1 + s2 + 2
    X, M, F = nx_graph(ei, n), GraphModel(ei, n), GraphModel(ei, n, fault='slack_off_by_one')
    same_lists(X, M)
    assert M.degree(z) == d0 and M.cap[z] == d0 + s1 and F.cap[z] == d0 + s1 - 1
    assert M.degree(0) == 129 and M.degree(1 + 129 + 129 * 130 // 2) == 65     # rows of more than two strides and more than one
    steps = []
    for k in range(s1 + s2 + 2):
        X.add_edge(z, partners[k])
        M.add_edge(z, partners[k])
        F.add_edge(z, partners[k])
        same_rows(X, M, [z, partners[k]])
        steps.append(M.relayouts)
    same_lists(X, M)
    assert steps == [0] * s1 + [1] * s2 + [2, 2]
    assert M.overflow_adds == [(z, partners[s1]), (z, partners[s1 + s2])]
    assert F.overflow_adds != M.overflow_adds and F.overflow_adds[0] == (z, partners[s1 - 1])


# ---------------------------------------------------------------------------------------------------------------- erase
@pytest.mark.parametrize('d', gm.ERASE_D)
def test_erase_shapes(d):
    positions = gm.erase_positions(d)
    assert positions == sorted({p for p in (0, 1, 62, 63, 64, 65, 126, 127, 128, d - 66, d - 65, d - 64, d - 2, d - 1) if 0 <= p < d})
    leaf_side = set()
    for k, p in enumerate(positions):
        ei, n, hub, leaf, p2, lp = gm.erase_shape(d, k)
        assert p2 == p
        X, M, F = nx_graph(ei, n), GraphModel(ei, n), GraphModel(ei, n, fault='erase_last_stride')
        assert M.neighbors(hub).index(leaf) == p and M.neighbors(leaf).index(hub) == lp and M.degree(leaf) == p + 2
        leaf_side.add('first' if lp == 0 else 'last' if lp == p + 1 else 'middle')
        tree_values(M)
        eu, ev, cv, _ = M.values()
        hv = cv[eu == hub]
        assert hv.size == d and np.unique(hv).size == d              # the hub edges' values are pairwise distinct
        F.set_values(eu, ev, cv)
        replay(X, M, [('remove', hub, leaf)], every_step=(d < 128 or k % 5 == 0))
        F.remove_edge(hub, leaf)
        moved = d - 1 - p                                           # entries behind the removed one
        differs = not np.array_equal(M.values()[2], F.values()[2])
        assert differs == (moved >= 1 or lp < p + 1), (d, p)         # the shape tells a dropped value shift from a right one
    if d >= 64:
        assert leaf_side == {'first', 'middle', 'last'}
    if d >= 129:
        assert {d - 1 - p for p in positions} >= {63, 64, 65} and set(positions) >= {63, 64, 65, 127, 128}


@pytest.mark.parametrize('d', gm.ERASE_D)
def test_tail_erase_plan(d):
    order, probes = gm.tail_erase_plan(d)
    assert sorted(order) == list(range(1, d + 1))
    P = gm.Parts()
    hub, leaf, pend = gm.add_ladder_hub(P, d, hub_order=order)
    q1, q2 = P.nodes(2)
    ei, n = P.edge_index(), P.n
    X, M, F = nx_graph(ei, n), GraphModel(ei, n), GraphModel(ei, n, fault='erase_last_stride')
    tree_values(M)
    F.set_values(*M.values()[:3])
    ops = [('remove', leaf[i], q) for i in range(1, d + 1) for q in pend[i]]
    replay(X, M, ops, every_step=False)
    for _, a, b in ops:
        F.remove_edge(a, b)
    bites = 0
    for k, (p, length) in enumerate(probes):
        target = leaf[k + 1]
        assert M.degree(hub) == length and M.neighbors(hub).index(target) == p     # the probed position exists
        removed, _ = M.sdrf_tail((q1, q2), True, -10.0)
        assert removed == (hub, target)                                            # ... and holds the stale arg-max
        F.add_edge(q1, q2)
        F.remove_edge(hub, target)
        X.add_edge(q1, q2)
        X.remove_edge(hub, target)
        for G in (X, M, F):
            G.remove_edge(q2, q1)
        same_rows(X, M, [hub, target, q1, q2])
        bites += not np.array_equal(M.values()[2], F.values()[2])
    same_lists(X, M)
    assert M.degree(hub) == d - len(probes) >= 1
    got = set(probes)
    if d >= 129:
        assert {length - 1 - p for p, length in got} >= {0, 1, 63, 64, 65} and {p for p, _ in got} >= {0, 1, 62, 63, 64, 65}
    if d >= 193:
        assert {p for p, _ in got} >= {126, 127, 128}
    assert bites >= len(probes) - 2                # every probe with an entry behind it


# ---------------------------------------------------------------------------------------------------------------- find
@pytest.mark.parametrize('q', gm.FIND_POS)
def test_find_shapes(q):
    ei, n, s, t, spare = gm.find_shape(q, True)
    X, M, F = nx_graph(ei, n), GraphModel(ei, n), GraphModel(ei, n, fault='find_64')
    same_lists(X, M)
    assert M.degree(s) == 130 and M.degree(t) == 131 and M.neighbors(s).index(t) == q and M.neighbors(t).index(s) == 100
    assert M.has_edge(s, t) and M.has_edge(t, s) and not F.has_edge(s, t) and not F.has_edge(t, s)
    assert M.add_edge(s, t) == 2 and M.add_edge(t, s) == 2 and F.add_edge(s, t) == 0
    replay(X, M, [('add', s, t), ('add', t, s), ('remove', t, s)])
    with pytest.raises(KeyError):
        F.remove_edge(spare, s)
    ei, n, s, t, spare = gm.find_shape(q, False)
    X, M = nx_graph(ei, n), GraphModel(ei, n)
    assert M.degree(s) == 130 and M.degree(t) == 131 and not M.has_edge(s, t)
    replay(X, M, [('add', s, t), ('remove', s, t), ('add', t, s)])


# ---------------------------------------------------------------------------------------------------------------- flags
@pytest.mark.parametrize('op', ['add', 'remove'])
@pytest.mark.parametrize('pending', [1, 3, 4])
def test_flag_shape(pending, op):
    S = gm.flag_shape(with_uv=(op == 'remove'))
    u, v, n = S['u'], S['v'], S['n']
    X, M, F = nx_graph(S['edge_index'], n), GraphModel(S['edge_index'], n), GraphModel(S['edge_index'], n, fault='flag_256')
    same_lists(X, M)
    assert M.degree(u) == M.degree(v) == gm.FLAG_DEG + (op == 'remove')
    for k, p in enumerate(gm.FLAG_POS):
        a, b = S['a'][k], S['b'][k]
        assert M.neighbors(u)[p] == a and M.neighbors(v)[p] == b
        # the witness edge is all a and b are there for: their other edge goes to the endpoint itself
        assert sorted(M.neighbors(a)) == sorted([u, b]) and sorted(M.neighbors(b)) == sorted([v, a])
    ops = [(kind, x, y) for kind, x, y in gm.flag_extra_edits(S, pending - 1)] + [(op, u, v)]
    assert len(ops) == pending
    for kind, x, y in ops[:-1]:
        assert not ({x, y} | set(M.neighbors(x)) | set(M.neighbors(y))) & ({u, v} | set(M.neighbors(u)) | set(M.neighbors(v)))
    replay(X, M, ops)
    for kind, x, y in ops:
        getattr(F, kind + '_edge')(x, y)
    assert M.pending == pending
    for k, p in enumerate(gm.FLAG_POS):
        a, b = S['a'][k], S['b'][k]
        assert X.has_edge(u, v) == (op == 'add') and X.has_edge(a, u) and X.has_edge(b, v)    # the 4-cycle a-u-v-b came or went
        assert M.edge_is_dirty(a, b) and M.edge_is_dirty(b, a)
        assert F.edge_is_dirty(a, b) == (p < gm.FLAG_STRIDE)       # both walks stop at 256: the witnesses behind it are missed
    if pending <= gm.DIRTY_EDITS:
        assert not M.edge_is_dirty(S['xs'][0], S['far'][11])        # exact flags: an A bit alone recomputes nothing


# ---------------------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize('wide', [False, True])
def test_weight_shape(wide):
    S = gm.flag_shape(with_uv=False, common=True)
    u, v, c, n = S['u'], S['v'], S['c'], S['n']
    M, F = GraphModel(S['edge_index'], n), GraphModel(S['edge_index'], n, fault='weight_64')
    assert M.neighbors(u)[-1] == c and M.neighbors(v)[-1] == c and M.degree(u) == gm.FLAG_DEG + 1
    for G in (M, F):
        G.start_weights()
        assert G.weight_mismatches() == 0
        G.add_edge(u, v, wide=wide)
    assert M.weight_mismatches() == 0 and M.W[c] == 2 * (gm.FLAG_DEG + 2)
    assert (F.weight_mismatches() > 0) == (not wide)               # the 64-wide walk is the one the fault cuts short
    for G in (M, F):
        G.remove_edge(v, u, wide=wide)
    assert M.weight_mismatches() == 0 and M.W[c] == 2 * (gm.FLAG_DEG + 1)
    room = M.cap[u] - M.degree(u)
    targets = (S['far'][6:] + S['b'] + S['ys'])[:room + 1]
    assert len(targets) == room + 1 and not any(M.has_edge(u, w) for w in targets)
    for w in targets:
        M.add_edge(u, w, wide=wide)
    assert M.overflow_adds == [(u, targets[-1])] and M.weight_mismatches() == 0


# ---------------------------------------------------------------------------------------------------------------- the rest
def test_creation_shape_and_refused_calls():
    raw, coalesced, n = gm.creation_shape()
    rows = []
    for ei, is_sorted in ((raw, False), (coalesced, True)):
        X, M = nx_graph(ei, n), GraphModel(ei, n)
        assert M.created_sorted == is_sorted and M.degree(0) == 70 > gm.STRIDE
        same_rows(X, M, range(n))
        same_lists(X, M)
        rows.append([M.neighbors(x) for x in range(n)])
    assert rows[0] != rows[1] and [sorted(r) for r in rows[0]] == [sorted(r) for r in rows[1]]
    pairs = list(zip(raw[0].tolist(), raw[1].tolist()))
    assert len(set(pairs)) < len(pairs) and any((b, a) in pairs for a, b in pairs)       # duplicates, both orientations
    M = GraphModel(raw, n)
    before = ([M.neighbors(x) for x in range(n)], M.pending)
    for call in (M.add_edge, M.remove_edge, M.has_edge):
        for a, b in ((-1, 0), (0, n), (n, 0)):
            with pytest.raises(ValueError):
                call(a, b)
    for call in (M.add_edge, M.remove_edge):
        with pytest.raises(ValueError):
            call(3, 3)
    assert not M.has_edge(3, 3)
    assert ([M.neighbors(x) for x in range(n)], M.pending) == before
    with pytest.raises(KeyError):
        M.remove_edge(0, 80)
    assert M.pending == 1 and [M.neighbors(x) for x in range(n)] == before[0]     # flagged and counted, nothing else
    for bad, bad_n in ((np.array([[1, 2], [0, 2]]), 3), (np.array([[1, 3], [0, 1]]), 3), (np.array([[0], [0]]), 0)):
        with pytest.raises(ValueError):
            GraphModel(bad, bad_n)
    E = GraphModel(np.zeros((2, 0), dtype=np.int64), 0)
    assert E.number_of_edges() == 0 and E.edges()[0].shape == (0,) and E.to_edge_index().shape == (2, 0)


def test_the_source_patterns_fail_loudly(monkeypatch):
    monkeypatch.setattr(gm, '_read', lambda name: 'static inline int32_t slack_for(int32_t deg) { return 8; }')
    with pytest.raises(AssertionError):
        gm._layout_constants()
