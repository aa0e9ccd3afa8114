"""Betweenness on the device (csrc/dcr_betweenness.hip) against tests/betweenness_ref.py, which tests/test_betweenness_cpu.py holds
against networkx on every graph used here.  Closed forms and everything whose path counts are 1 or powers of two compare by ==;
the rest under the derived tolerance of betweenness_ref.rtol: rtol = 4 k 2^-53 with k = 2 D (maxdeg + 3) + S, atol = 0.  Shapes are
the smallest at which each piece can go wrong: degenerate and disconnected graphs, 299 levels, every row class at its workgroup,
wave and turn boundaries, source counts either side of the batch of 16, a graph edited between calls, path counts past 2^53 and
past the float64 range, and one size of tests/scale_ref.py where the row kernels have more than a thousand workgroups."""
import numpy as np
import pytest

import betweenness_ref as br
import hops_ref
import spectral_ref

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name, ei, n, sources=None):
    """(node, edge matrix, info) of the replica for a named graph and source list, computed once and never written to."""
    key = (name, None if sources is None else tuple(np.asarray(sources).tolist()))
    if key not in _REF:
        node, M, info = br.betweenness(ei, n, sources, edges=True)
        node.setflags(write=False)
        _REF[key] = (node, M, info)
    return _REF[key]


def graph(ei, n):
    from dcr.graph import DcrGraph
    return DcrGraph(ei, n)


def call(G, sources=None):
    """(node, eu, ev, edge, info) of one call with edge values; the node values of a call without them must be the same bits."""
    node, (eu, ev, edge), info = G.betweenness(sources, edges=True, return_info=True)
    assert node.dtype == np.float64 and edge.dtype == np.float64 and node.shape == (G.num_nodes,) and edge.shape == eu.shape
    geu, gev = G.edges()
    assert np.array_equal(eu, geu) and np.array_equal(ev, gev)
    alone = G.betweenness(sources)
    assert alone.tobytes() == node.tobytes()
    return node, eu, ev, edge, info


def check(G, name, ei, n, sources=None, exact=False):
    """One call against the replica: by == where `exact`, under the tolerance otherwise."""
    want_node, M, want_info = reference(name, ei, n, sources)
    node, eu, ev, edge, info = call(G, sources)
    want_edge = br.edge_values(M, eu, ev)
    P = n if sources is None else len(sources)
    assert info['levels_max'] == want_info['levels_max'] and info['batches'] == -(-P // 16), name
    if exact:
        assert info['sigma_max'] == want_info['sigma_max']
        assert np.array_equal(node, want_node) and np.array_equal(edge, want_edge), name
    else:
        tol = br.rtol(ei, n, want_info['levels_max'], P)
        br.assert_close(info['sigma_max'], want_info['sigma_max'], tol, name + ' sigma_max')
        br.assert_close(node, want_node, tol, name + ' nodes')
        br.assert_close(edge, want_edge, tol, name + ' edges')
    return node, eu, ev, edge, info


# 1
@pytest.mark.parametrize('name,ei,n', hops_ref.degenerate(), ids=[g[0] for g in hops_ref.degenerate()])
def test_degenerate_graphs(name, ei, n):
    node, eu, ev, edge, info = check(graph(ei, n), name, ei, n, exact=True)   # path counts 1 and 2 only: every value a dyadic fraction
    isolated = np.bincount(np.asarray(ei[0], dtype=np.int64), minlength=n) == 0
    assert (node[isolated] == 0).all()
    if isolated.all():
        assert edge.size == 0 and info['levels_max'] == 0 and (node == 0).all()
    # a pair in different components contributes nothing: the values are those of the components on their own
    _, labels = spectral_ref.components(ei, n)
    for root in np.unique(labels):
        inside = np.flatnonzero(labels == root)
        if inside.size < 3:
            continue
        sub = np.searchsorted(inside, np.asarray(ei)[:, np.isin(np.asarray(ei)[0], inside)])
        own, _, own_info = br.betweenness(sub, inside.size)
        br.assert_close(node[inside], own, br.rtol(sub, inside.size, own_info['levels_max'], inside.size), name)


# 2
def test_path_of_300_has_299_levels():
    ei, n = spectral_ref.path(300)
    G = graph(ei, n)
    node, _, _, _, info = check(G, 'path300', ei, n, np.array([0, 299, 150]), exact=True)
    i = np.arange(300)
    want = ((299 - i) + i + np.where(i < 150, i, np.where(i > 150, 299 - i, 0))).astype(np.float64)
    want[[0, 299]] = 0
    assert np.array_equal(node, want) and info['levels_max'] == 299 and info['sigma_max'] == 1.0
    node, eu, ev, edge, info = check(G, 'path300', ei, n, exact=True)
    assert np.array_equal(node, 2.0 * i * (299 - i)) and info['batches'] == 19
    assert np.array_equal(ev, eu + 1) and np.array_equal(edge, 2.0 * (eu + 1) * (299 - eu))


# 3
def test_cycles():
    ei, n = spectral_ref.cycle(257)
    node, _, _, edge, _ = check(graph(ei, n), 'cycle257', ei, n, exact=True)
    assert (node == 2 * (128 * 127 / 2)).all() and (edge == 2 * (128 * 129 / 2)).all()
    ei, n = spectral_ref.cycle(64)                 # sigma = 2 at the antipodes: halves, all exact in float64
    node, _, _, edge, info = check(graph(ei, n), 'cycle64', ei, n, exact=True)
    # ordered pairs at distance d < 32 put d - 1 inner nodes on their one path, the 64 antipodal ones 31 on each of two at weight 1/2
    assert info['sigma_max'] == 2.0 and (node == (2 * 64 * sum(d - 1 for d in range(1, 32)) + 64 * 31) / 64).all()
    assert (edge == (2 * 64 * sum(range(1, 32)) + 64 * 32) / 64).all()


# 4
def test_star_with_a_long_hub_row():
    ei, n = hops_ref.hub_star(2100)
    G = graph(ei, n)
    assert G.degree(0) == 2100
    node, eu, ev, edge, info = call(G)
    assert node[0] == 2100 * 2099 and (node[1:] == 0).all() and (edge == 2 * 2100).all() and edge.size == 2100
    assert info['levels_max'] == 2 and info['sigma_max'] == 1.0 and info['batches'] == -(-2101 // 16)


# 5
@pytest.mark.parametrize('name', spectral_ref.PLAN_NAMES)
def test_every_row_class(name):
    ei, n = br.plan_graph(name)
    src = br.plan_sources(name)
    deg = np.bincount(np.asarray(ei)[0], minlength=n)
    assert src.size == 48 and deg[src[0]] == deg.max()
    check(graph(ei, n), name, ei, n, src)


# 6
@pytest.mark.parametrize('P', [1, 15, 16, 17, 33])
def test_source_counts_either_side_of_the_batch(P):
    ei, n = hops_ref.irregular330()
    src = br.boundary_sources(P, n)
    assert src.size == P and (P < 15 or (np.unique(src).size < P and n - 1 in src and n - 2 in src))
    node, _, _, _, info = check(graph(ei, n), 'irregular330', ei, n, src)
    assert info['batches'] == -(-P // 16) and node[n - 1] == 0 and node[n - 2] == 0


# 7
def test_sums_agree_with_the_hop_totals():
    ei, n = hops_ref.irregular330()
    G = graph(ei, n)
    node, _, _, edge, info = call(G)
    _, reached, total = G.hop_summary()
    tol = br.rtol(ei, n, info['levels_max'], n)
    # every ordered pair (s, t) puts d(s, t) edges and d(s, t) - 1 inner nodes on its shortest paths, in shares that add up to one
    br.assert_close(edge.sum(), float(total.sum()), tol, 'edges')
    br.assert_close(node.sum(), float((total - reached + 1).sum()), tol, 'nodes')
    check(G, 'irregular330', ei, n)


# 8
def test_graph_edited_between_calls():
    name = 'long3_mid9_short63'
    ei, n = br.plan_graph(name)
    names = spectral_ref.plan_nodes(name)
    src = br.plan_sources(name)
    G = graph(ei, n)
    check(G, name, ei, n, src)
    h0, h2 = names['hub0'], names['hub2']
    assert not G.has_edge(h0, h2)
    G.add_edge(h0, h2)                                           # hub to hub: two long rows grow
    ei1, _ = hops_ref.with_edge(ei, n, h0, h2)
    check(G, name + '+hubs', ei1, n, src)
    middle = G.neighbors(h0)[1000]
    G.remove_edge(h0, middle)                                    # leaves a hole in the long row, filled from its end
    ei2, _ = hops_ref.with_edge(ei1, n, h0, middle, remove=True)
    check(G, name + '+hubs-middle', ei2, n, src)
    a, b = names['leaf_first'], names['isolated']
    G.add_edge(a, b)                                             # an isolated node joins
    ei3, _ = hops_ref.with_edge(ei2, n, a, b)
    node, _, _, _, _ = check(G, name + '+hubs-middle+isolated', ei3, n, np.concatenate([src, [b]]).astype(np.int32))
    assert node[b] == 0


# 9
def test_two_calls_return_the_same_bits():
    ei, n = hops_ref.irregular330()
    G = graph(ei, n)
    first = call(G)
    second = call(G)
    assert first[0].tobytes() == second[0].tobytes() and first[3].tobytes() == second[3].tobytes()
    other = call(graph(ei, n))                                   # and on another handle of the same graph
    assert first[0].tobytes() == other[0].tobytes() and first[3].tobytes() == other[3].tobytes()


# 10
def test_path_counts_past_2_to_53_and_past_float64():
    from dcr import _lib
    ei, n = br.diamonds(60)
    node, _, _, _, info = check(graph(ei, n), 'diamonds60', ei, n, np.array([0, 180, 90], dtype=np.int32))
    assert info['sigma_max'] == 2.0 ** 60 and info['sigma_max'] > 2.0 ** 53 and info['levels_max'] == 120
    ei, n = br.diamonds(1030)                                    # 2^1030 paths: beyond the float64 range
    G = graph(ei, n)
    with pytest.raises(_lib.DcrError, match='float64 range'):
        G.betweenness(np.array([0], dtype=np.int32), edges=True)
    # an error return, not a fault: the handle goes on working
    middle = 3 * 515                                             # from a_515 every count is a power of two up to 2^515: exact
    node, _, _, edge, info = check(G, 'diamonds1030', ei, n, np.array([middle], dtype=np.int32), exact=True)
    assert np.isfinite(node).all() and np.isfinite(edge).all() and info['sigma_max'] == 2.0 ** 515
    assert node[middle] == 0 and node[0] == 0 and node[3] == 3.0  # through a_1 go the paths to a_0 and to the two nodes before it


# 11
def test_one_size_of_the_scale_family():
    ei, n, src = br.scale_case()
    assert src.size == 16
    node, _, _, _, info = check(graph(ei, n), 'whole_small', ei, n, src)
    assert info['levels_max'] > 1000 and node.max() > 0


# 12
@pytest.mark.parametrize('normalized', [True, False])
def test_experiment_module_against_networkx(normalized):
    import networkx as nx

    from experiment import betweenness as eb
    ei, n = hops_ref.irregular330()
    H = nx.Graph()
    H.add_nodes_from(range(n))
    H.add_edges_from(np.asarray(ei, dtype=np.int64).T.tolist())
    G = graph(ei, n)
    out = eb.betweenness_centrality(G, normalized=normalized)
    want = nx.betweenness_centrality(H, normalized=normalized)
    tol = br.rtol(ei, n, out['levels_max'], n)
    assert out['exact'] and out['num_sources'] == n
    br.assert_close(out['values'], [want[v] for v in range(n)], tol)
    out = eb.edge_betweenness_centrality(G, normalized=normalized)
    want = nx.edge_betweenness_centrality(H, normalized=normalized)
    eu, ev = out['edges']
    br.assert_close(out['values'], [want[p] if p in want else want[p[::-1]] for p in zip(eu.tolist(), ev.tolist())], tol)
    sampled = eb.betweenness_centrality(G, k=40, normalized=False, seed=3)
    assert not sampled['exact'] and sampled['num_sources'] == 40
