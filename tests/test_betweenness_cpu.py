"""tests/betweenness_ref.py, the numpy restatement of the betweenness rule of include/dcr.h, against networkx (raw sums over all
sources are the ordered-pair convention: 2 x networkx's unnormalised undirected values) and against closed forms, on every graph
tests/test_betweenness_gpu.py uses; and the scalings of experiment/betweenness.py with the device call replaced by the replica."""
import networkx as nx
import numpy as np
import pytest

import betweenness_ref as br
import hops_ref
import spectral_ref

CASES = br.cases()
ALL_SOURCES_LIMIT = 400     # networkx runs every source up to this many nodes, the case's own (or eight drawn) sources above


def nx_graph(ei, n):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(np.asarray(ei, dtype=np.int64).T.tolist())
    return G


def nx_raw(G, n, eu, ev, sources):
    """The raw sums over `sources` (None: every node) from networkx: 2 x its unnormalised undirected values."""
    pairs = list(zip(eu.tolist(), ev.tolist()))
    if sources is None:
        bn, be = nx.betweenness_centrality(G, normalized=False), nx.edge_betweenness_centrality(G, normalized=False)
        return 2 * np.array([bn[v] for v in range(n)]), 2 * np.array([be[p] if p in be else be[p[::-1]] for p in pairs])
    node, edge = np.zeros(n), np.zeros(len(pairs))
    everyone = list(range(n))
    for s in np.asarray(sources).tolist():      # one at a time: a duplicated source counts twice
        bn = nx.betweenness_centrality_subset(G, [s], everyone, normalized=False)
        be = nx.edge_betweenness_centrality_subset(G, [s], everyone, normalized=False)
        node += 2 * np.array([bn[v] for v in range(n)])
        edge += 2 * np.array([be[p] if p in be else be[p[::-1]] for p in pairs])
    return node, edge


@pytest.mark.parametrize('name,ei,n,sources', CASES, ids=[c[0] for c in CASES])
def test_replica_against_networkx(name, ei, n, sources):
    if sources is None and n > ALL_SOURCES_LIMIT:
        sources = np.random.Generator(np.random.PCG64(n)).choice(n, size=8, replace=False)
    node, M, info = br.betweenness(ei, n, sources, edges=True)
    eu, ev = br.undirected_edges(ei)
    want_node, want_edge = nx_raw(nx_graph(ei, n), n, eu, ev, sources)
    tol = br.rtol(ei, n, info['levels_max'], n if sources is None else len(sources))
    br.assert_close(node, want_node, tol, name + ' nodes')
    br.assert_close(br.edge_values(M, eu, ev), want_edge, tol, name + ' edges')


def test_replica_at_scale_against_the_hop_totals():
    """70,001 nodes are minutes of networkx; the same code, held against it above, must at least put d(s, t) edges and d(s, t) - 1
    inner nodes on the paths of every pair: sums against the exact integers of hops_ref."""
    ei, n, src = br.scale_case()
    node, M, info = br.betweenness(ei, n, src, edges=True)
    _, ecc, reached, total = hops_ref.hops_sparse(ei, n, src, rows=False)
    eu, ev = br.undirected_edges(ei)
    tol = br.rtol(ei, n, info['levels_max'], src.size)
    assert info['levels_max'] == ecc.max() and (node >= 0).all()
    br.assert_close(br.edge_values(M, eu, ev).sum(), float(total.sum()), tol, 'scale edges')
    br.assert_close(node.sum(), float((total - reached + 1).sum()), tol, 'scale nodes')


def test_the_chunk_of_columns_changes_the_order_of_the_sums_only(monkeypatch):
    ei, n = hops_ref.irregular330()
    node, M, _ = br.betweenness(ei, n, edges=True)
    monkeypatch.setattr(br, 'CHUNK', 7)
    node7, M7, _ = br.betweenness(ei, n, edges=True)
    eu, ev = br.undirected_edges(ei)
    tol = br.rtol(ei, n, 6, n)
    br.assert_close(node7, node, tol)
    br.assert_close(br.edge_values(M7, eu, ev), br.edge_values(M, eu, ev), tol)


# ---- closed forms, by == ------------------------------------------------------------------------------------------------------------
def test_path_closed_form():
    ei, n = spectral_ref.path(300)
    node, M, info = br.betweenness(ei, n, edges=True)
    i = np.arange(300)
    assert np.array_equal(node, 2.0 * i * (299 - i)) and info['levels_max'] == 299 and info['sigma_max'] == 1.0
    j = np.arange(299)
    assert np.array_equal(br.edge_values(M, j, j + 1), 2.0 * (j + 1) * (299 - j))
    node3, _, _ = br.betweenness(ei, n, [0, 299, 150])
    assert np.array_equal(node3, path_three_sources())


def path_three_sources():
    """path(300), sources 0, 299 and 150: a source depends on an inner node by the number of nodes behind it."""
    i = np.arange(300)
    want = (299 - i) + i + np.where(i < 150, i, np.where(i > 150, 299 - i, 0))
    want[[0, 299]] = 0               # the ends are leaves: nothing passes through them
    return want.astype(np.float64)


def test_cycle_closed_forms():
    ei, n = spectral_ref.cycle(257)
    node, M, _ = br.betweenness(ei, n, edges=True)
    eu, ev = br.undirected_edges(ei)
    assert (node == 2 * (128 * 127 / 2)).all() and (br.edge_values(M, eu, ev) == 2 * (128 * 129 / 2)).all()
    ei, n = spectral_ref.cycle(64)                 # sigma = 2 at the antipode: halves
    node, M, info = br.betweenness(ei, n, edges=True)
    eu, ev = br.undirected_edges(ei)
    assert info['sigma_max'] == 2.0
    # ordered pairs at distance d < 32 put d - 1 inner nodes on their one path, the 64 antipodal ordered pairs 31 on each of two
    # paths at weight 1/2; by symmetry every node gets the same share
    assert (node == (2 * 64 * sum(d - 1 for d in range(1, 32)) + 64 * 31) / 64).all()
    assert (br.edge_values(M, eu, ev) == (2 * 64 * sum(range(1, 32)) + 64 * 32) / 64).all()


def test_star_closed_form():
    ei, n = hops_ref.hub_star(2100)
    node, M, _ = br.betweenness(ei, n, edges=True)
    assert node[0] == 2100 * 2099 and (node[1:] == 0).all()
    assert (br.edge_values(M, np.zeros(2100, dtype=np.int64), np.arange(1, 2101)) == 2 * 2100).all()


def test_diamond_chain_counts_paths():
    ei, n = br.diamonds(60)
    _, _, info = br.betweenness(ei, n, [0])
    assert info['sigma_max'] == 2.0 ** 60 and info['levels_max'] == 120


def test_sums_agree_with_the_hop_totals():
    ei, n = hops_ref.irregular330()
    node, M, info = br.betweenness(ei, n, edges=True)
    _, _, reached, total = hops_ref.hops(ei, n)
    eu, ev = br.undirected_edges(ei)
    tol = br.rtol(ei, n, info['levels_max'], n)
    # every ordered pair (s, t) puts d(s, t) edges and d(s, t) - 1 inner nodes on its paths, in shares that add up to one
    br.assert_close(br.edge_values(M, eu, ev).sum(), float(total.sum()), tol)
    br.assert_close(node.sum(), float((total - reached + 1).sum()), tol)


# ---- experiment/betweenness.py with the device call replaced by the replica ------------------------------------------------------------
class ReplicaGraph:
    """What experiment.betweenness needs of a DcrGraph, from the replica."""

    def __init__(self, ei, n):
        self.ei, self.n = ei, n
        self.calls = []

    def number_of_nodes(self):
        return self.n

    def betweenness(self, sources=None, edges=False, return_info=False):
        self.calls.append(None if sources is None else np.asarray(sources).copy())
        node, M, info = br.betweenness(self.ei, self.n, sources, edges=edges)
        info = dict(info, batches=-(-(self.n if sources is None else len(sources)) // 16))
        eu, ev = br.undirected_edges(self.ei)
        return (node, (eu, ev, br.edge_values(M, eu, ev)), info) if edges else (node, info)


@pytest.fixture
def replica_graph(monkeypatch):
    from experiment import betweenness as eb
    monkeypatch.setattr(eb, '_graph', lambda g: g)
    return eb


@pytest.mark.parametrize('normalized', [True, False])
def test_scalings_against_networkx(replica_graph, normalized):
    eb = replica_graph
    ei, n = hops_ref.irregular330()
    G = nx_graph(ei, n)
    out = eb.betweenness_centrality(ReplicaGraph(ei, n), normalized=normalized)
    want = nx.betweenness_centrality(G, normalized=normalized)
    tol = br.rtol(ei, n, out['levels_max'], n)
    assert out['exact'] and out['num_sources'] == n and out['normalized'] == normalized
    br.assert_close(out['values'], [want[v] for v in range(n)], tol)
    out = eb.edge_betweenness_centrality(ReplicaGraph(ei, n), normalized=normalized)
    want = nx.edge_betweenness_centrality(G, normalized=normalized)
    eu, ev = out['edges']
    assert out['exact']
    br.assert_close(out['values'], [want[p] if p in want else want[p[::-1]] for p in zip(eu.tolist(), ev.tolist())], tol)


@pytest.mark.parametrize('n', [1, 2, 3])
def test_scalings_of_tiny_graphs(replica_graph, n):
    eb = replica_graph
    ei, _ = spectral_ref.path(n) if n > 1 else hops_ref.empty(1)
    G = nx_graph(ei, n)
    for normalized in (True, False):
        want = nx.betweenness_centrality(G, normalized=normalized)
        assert eb.betweenness_centrality(ReplicaGraph(ei, n), normalized=normalized)['values'].tolist() == [want[v] for v in range(n)]
        want = nx.edge_betweenness_centrality(G, normalized=normalized)
        out = eb.edge_betweenness_centrality(ReplicaGraph(ei, n), normalized=normalized)
        assert out['values'].tolist() == [want[p] for p in zip(out['edges'][0].tolist(), out['edges'][1].tolist())]


def test_sampled_sources_are_scaled_by_n_over_k(replica_graph):
    from experiment.hop_metrics import draw_sources
    eb = replica_graph
    ei, n = hops_ref.irregular330()
    R = ReplicaGraph(ei, n)
    out = eb.betweenness_centrality(R, k=40, normalized=False, seed=3)
    src = draw_sources(n, 40, 3)
    assert np.array_equal(R.calls[0], src) and not out['exact'] and out['num_sources'] == 40
    raw, _, _ = br.betweenness(ei, n, src)
    assert np.array_equal(out['values'], raw * (0.5 * n / 40))
    out = eb.edge_betweenness_centrality(R, k=40, normalized=True, seed=3)
    _, M, _ = br.betweenness(ei, n, src, edges=True)
    eu, ev = out['edges']
    assert np.array_equal(out['values'], br.edge_values(M, eu, ev) * (1.0 / (n * (n - 1)) * n / 40)) and not out['exact']
    assert eb.betweenness_centrality(R, k=n)['exact'] and R.calls[-1] is None       # k >= n: every node
    with pytest.raises(ValueError):
        eb.betweenness_centrality(R, k=0)
