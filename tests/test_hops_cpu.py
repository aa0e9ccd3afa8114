"""Hop distances without a GPU: the rule of include/dcr.h (tests/hops_ref.py) against scipy's shortest paths and networkx on every
graph tests/test_hops_gpu.py uses, the pure aggregation of experiment/hop_metrics.py on hand-made arrays, and the call surface."""
import os
import re

import networkx as nx
import numpy as np
import pytest
import scipy.sparse.csgraph

import hops_ref
import spectral_ref
from conftest import PKG, REPO

CSRC = os.path.join(PKG, 'csrc')


def fixtures():
    out = hops_ref.degenerate() + hops_ref.deep() + spectral_ref.plan_family()
    out += [('hub_star', *hops_ref.hub_star()), ('irregular330', *hops_ref.irregular330())]
    chord = hops_ref.with_edge(*spectral_ref.path(300), 10, 250)
    out += [('path300_chord', *chord), ('path300_chord_cut', *hops_ref.with_edge(*chord, 100, 101, remove=True))]
    return out


FIXTURES = {name: (ei, n) for name, ei, n in fixtures()}


def scipy_dist(ei, n):
    d = scipy.sparse.csgraph.shortest_path(spectral_ref.adjacency(ei, n), method='D', directed=False, unweighted=True)
    return np.where(np.isinf(d), -1, d).astype(np.int32)


@pytest.fixture(scope='module')
def solved():
    """name -> (reference outputs over all sources, scipy's distance matrix), computed once."""
    return {name: (hops_ref.hops(ei, n), scipy_dist(ei, n)) for name, (ei, n) in FIXTURES.items()}


@pytest.mark.parametrize('name', list(FIXTURES))
def test_reference_is_scipy_shortest_path(name, solved):
    (dist, ecc, reached, total), want = solved[name]
    assert dist.dtype == np.int32 and np.array_equal(dist, want)
    e, r, t = hops_ref.summaries_of(want)
    assert np.array_equal(ecc, e) and np.array_equal(reached, r) and np.array_equal(total, t)
    assert np.array_equal(dist, dist.T) and (np.diag(dist) == 0).all()


@pytest.mark.parametrize('name', list(FIXTURES))
@pytest.mark.parametrize('max_hops', [0, 1, 2, 7])
def test_reference_hop_limit_is_a_cut_of_the_full_distances(name, max_hops, solved):
    ei, n = FIXTURES[name]
    src = np.unique(np.linspace(0, n - 1, 9).astype(np.int64))
    dist, ecc, reached, total = hops_ref.hops(ei, n, src, max_hops=max_hops)
    want = solved[name][1][src]
    want = np.where(want > max_hops, -1, want)
    assert np.array_equal(dist, want)
    e, r, t = hops_ref.summaries_of(want)
    assert np.array_equal(ecc, e) and np.array_equal(reached, r) and np.array_equal(total, t)
    if max_hops == 0:
        assert (ecc == 0).all() and (reached == 1).all() and (total == 0).all()


@pytest.mark.parametrize('name', ['two_components', 'three_components', 'isolated_among_connected', 'cycle257', 'mid5_short9',
                                  'irregular330', 'path300_chord_cut'])
def test_reference_and_aggregation_are_networkx(name, solved):
    from experiment.hop_metrics import aggregate
    ei, n = FIXTURES[name]
    (dist, ecc, reached, total), _ = solved[name]
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(np.asarray(ei).T.tolist())
    labels = spectral_ref.components(ei, n)[1]
    m = aggregate(ecc, reached, total, labels)
    comps = sorted(nx.connected_components(G), key=lambda c: (-len(c), min(c)))
    for c in comps:
        sub = G.subgraph(c)
        want = nx.eccentricity(sub)
        assert all(ecc[v] == want[v] for v in c)
    big = G.subgraph(comps[0])
    assert m['exact'] and m['largest_component'] == len(comps[0])
    assert m['radius'] == nx.radius(big)
    assert m['diameter'] == max(nx.diameter(G.subgraph(c)) for c in comps)
    want = nx.average_shortest_path_length(big)
    assert abs(m['average_path_length'] - want) <= 4 * np.finfo(np.float64).eps * want   # one division here, a sum of quotients there


def test_aggregation_on_hand_made_arrays():
    from experiment.hop_metrics import aggregate
    # a path 0-1-2-3, a triangle 4-5-6 and the isolated node 7
    labels = np.array([0, 0, 0, 0, 4, 4, 4, 7])
    ecc = np.array([3, 2, 2, 3, 1, 1, 1, 0], dtype=np.int32)
    reached = np.array([4, 4, 4, 4, 3, 3, 3, 1], dtype=np.int64)
    total = np.array([6, 4, 4, 6, 2, 2, 2, 0], dtype=np.int64)
    m = aggregate(ecc, reached, total, labels)
    assert m['exact'] and m['diameter'] == 3 and m['radius'] == 2 and m['largest_component'] == 4 and m['num_sources'] == 8
    assert m['average_path_length'] == 20 / 12
    assert m['eccentricity'] is ecc and np.array_equal(m['reached'], reached)
    # sampled sources: one in the path, one in the triangle, the isolated node
    src = np.array([1, 5, 7])
    m = aggregate(ecc[src], reached[src], total[src], labels, src)
    assert not m['exact'] and m['diameter'] == 2 and m['radius'] == 2 and m['average_path_length'] == 4 / 3
    # no source in the largest component
    src = np.array([7, 4])
    m = aggregate(ecc[src], reached[src], total[src], labels, src)
    assert m['diameter'] == 1 and m['radius'] is None and np.isnan(m['average_path_length']) and not m['exact']
    # two components of equal size: the one with the smaller label is the largest; duplicated sources do not make a sample exact
    labels = np.array([0, 1, 0, 1])
    m = aggregate([1, 1], [2, 2], [1, 1], labels, [1, 3])
    assert m['radius'] is None and m['largest_component'] == 2
    m = aggregate([1, 1, 1, 1], [2, 2, 2, 2], [1, 1, 1, 1], labels, [0, 0, 2, 2])
    assert not m['exact'] and m['radius'] == 1 and m['average_path_length'] == 1.0
    # isolated nodes only: every component is a single node
    m = aggregate(np.zeros(3, np.int32), np.ones(3, np.int64), np.zeros(3, np.int64), np.arange(3))
    assert m['exact'] and m['diameter'] == 0 and m['radius'] == 0 and m['average_path_length'] == 0.0
    # no sources at all
    m = aggregate(np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.arange(3), np.zeros(0, np.int64))
    assert m['diameter'] is None and m['radius'] is None and np.isnan(m['average_path_length']) and not m['exact']
    with pytest.raises(ValueError):
        aggregate([1, 2], [1], [1, 2], labels, [0, 1])


def test_sampled_sources_are_seeded_distinct_and_sorted():
    from experiment.hop_metrics import draw_sources
    a, b = draw_sources(1000, 50, seed=3), draw_sources(1000, 50, seed=3)
    assert np.array_equal(a, b) and a.dtype == np.int32 and np.unique(a).size == 50 and (np.diff(a) > 0).all()
    assert not np.array_equal(a, draw_sources(1000, 50, seed=4))
    assert np.array_equal(a, np.sort(np.random.Generator(np.random.PCG64(3)).choice(1000, size=50, replace=False)))
    assert np.array_equal(draw_sources(5, 9), np.arange(5))


def test_call_surface():
    from dcr import _lib
    from dcr.graph import DcrGraph
    from experiment import hop_metrics
    header = open(os.path.join(REPO, 'include', 'dcr.h')).read()
    bare = re.sub(r'/\*.*?\*/', '', header, flags=re.S)               # (a comment of the declaration holds a semicolon)
    m = re.search(r'\bint\s+dcr_hop_distances\s*\(([^;]*)\)\s*;', bare)
    assert m, 'dcr_hop_distances is not declared in include/dcr.h'
    assert len(m.group(1).split(',')) == len(_lib.SIGNATURES['dcr_hop_distances'][1]) == 8
    assert re.search(r'typedef\s+struct\s*\{\s*int32_t\s+max_hops\s*;[^}]*\}\s*dcr_hops_opts', header)
    assert [f[0] for f in _lib.HopsOpts._fields_] == ['max_hops'] and _lib.HopsOpts._fields_[0][1] is _lib._i32
    assert callable(DcrGraph.hop_distances) and callable(DcrGraph.hop_summary)
    assert callable(hop_metrics.hop_metrics) and callable(hop_metrics.ball_sizes) and callable(hop_metrics.aggregate)
    assert 'dcr_hops' in open(os.path.join(CSRC, 'build.sh')).read().split()
    assert 'dcr_hops' in open(os.path.join(REPO, 'tools', 'build_variant.sh')).read().split()
    source = open(os.path.join(CSRC, 'dcr_hops.hip')).read()
    assert 'asm' not in re.sub(r'//.*', '', source)                    # plain HIP: no inline assembly
    for w in (1, 2, 4):
        assert f'batch<{w}>' in source                                    # the widths the entry point dispatches to
    state = open(os.path.join(CSRC, 'dcr_analysis.h')).read()
    assert all(f'hop_{b}' in state for b in ('bits', 'ctl', 'dist'))


# ---- the sparse reference of the 70,001- and 262,182-node tests ---------------------------------------------------------------------
@pytest.mark.parametrize('name', list(FIXTURES))
def test_sparse_reference_is_the_reference(name, solved):
    ei, n = FIXTURES[name]
    want = solved[name][0]
    src = np.concatenate([np.arange(n), [n - 1, 0, n // 2, 0]])                      # every node, then repeats: 16 is no divisor
    got = hops_ref.hops_sparse(ei, n, src)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w[src])
    none, e, r, t = hops_ref.hops_sparse(ei, n, src, rows=False)
    assert none is None and np.array_equal(e, want[1][src]) and np.array_equal(r, want[2][src]) and np.array_equal(t, want[3][src])
    for max_hops in (0, 1, 2, 7):
        some = src[::5]
        for g, w in zip(hops_ref.hops_sparse(ei, n, some, max_hops=max_hops), hops_ref.hops(ei, n, some, max_hops=max_hops)):
            assert np.array_equal(g, w)


def test_sparse_reference_is_scipy_at_70001_nodes():
    import scale_ref as sc
    ei, n = sc.whole_small()
    src = sc.hop_sources_small()[:6]                                                  # the long row, a medium row, node 0, isolated ones
    dist, ecc, reached, total = hops_ref.hops_sparse(ei, n, src)
    d = scipy.sparse.csgraph.shortest_path(spectral_ref.adjacency(ei, n), method='D', directed=False, unweighted=True, indices=src)
    want = np.where(np.isinf(d), -1, d).astype(np.int32)
    assert np.array_equal(dist, want)
    e, r, t = hops_ref.summaries_of(want)
    assert np.array_equal(ecc, e) and np.array_equal(reached, r) and np.array_equal(total, t)
    assert reached.tolist() == [n - 3, n - 3, n - 3, 1, 1, n - 3]
