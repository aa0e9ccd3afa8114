"""Node and edge betweenness centrality of a graph on the device, in networkx's scalings.  No counterpart in the reference.

The cuts, the spectrum, the commute times and the hop distances say how narrow a graph is and how far apart its nodes are; these
say WHICH edges and nodes carry the traffic.  A bottleneck in the sense of the over-squashing argument behind SDRF is an edge that
most shortest paths cross, and the negatively curved edges SDRF goes after are supposed to be those: the three rewirings (``sdrf``,
``digl``, ``fosr``) can be compared by how far they flatten the betweenness of the worst edges, before and after on one handle.
All of it comes from ``DcrGraph.betweenness`` (csrc/dcr_betweenness.hip: Brandes' algorithm, 16 sources a batch).

  betweenness_centrality(G, k=None, normalized=True, seed=0)        {'values': float64 [n], 'exact', 'num_sources', ...}
  edge_betweenness_centrality(G, k=None, normalized=True, seed=0)   {'edges': (eu, ev), 'values': float64 [E], 'exact', ...}
  scale_nodes(raw, n, normalized, k=None) / scale_edges(...)        the pure step from the device's raw sums to networkx's values

With ``k=None`` the values are those of ``networkx.betweenness_centrality(G, normalized=...)`` and
``networkx.edge_betweenness_centrality(G, normalized=...)`` for an undirected graph, endpoints not counted.  With ``k`` the sources
are ``hop_metrics.draw_sources(n, k, seed)`` and the sums are scaled by ``n / k`` as networkx scales a sample.  networkx draws
ITS sample with ``random.Random(seed).sample``, a different set of nodes: sampled values agree with networkx's in expectation
only, not value by value.  The dict says ``exact`` or not, as ``hop_metrics`` does.

Cost, honestly.  One batch of 16 sources is about 2 x (levels) sweeps of the adjacency: one per level forward, one per level back,
and the levels are the largest eccentricity of the batch.  All sources of a Cora-sized graph are 156 batches.  All sources of the
100,000-node bench graph are 6,250 batches: that is not what this is for; pass ``k`` there and read the values as estimates.
"""
import numpy as np

from experiment.hop_metrics import _graph, draw_sources


def scale_nodes(raw, n, normalized=True, k=None):
    """networkx's node values from the raw sums over the sources (ordered pairs where every node is a source): times
    ``1 / ((n - 1) (n - 2))`` normalised (unchanged for ``n <= 2``), times ``1 / 2`` otherwise; times ``n / k`` for a sample."""
    raw = np.asarray(raw, dtype=np.float64)
    scale = (1.0 / ((n - 1) * (n - 2)) if n > 2 else None) if normalized else 0.5
    if scale is None:
        return raw.copy()
    if k is not None:
        scale = scale * n / k
    return raw * scale


def scale_edges(raw, n, normalized=True, k=None):
    """networkx's edge values from the raw sums: times ``1 / (n (n - 1))`` normalised (unchanged for ``n <= 1``), times ``1 / 2``
    otherwise; times ``n / k`` for a sample."""
    raw = np.asarray(raw, dtype=np.float64)
    scale = (1.0 / (n * (n - 1)) if n > 1 else None) if normalized else 0.5
    if scale is None:
        return raw.copy()
    if k is not None:
        scale = scale * n / k
    return raw * scale


def _sources(n, k, seed):
    if k is None or k >= n:
        return None, None
    if k < 1:
        raise ValueError('k must be None or at least 1')
    return draw_sources(n, int(k), seed), int(k)


def betweenness_centrality(G, k=None, normalized=True, seed=0):
    """Node betweenness of a ``Data`` or a live ``DcrGraph`` as a dict: ``values`` float64 ``[n]`` in networkx's scaling,
    ``exact`` (every node was a source), ``num_sources``, ``normalized``, and ``levels_max`` / ``sigma_max`` of the device call
    (``sigma_max > 2 ** 53``: the path counts were rounded)."""
    G = _graph(G)
    n = G.number_of_nodes()
    src, k = _sources(n, k, seed)
    raw, info = G.betweenness(src, return_info=True)
    return {'values': scale_nodes(raw, n, normalized, k), 'exact': src is None, 'num_sources': n if src is None else int(src.size),
            'normalized': bool(normalized), 'levels_max': info['levels_max'], 'sigma_max': info['sigma_max']}


def edge_betweenness_centrality(G, k=None, normalized=True, seed=0):
    """Edge betweenness as a dict: ``edges`` = ``(eu, ev)`` in ``G.edges`` order, ``values`` float64 ``[E]`` in networkx's scaling,
    and the entries of ``betweenness_centrality``."""
    G = _graph(G)
    n = G.number_of_nodes()
    src, k = _sources(n, k, seed)
    _, (eu, ev, raw), info = G.betweenness(src, edges=True, return_info=True)
    return {'edges': (eu, ev), 'values': scale_edges(raw, n, normalized, k), 'exact': src is None,
            'num_sources': n if src is None else int(src.size), 'normalized': bool(normalized), 'levels_max': info['levels_max'],
            'sigma_max': info['sigma_max']}
