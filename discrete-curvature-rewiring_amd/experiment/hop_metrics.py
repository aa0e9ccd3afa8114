"""Hop-distance metrics of a graph on the device: diameter, radius, average shortest-path length, eccentricities and ball sizes.
No counterpart in the reference.

The cuts, the spectrum and the commute times (``compute_cheeger.py``, ``cheeger_bounds.py``, ``effective_resistance.py``) say how
narrow a graph is; these say how far apart its nodes are and how fast a receptive field grows, the quantities the over-squashing
papers start from (SDRF's bottleneck theorem is stated for nodes at distance r + 1).  All of it comes from
``DcrGraph.hop_summary`` (csrc/dcr_hops.hip: breadth-first search from up to 256 sources per sweep of the live adjacency), so a
graph can be measured before and after ``sdrf``, ``digl`` or ``fosr`` on the same handle.

  hop_metrics(G, sources=None, max_hops=None, seed=0)   the dict described there
  ball_sizes(G, r, sources=None)                        |B_r(v)|: the nodes within r hops of v, v included
  aggregate(ecc, reached, total, labels, sources)       the pure step from the per-source summaries to the dict

Everything is an exact integer except the one division of the average.

Cost, honestly.  A batch of 256 sources costs one sweep of the adjacency per level, and there are as many levels as the largest
eccentricity of the batch.  All sources of a Cora-sized graph are ten batches.  All sources of the 100,000-node bench graph are
391 batches of 256 (1,563 at 64): that is not what this is for; pass ``sources=k`` there and read the diameter as a lower bound
and the average as an estimate.
"""
import numpy as np


def _graph(data):
    from dcr.graph import DcrGraph
    return data if isinstance(data, DcrGraph) else DcrGraph.from_data(data)


def draw_sources(n, k, seed=0):
    """``k`` distinct nodes of ``0 .. n - 1`` (all of them where ``k >= n``), sorted, drawn by ``Generator(PCG64(seed))``."""
    if k >= n:
        return np.arange(n, dtype=np.int32)
    return np.sort(np.random.Generator(np.random.PCG64(seed)).choice(n, size=int(k), replace=False)).astype(np.int32)


def aggregate(ecc, reached, total, labels, sources=None):
    """The dict of ``hop_metrics`` from the per-source summaries.  ``labels`` int ``[n]``: a component label per node (any labels;
    ``DcrGraph.connected_components`` gives the smallest node id).  ``sources``: the node of each summary, ``None`` for every node
    in order.  The largest component is the one with the most nodes, among equals the one with the smallest label.  Pure: no
    device, no graph."""
    ecc, reached, total = np.asarray(ecc), np.asarray(reached, dtype=np.int64), np.asarray(total, dtype=np.int64)
    labels = np.asarray(labels)
    n = labels.shape[0]
    src = np.arange(n) if sources is None else np.asarray(sources, dtype=np.int64)
    if not (ecc.shape == reached.shape == total.shape == src.shape):
        raise ValueError('ecc, reached, total and sources must have one entry per source')
    exact = bool(n > 0 and np.array_equal(np.unique(src), np.arange(n)))
    out = {'eccentricity': ecc, 'reached': reached, 'exact': exact, 'num_sources': int(src.size),
           'diameter': None, 'radius': None, 'average_path_length': float('nan'), 'largest_component': 0}
    if n:
        values, sizes = np.unique(labels, return_counts=True)
        largest = values[np.argmax(sizes)]            # argmax takes the first maximum: the smallest label among equals
        out['largest_component'] = int(sizes.max())
    if src.size:
        out['diameter'] = int(ecc.max())
        inside = labels[src] == largest
        if inside.any():
            out['radius'] = int(ecc[inside].min())
            pairs = int((reached[inside] - 1).sum())
            out['average_path_length'] = float(total[inside].sum()) / pairs if pairs else 0.0
    return out


def hop_metrics(G, sources=None, max_hops=None, seed=0):
    """Distance metrics of a ``Data`` or a live ``DcrGraph``.  Returns a dict:

      diameter             the largest eccentricity of a source: the largest finite distance, so on a disconnected graph the
                           largest diameter of a component (networkx raises there)
      radius               the smallest eccentricity among the sources of the largest component; ``None`` where none lies in it
      average_path_length  sum of ``total`` over sum of ``reached - 1``, over the sources of the largest component: with every
                           node a source, ``networkx.average_shortest_path_length`` of that component (0.0 for a single node;
                           nan where no source lies in it)
      eccentricity, reached  per source, as ``DcrGraph.hop_summary`` returns them
      exact                True when every node was a source
      largest_component, num_sources

    ``sources``: ``None`` for every node, an array of nodes, or an int ``k``: ``k`` distinct nodes drawn by
    ``np.random.Generator(PCG64(seed))``.  With a sample the diameter is a LOWER bound (a maximum over fewer sources), the radius
    an UPPER bound, and the average an estimate: the mean over the sampled sources' rows, each row exact.  With ``max_hops`` every
    quantity is that of the distances up to the limit only."""
    G = _graph(G)
    n = G.number_of_nodes()
    if isinstance(sources, (int, np.integer)) and not isinstance(sources, bool):
        sources = draw_sources(n, int(sources), seed)
    ecc, reached, total = G.hop_summary(sources, max_hops=max_hops)
    labels = G.connected_components()[1]
    return aggregate(ecc, reached, total, labels, sources)


def ball_sizes(G, r, sources=None):
    """int64 ``[len(sources)]`` (every node for ``None``): ``|B_r(v)|``, the number of nodes within ``r`` hops of ``v``, ``v``
    included: ``reached`` of ``DcrGraph.hop_summary`` at ``max_hops=r``."""
    return _graph(G).hop_summary(sources, max_hops=int(r))[1]
