"""Effective resistance of node pairs and the resistance curvature, on the device-resident graph.  No counterpart in the reference.

The Cheeger estimate, the spectral bracket and the sweep cut (``compute_cheeger.py``, ``cheeger_bounds.py``) give one number per
graph.  SDRF acts locally: it adds an edge across the most negatively curved one and removes the most positively curved one.  The
per-pair quantity that says how much closer two nodes have become is the effective resistance
``R(u, v) = (e_u - e_v)^T L^+ (e_u - e_v)``, ``L = D - A``: the commute time between u and v divided by 2 E, and the quantity the
over-squashing bounds of the literature after SDRF are written in.

  effective_resistance(data, pairs)   R of each pair (``DcrGraph.effective_resistance``: csrc/dcr_resistance.hip, conjugate
                                      gradients on the normalised Laplacian, 16 pairs per sweep of the adjacency)
  edge_resistances(data)              (eu, ev, R) over ``G.edges()``.  Foster: they sum to n - c, c the connected components
  resistance_curvature(data)          (p, eu, ev, kappa): the node curvature p_u = 1 - 1/2 sum_{v ~ u} R_uv and the link curvature
                                      kappa_uv = 2 (p_u + p_v) / R_uv of Devriendt and Lambiotte; sum_u p_u = c
  resistance_upper(lower, residual, gap)   the other side of the bracket around a returned value
  sketch_relative_std(columns)        sqrt(2 / columns): the relative standard deviation ``method='sketch'`` stays within

With the default ``method='cg'`` every returned resistance is a LOWER bound, ``lower = 2 c^T y - y^T L' y`` for the iterate y the
solver stopped at, with ``L' = I - D^-1/2 A D^-1/2`` and ``c = D^-1/2 (e_u - e_v)``: R - lower = (y* - y)^T L' (y* - y) >= 0 for
any y, so also when ``max_steps`` cut the solve short.  ``resistance_upper`` closes the bracket from the solver's true residual.

``edge_resistances`` and ``resistance_curvature`` also take ``method='sketch'`` (``DcrGraph.resistance_sketch``:
csrc/dcr_resistance_sketch.hip): the estimator of Spielman and Srivastava with k = ``columns`` Rademacher sign vectors q_j on the
edges, ``R~(u, v) = 1/k sum_j (z_j[u] - z_j[v])^2`` with ``L z_j = B^T q_j``.  It is unbiased, NOT a bound: each value has a relative
standard deviation of at most sqrt(2 / k) (12.5 % at k = 128, 8.8 % at the default 256, 4.4 % at 1,024), the sum over the edges
has mean n - c and a standard deviation of at most sqrt(2 (n - c) / k), and a bridge comes out as 1 whatever the signs.  ``seed``
fixes the signs, which are keyed by an edge's endpoints: the same edge draws the same signs before and after a rewiring.

Cost, honestly.  ``method='cg'``: a batch of 16 pairs costs one conjugate-gradient solve, about sqrt(2 / lambda_1) ln(1 / tol)
sweeps of the adjacency, lambda_1 the spectral gap, three kernel launches a sweep.  All edges of a Cora-sized graph (5,000 edges:
320 batches of a few dozen steps) are a second or so; all edges of the 1 M-edge bench graph would be 65,000 batches, which is not
what it is for.  ``method='sketch'``: k / 16 batches whatever the number of edges (16 at the default k = 256, solved at ``tol`` =
1e-6, since the solve only has to sit well below sqrt(2 / k)), plus two sweeps of the adjacency a batch for the right-hand sides
and the squared differences: the route for every edge of a large graph, and for taking the curvature before and after a
rewiring.  tools/probe_resistance_sketch.py times both routes; DESIGN §4.8 has what it measured.
"""
import numpy as np

SOLVER = {'tol', 'max_steps'}


def _graph(data):
    from dcr.graph import DcrGraph
    return data if isinstance(data, DcrGraph) else DcrGraph.from_data(data)


def _check(opts):
    unknown = set(opts) - SOLVER
    if unknown:
        raise TypeError(f'unknown solver arguments: {sorted(unknown)}')


def effective_resistance(data, pairs, **opts):
    """float64 ``[P]``: the effective resistance of each pair of ``pairs`` (array-like ``[P, 2]``); 0 for u == v, inf across components.
    :param data: a ``Data``, or a live ``DcrGraph``.
    :param opts: ``tol``, ``max_steps`` and ``return_info`` of ``DcrGraph.effective_resistance``.
    """
    _check({k: v for k, v in opts.items() if k != 'return_info'})
    return _graph(data).effective_resistance(pairs, **opts)


def sketch_relative_std(columns):
    """``sqrt(2 / columns)``: the bound on the relative standard deviation of every value ``method='sketch'`` returns."""
    if columns < 1:
        raise ValueError('columns must be >= 1')
    return float(np.sqrt(2.0 / columns))


def edge_resistances(data, method='cg', columns=256, seed=0, **opts):
    """``(eu, ev, R)``: the resistance of every edge, in ``G.edges()`` order.  They sum to n - c (Foster).
    :param method: ``'cg'``, a solve per edge and a lower bound each; ``'sketch'``, ``columns`` solves for all edges together and
        an unbiased estimate each, within ``sketch_relative_std(columns)`` (``columns`` and ``seed`` are read by it alone).
    """
    _check(opts)
    G = _graph(data)
    if method == 'sketch':
        return G.resistance_sketch(columns=columns, seed=seed, **opts)
    if method != 'cg':
        raise ValueError(f"method must be 'cg' or 'sketch', not {method!r}")
    eu, ev = G.edges()
    return eu, ev, G.effective_resistance(np.stack([eu, ev], axis=1), **opts)


def resistance_curvature(data, method='cg', columns=256, seed=0, **opts):
    """``(p, eu, ev, kappa)``: p float64 ``[n]``, p_u = 1 - 1/2 sum_{v ~ u} R_uv accumulated in edge order (1 on an isolated
    node; sum_u p_u = c), and kappa float64 ``[E]``, kappa_uv = 2 (p_u + p_v) / R_uv, in ``G.edges()`` order.  ``method``,
    ``columns`` and ``seed`` as in ``edge_resistances``: with ``'sketch'`` sum_u p_u is c only up to the deviation
    sqrt(2 (n - c) / columns) of the sum of the edge values."""
    G = _graph(data)
    eu, ev, R = edge_resistances(G, method=method, columns=columns, seed=seed, **opts)
    p = np.ones(G.number_of_nodes(), dtype=np.float64)
    np.subtract.at(p, eu, 0.5 * R)
    np.subtract.at(p, ev, 0.5 * R)
    return p, eu, ev, 2.0 * (p[eu] + p[ev]) / R


def resistance_upper(lower, residual, gap):
    """``lower + residual ** 2 / gap``: an upper bound of the resistance whose solve returned ``lower`` with true residual
    ``residual``.  With r = c - L' y and y* the solution, y* - y = L'^+ r (both sides orthogonal to the null space of L'), so
    R - lower = (y* - y)^T L' (y* - y) = r^T L'^+ r <= |r|^2 / lambda_1.  ``gap`` must be a LOWER bound of lambda_1, the smallest
    positive eigenvalue of the normalised Laplacian on the pair's component; the whole graph's lambda_1 (``DcrGraph.spectral_gap``)
    serves for every component with an edge, being the minimum over them.  Note that a Lanczos value is never below the true
    lambda_1: subtract its residual, or use a known bound, where a certificate is wanted."""
    return np.asarray(lower, dtype=np.float64) + np.asarray(residual, dtype=np.float64) ** 2 / gap
