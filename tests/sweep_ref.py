"""Numpy restatement of the sweep cut as include/dcr.h states it (host only): the order is a lexsort by (score, node id) with -0.0
taken as +0.0, the counts of every prefix come from difference arrays and a cumsum, the value is one float64 division of exact
integers.  ``brute`` counts every prefix by explicit set membership instead, for graphs of a dozen nodes."""
from collections import namedtuple

import numpy as np

Sweep = namedtuple('Sweep', ['value', 'size', 'counts', 'order', 'profile'])


def undirected_edges(edge_index, num_nodes=None):
    """(a, b) with a < b, each undirected edge once, by (a, b).  The rows of np.unique(axis=0) are the definition; with num_nodes
    given (and a * num_nodes + b within int64) the same arrays come from a sort of that key: tests/test_sweep_cpu.py has the
    equality."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    lo, hi = np.minimum(ei[0], ei[1]), np.maximum(ei[0], ei[1])
    keep = lo < hi
    if num_nodes is not None and 0 < num_nodes < 2 ** 31 and keep.any() and hi.max() < num_nodes:
        key = np.unique(lo[keep] * np.int64(num_nodes) + hi[keep])
        return key // num_nodes, key % num_nodes
    pairs = np.unique(np.stack([lo[keep], hi[keep]], axis=1), axis=0) if keep.any() else np.zeros((0, 2), dtype=np.int64)
    return pairs[:, 0], pairs[:, 1]


def order_of(score):
    score = np.asarray(score, dtype=np.float64)
    if np.isnan(score).any():
        raise ValueError('NaN in the score')
    return np.lexsort((np.arange(score.shape[0]), np.where(score == 0, 0.0, score)))


def values(n_in, n_lo, n_hi, num_edges, definition):
    n_in, n_lo, n_hi = (np.asarray(x, dtype=np.int64) for x in (n_in, n_lo, n_hi))
    n_out = num_edges - n_in - n_lo - n_hi
    if definition == 'reference':
        cut, small = n_lo, np.minimum(2 * n_in, 2 * n_out)
    elif definition == 'conductance':
        cut, small = n_lo + n_hi, np.minimum(2 * n_in + n_lo + n_hi, 2 * n_out + n_lo + n_hi)
    else:
        raise ValueError(definition)
    out = np.full(cut.shape, np.inf)
    ok = small > 0
    out[ok] = cut[ok].astype(np.float64) / small[ok].astype(np.float64)
    return out


def _finish(order, n_in, n_lo, n_hi, num_edges, definition):
    profile = values(n_in, n_lo, n_hi, num_edges, definition)
    best = int(np.argmin(profile))
    counts = np.array([n_in[best], n_lo[best], n_hi[best], num_edges - n_in[best] - n_lo[best] - n_hi[best]], dtype=np.int64)
    return Sweep(float(profile[best]), best + 1, counts, order.astype(np.int32), profile)


def prefix_counts(edge_index, n, score):
    """(order, n_in, n_lo, n_hi of every prefix S_1 .. S_{n-1}, the number of edges): everything of a sweep that does not depend
    on the definition, so that a test of both definitions computes it once."""
    if n < 2:
        raise ValueError('a sweep needs two nodes')
    a, b = undirected_edges(edge_index, n)
    order = order_of(score)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    p, q = rank[a], rank[b]
    d = np.zeros((3, n + 2), dtype=np.int64)   # index k; S_k = the nodes of rank < k
    up = p < q
    np.add.at(d[1], p[up] + 1, 1)      # lo for k in [p + 1, q]
    np.add.at(d[1], q[up] + 1, -1)
    np.add.at(d[2], q[~up] + 1, 1)     # hi for k in [q + 1, p]
    np.add.at(d[2], p[~up] + 1, -1)
    np.add.at(d[0], np.maximum(p, q) + 1, 1)   # in from k = max + 1
    c = np.cumsum(d, axis=1)[:, 1:n]
    return order, c[0], c[1], c[2], a.shape[0]


def from_counts(counts, definition):
    return _finish(*counts, definition)


def sweep(edge_index, n, score, definition='conductance'):
    return from_counts(prefix_counts(edge_index, n, score), definition)


def brute(edge_index, n, score, definition='conductance'):
    a, b = undirected_edges(edge_index)
    order = order_of(score)
    n_in, n_lo, n_hi = [], [], []
    for k in range(1, n):
        S = set(order[:k].tolist())
        ia = np.array([x in S for x in a.tolist()], dtype=bool)
        ib = np.array([x in S for x in b.tolist()], dtype=bool)
        n_in.append(int((ia & ib).sum()))
        n_lo.append(int((ia & ~ib).sum()))
        n_hi.append(int((~ia & ib).sum()))
    return _finish(order, np.array(n_in), np.array(n_lo), np.array(n_hi), a.shape[0], definition)


def fiedler_score(edge_index, n):
    """(lambda_1, D^-1/2 y) from a dense eigh, y the eigenvector of the (c+1)-th smallest eigenvalue of the normalised Laplacian."""
    import scipy.linalg
    import spectral_ref
    c, _ = spectral_ref.components(edge_index, n)
    lam, vec = scipy.linalg.eigh(spectral_ref.laplacian(edge_index, n).toarray())
    _, deg = spectral_ref.normalised_adjacency(edge_index, n)
    s = np.zeros(n)
    s[deg > 0] = 1.0 / np.sqrt(deg[deg > 0])
    return float(lam[c]), s * vec[:, c]


def table_graphs():
    """(name, (edge_index, n), lambda_1 / 2, sweep conductance, best k or None, sqrt(2 lambda_1)) as printed in DESIGN §4.7."""
    import spectral_ref
    from dcr import synthetic
    return [
        ('barbell20_4', spectral_ref.barbell(20, 4), 5.14e-4, 1 / 385, 22, 4.53e-2),
        ('powerlaw300', synthetic.powerlaw_graph(300, 2, seed=3), 0.0926, 0.2088, None, 0.6087),
        ('grid12x9', synthetic.grid_graph(12, 9), 0.00985, 0.04615, 54, 0.1985),
        ('er200', synthetic.erdos_renyi_graph(200, 0.05, seed=1), 0.2101, 0.2990, None, 0.9168),
    ]
