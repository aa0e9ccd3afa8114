"""The two triangle curvatures of curvature/classical_curvatures.py:17-27 restated in plain numpy, from an edge index alone:

    'augmented'  4 - deg(u) - deg(v) + 3 T(u, v)          'haantjes'  T(u, v)

with T the number of common neighbours of the edge's endpoints.  Nothing of the library and nothing of oracle/ is used: this
is the second, independent reference behind tests/test_tri_incremental_gpu.py (tests/test_tri_ref_cpu.py holds it against the
reference's recorded values and against the C oracle).  Values are float64 of exact integers, in ``G.edges()`` order.

``G.edges()`` of networkx walks the nodes in order and, for each, its adjacency row in insertion order, giving an edge at the
first endpoint it meets: (u, v) with u < v, ordered by u, then by v's position in u's row.  Two ways to state the rows:
  * ``edges_of_input``: an edge index as ``to_networkx(data, to_undirected=True)`` reads it (sdrf_no_cuda.py:20): the pairs
    with dst <= src, in order, each appended to both rows (a repeated pair keeps its first position, a self-loop is none);
  * ``edges_of_rows``: an edge index that already lists the rows (``from_networkx(G).edge_index``, what ``to_edge_index()``
    of a live graph exports: row 0, row 1, ...): the pairs with src < dst in the order they stand.
"""
import numpy as np

KINDS = ('augmented', 'haantjes')


def edges_of_input(edge_index, num_nodes):
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    rows = [[] for _ in range(num_nodes)]
    seen = set()
    for u, v in zip(ei[0].tolist(), ei[1].tolist()):
        if v >= u or (u, v) in seen:         # (v == u: the library refuses self-loops; none in any fixture)
            continue
        seen.add((u, v))
        rows[u].append(v)
        rows[v].append(u)
    eu, ev = [], []
    for u, row in enumerate(rows):
        for v in row:
            if v > u:
                eu.append(u)
                ev.append(v)
    return np.array(eu, dtype=np.int32), np.array(ev, dtype=np.int32)


def edges_of_rows(edge_index):
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    assert np.all(np.diff(ei[0]) >= 0), 'not a list of rows'
    keep = ei[0] < ei[1]
    return ei[0, keep].astype(np.int32), ei[1, keep].astype(np.int32)


def common_neighbours(eu, ev, num_nodes):
    """T per edge of the simple undirected graph whose edges are (eu, ev), from the sorted adjacency: for every edge, each
    neighbour w of its lower-degree endpoint a is looked up in the sorted list of directed pairs as (w, b).  The work is the sum
    over the edges of the smaller degree, so a hub of 17,000 leaves costs what its leaves cost."""
    eu = np.asarray(eu, dtype=np.int64)
    ev = np.asarray(ev, dtype=np.int64)
    if eu.size == 0:
        return np.zeros(0, dtype=np.int64)
    n = int(num_nodes)
    src, dst = np.concatenate([eu, ev]), np.concatenate([ev, eu])
    keys = np.sort(src * n + dst)                       # every directed pair, sorted: row u is keys[start[u]:start[u + 1]] - u n
    assert np.all(np.diff(keys) > 0), 'repeated edge'
    start = np.searchsorted(keys, np.arange(n + 1, dtype=np.int64) * n)
    deg = np.diff(start)
    a = np.where(deg[eu] <= deg[ev], eu, ev)
    b = eu + ev - a
    reps = deg[a]
    edge = np.repeat(np.arange(eu.size), reps)          # one entry per (edge, neighbour of a)
    first = np.cumsum(reps) - reps
    w = keys[start[a][edge] + (np.arange(edge.size) - first[edge])] - a[edge] * n
    probe = w * n + b[edge]
    at = np.minimum(np.searchsorted(keys, probe), keys.size - 1)
    return np.bincount(edge[keys[at] == probe], minlength=eu.size).astype(np.int64)


def common_neighbours_scipy(eu, ev, num_nodes):
    """The same integers as (A @ A) masked by A, read at the edges (needs scipy; for graphs without large hubs)."""
    import scipy.sparse as sp
    eu = np.asarray(eu, dtype=np.int64)
    ev = np.asarray(ev, dtype=np.int64)
    one = np.ones(2 * eu.size, dtype=np.int64)
    A = sp.csr_matrix((one, (np.concatenate([eu, ev]), np.concatenate([ev, eu]))), shape=(num_nodes, num_nodes))
    P = (A @ A).multiply(A).tocsr()                     # paths of length two between adjacent nodes
    return np.asarray(P[eu, ev]).ravel().astype(np.int64)


def values(eu, ev, num_nodes, kind):
    """float64 curvature of every edge (eu[i], ev[i]) of the graph these edges make up."""
    if kind not in KINDS:
        raise ValueError(kind)
    T = common_neighbours(eu, ev, num_nodes)
    if kind == 'haantjes':
        return T.astype(np.float64)
    deg = np.bincount(np.concatenate([eu, ev]).astype(np.int64), minlength=num_nodes)
    return (4 - deg[eu] - deg[ev] + 3 * T).astype(np.float64)


def curv_all(edge_index, num_nodes, kind, rows=False):
    """(eu, ev, values) in ``G.edges()`` order; ``rows``: the edge index lists the adjacency rows of a live graph."""
    eu, ev = edges_of_rows(edge_index) if rows else edges_of_input(edge_index, num_nodes)
    return eu, ev, values(eu, ev, num_nodes, kind)
