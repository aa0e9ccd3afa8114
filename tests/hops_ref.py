"""The hop-distance rule of include/dcr.h in numpy, frontier by frontier over the CSR adjacency: level 0 is the source, level L
the nodes with a neighbour in level L - 1 that are in no earlier level; the levels stop at max_hops.  Exact integers throughout.
tests/test_hops_cpu.py holds it against scipy and networkx; tests/test_hops_gpu.py compares the device with it by ==.  Also the
graphs both files use."""
import numpy as np

import spectral_ref


def csr(edge_index, n):
    a = spectral_ref.adjacency(edge_index, n)
    return a.indptr.astype(np.int64), a.indices.astype(np.int64)


def bfs(indptr, indices, n, source, max_hops=None):
    """(dist int32 [n] with -1 where not reached, ecc, reached, total) of one source."""
    dist = np.full(n, -1, dtype=np.int32)
    dist[source] = 0
    frontier = np.array([source], dtype=np.int64)
    ecc, reached, total, level = 0, 1, 0, 0
    while frontier.size and (max_hops is None or level < max_hops):
        level += 1
        starts, ends = indptr[frontier], indptr[frontier + 1]
        lens = ends - starts
        if lens.sum() == 0:
            break
        slots = np.repeat(starts - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(lens.sum())
        nb = np.unique(indices[slots])
        frontier = nb[dist[nb] < 0]
        if frontier.size == 0:
            break
        dist[frontier] = level
        ecc, reached, total = level, reached + int(frontier.size), total + level * int(frontier.size)
    return dist, ecc, reached, total


def hops(edge_index, n, sources=None, max_hops=None):
    """(dist int32 [P][n], ecc int32 [P], reached int64 [P], total int64 [P]); sources None: every node."""
    indptr, indices = csr(edge_index, n)
    src = np.arange(n) if sources is None else np.asarray(sources, dtype=np.int64)
    dist = np.empty((src.size, n), dtype=np.int32)
    ecc, reached, total = np.empty(src.size, dtype=np.int32), np.empty(src.size, dtype=np.int64), np.empty(src.size, dtype=np.int64)
    for i, s in enumerate(src):
        dist[i], ecc[i], reached[i], total[i] = bfs(indptr, indices, n, int(s), max_hops)
    return dist, ecc, reached, total


def hops_sparse(edge_index, n, sources, max_hops=None, rows=True):
    """hops() for graphs of hundreds of thousands of nodes: the scipy CSR adjacency, the sources in chunks of at most 16, a chunk's
    frontiers as one list of (source, node) entries that a level expands through the CSR rows all at once, and what has been
    seen as one boolean row per source.  A node that is a source several times is searched once.  No float array of [P, n] is
    made, and with rows=False no distance row either (dist is then None).  tests/test_hops_cpu.py holds it against hops() by ==
    on every small graph and against scipy's shortest paths at 70,001 nodes."""
    a = spectral_ref.adjacency(edge_index, n)
    indptr, indices = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    deg = np.diff(indptr)
    src, back = np.unique(np.asarray(sources, dtype=np.int64), return_inverse=True)
    P = src.size
    dist = np.full((P, n), -1, dtype=np.int32) if rows else None
    ecc, reached, total = np.zeros(P, dtype=np.int32), np.ones(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    for lo in range(0, P, 16):
        chunk = src[lo:lo + 16]
        k = chunk.size
        r, v = np.arange(k), chunk
        seen = np.zeros((k, n), dtype=bool)
        seen[r, v] = True
        if rows:
            dist[lo + r, v] = 0
        level = 0
        while r.size and (max_hops is None or level < max_hops):
            level += 1
            lens = deg[v]
            m = int(lens.sum())
            if m == 0:
                break
            slots = np.repeat(indptr[v] - (np.cumsum(lens) - lens), lens) + np.arange(m)
            nb, rr = indices[slots], np.repeat(r, lens)
            fresh = ~seen[rr, nb]
            key = np.unique(rr[fresh] * n + nb[fresh])       # a node may have several neighbours in the frontier
            r, v = key // n, key % n
            seen[r, v] = True
            if rows:
                dist[lo + r, v] = level
            count = np.bincount(r, minlength=k)
            ecc[lo:lo + k][count > 0] = level
            reached[lo:lo + k] += count
            total[lo:lo + k] += level * count
    return (dist[back] if rows else None), ecc[back], reached[back], total[back]


def summaries_of(dist):
    """(ecc, reached, total) read off distance rows."""
    seen = dist >= 0
    return (np.where(seen, dist, 0).max(axis=1).astype(np.int32), seen.sum(axis=1).astype(np.int64),
            np.where(seen, dist, 0).sum(axis=1, dtype=np.int64))


# ---- graphs ------------------------------------------------------------------------------------------------------------------------
def empty(n):
    return np.zeros((2, 0), dtype=np.int64), n


def union(*graphs):
    """The disjoint union, node ids shifted in order."""
    parts, off = [], 0
    for ei, n in graphs:
        parts.append(np.asarray(ei, dtype=np.int64) + off)
        off += n
    return np.concatenate(parts, axis=1), off


def hub_star(leaves=2100):
    """Node 0 joined to `leaves` leaves: one long row (above 2,048), the leaves short."""
    return spectral_ref.star(leaves + 1)


def irregular330():
    """330 nodes of mixed degrees in one component with two isolated nodes at the end (tests/fosr_ref.py::irregular_graph)."""
    import fosr_ref
    return fosr_ref.irregular_graph(330, seed=11, isolated=2)


def with_edge(edge_index, n, u, v, remove=False):
    """The edge list with {u, v} added (or removed)."""
    ei = np.asarray(edge_index, dtype=np.int64)
    keep = ~(((ei[0] == u) & (ei[1] == v)) | ((ei[0] == v) & (ei[1] == u)))
    ei = ei[:, keep]
    if not remove:
        ei = np.concatenate([ei, np.array([[u, v], [v, u]], dtype=np.int64)], axis=1)
    return ei, n


def degenerate():
    """(name, edge_index, n): the small and disconnected shapes."""
    p = spectral_ref.path
    return [('one_node', *empty(1)), ('two_nodes_no_edge', *empty(2)), ('two_nodes_edge', *p(2)), ('no_edges7', *empty(7)),
            ('isolated_among_connected', *union(p(5), empty(3), spectral_ref.cycle(6), empty(1))),
            ('two_components', *union(spectral_ref.barbell(4, 3), spectral_ref.star(9))),
            ('three_components', *union(p(40), spectral_ref.complete(6), spectral_ref.cycle(71)))]


def deep():
    return [('path300', *spectral_ref.path(300)), ('cycle257', *spectral_ref.cycle(257))]
