"""The betweenness rule of include/dcr.h in numpy: Brandes' algorithm for unweighted graphs as csrc/dcr_betweenness.hip runs it,
pull-style and level by level over the CSR of spectral_ref.adjacency, a column per source.

  forward, level L    mask = dist[row] == -1 & dist[col] == L - 1 over the slots (row -> col); sigma[row] = the masked sum of
                      sigma[col] and dist[row] = L where a slot matched
  backward, level l   mask = dist[row] == l & dist[col] == l + 1; delta[row] = sigma[row] * the masked sum of
                      (1 + delta[col]) / sigma[col]; the slot adds sigma[row] (1 + delta[col]) / sigma[col] to its edge
  closing             node[v] += sum of delta[v] over the columns, the column of a source left out at the source

A level only looks at the slots that can match: those whose col lies in the frontier, which by the symmetry of the adjacency are
the rows of the frontier's nodes read the other way round.  The values are the raw sums over the sources (ordered pairs where
every node is a source: twice networkx's unnormalised undirected value).  tests/test_betweenness_cpu.py holds it against
networkx; tests/test_betweenness_gpu.py compares the device with it.  Also the tolerance and the graphs both files use."""
import numpy as np
import scipy.sparse

import hops_ref
import spectral_ref

U = 2.0 ** -53
CHUNK = 16     # columns at a time (csrc/dcr_betweenness.hip: BTW_B); the values do not depend on it


def _expand(indptr, indices, front):
    """(col, row) of every slot row -> col with col in `front` (sorted nodes): the rows of the front's nodes, mirrored."""
    lens = indptr[front + 1] - indptr[front]
    m = int(lens.sum())
    slots = np.repeat(indptr[front] - (np.cumsum(lens) - lens), lens) + np.arange(m)
    return np.repeat(front, lens), indices[slots]


def _sum_by(keys, values):
    """(the distinct keys in ascending order, the rows of `values` added per key in their order of appearance)."""
    order = np.argsort(keys, kind='stable')
    k = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    return k[starts], np.add.reduceat(values[order], starts, axis=0)


def betweenness(edge_index, n, sources=None, edges=False):
    """(node float64 [n], edge values as a scipy CSR matrix M or None, info).  The value of the edge {u, v} is M[u, v] + M[v, u]
    (edge_values); info has levels_max and sigma_max.  sources None: every node; a duplicated source counts twice."""
    a = spectral_ref.adjacency(edge_index, n)
    indptr, indices = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    src = np.arange(n, dtype=np.int64) if sources is None else np.asarray(sources, dtype=np.int64).reshape(-1)
    node = np.zeros(n)
    parts = []
    info = {'levels_max': 0, 'sigma_max': 1.0 if src.size else 0.0}
    for lo in range(0, src.size, CHUNK):
        s = src[lo:lo + CHUNK]
        B = s.size
        cols = np.arange(B)
        dist = np.full((n, B), -1, dtype=np.int32)
        sigma, delta = np.zeros((n, B)), np.zeros((n, B))
        dist[s, cols], sigma[s, cols] = 0, 1.0
        levels = []     # per level L the slots (row, col) of which one column matched
        front = np.unique(s)
        while front.size:
            L = len(levels) + 1
            col, row = _expand(indptr, indices, front)
            mask = (dist[row] == -1) & (dist[col] == L - 1)
            keep = mask.any(axis=1)
            if not keep.any():
                break
            row, col, mask = row[keep], col[keep], mask[keep]
            rows, sums = _sum_by(row, np.where(mask, sigma[col], 0.0))
            r, c = np.nonzero(sums > 0.0)              # sigma >= 1 wherever a slot matched
            dist[rows[r], c] = L
            sigma[rows[r], c] = sums[r, c]
            levels.append((col, row))                  # read the other way round on the way back
            front = rows
        for l in range(len(levels) - 1, -1, -1):
            row, col = levels[l]
            mask = (dist[row] == l) & (dist[col] == l + 1)
            t = np.where(mask, (1.0 + delta[col]) / np.where(mask, sigma[col], 1.0), 0.0)
            rows, acc = _sum_by(row, t)
            r, c = np.nonzero(dist[rows] == l)
            delta[rows[r], c] = sigma[rows[r], c] * acc[r, c]
            if edges:
                parts.append((row, col, np.where(mask, sigma[row] * t, 0.0).sum(axis=1)))
        info['levels_max'] = max(info['levels_max'], len(levels))
        info['sigma_max'] = max(info['sigma_max'], float(sigma.max()))
        delta[s, cols] = 0.0
        node += delta.sum(axis=1)
    M = None
    if edges:
        r = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, dtype=np.int64)
        c = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, dtype=np.int64)
        e = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0)
        M = scipy.sparse.coo_matrix((e, (r, c)), shape=(n, n)).tocsr()
    return node, M, info


def edge_values(M, eu, ev):
    """The values of the edges {eu[i], ev[i]}."""
    eu, ev = np.asarray(eu, dtype=np.int64), np.asarray(ev, dtype=np.int64)
    if eu.size == 0:
        return np.zeros(0)
    return np.asarray(M[eu, ev]).ravel() + np.asarray(M[ev, eu]).ravel()


def undirected_edges(edge_index):
    """(eu, ev) with eu < ev, each edge once, sorted."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    lo, hi = np.minimum(ei[0], ei[1]), np.maximum(ei[0], ei[1])
    pairs = np.unique(np.stack([lo, hi], axis=1), axis=0) if lo.size else np.zeros((0, 2), dtype=np.int64)
    return pairs[:, 0], pairs[:, 1]


# ---- the tolerance -----------------------------------------------------------------------------------------------------------------
def rtol(edge_index, n, levels_max, num_sources):
    """Every summand is non-negative, so a value's relative error is at most k u with k = 2 D (maxdeg + 3) + S, u = 2^-53: D the
    largest level count + 1, S the number of sources; sigma contributes D maxdeg, delta D (maxdeg + 3), the sum over the sources
    S.  The same bound holds for either side of a comparison (a factor 2), and another 2 covers the second-order terms."""
    deg = np.bincount(np.asarray(edge_index, dtype=np.int64).reshape(2, -1)[0], minlength=n)
    k = 2 * (levels_max + 1) * (int(deg.max(initial=0)) + 3) + num_sources
    return 4 * k * U


def assert_close(got, want, tol, what=''):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    bad = err > tol * np.abs(want)
    assert not bad.any(), (what, int(bad.sum()), float((err / np.maximum(np.abs(want), 1e-300)).max()), tol)


# ---- graphs ------------------------------------------------------------------------------------------------------------------------
def diamonds(k):
    """A chain of k diamonds: a_0, then per diamond the two middle nodes and a_(i + 1); node 3 i is a_i.  The number of shortest
    paths from a_0 to a_i is 2^i."""
    pairs = []
    for i in range(k):
        a, b, c, d = 3 * i, 3 * i + 1, 3 * i + 2, 3 * i + 3
        pairs += [(a, b), (a, c), (b, d), (c, d)]
    return spectral_ref._und(pairs, 3 * k + 1)


def plan_sources(name):
    """48 sources of the plan_family graph `name`: the largest-degree node, then nodes drawn by Generator(PCG64), three of them
    given twice."""
    ei, n = plan_graph(name)
    deg = np.bincount(np.asarray(ei)[0], minlength=n)
    rng = np.random.Generator(np.random.PCG64(len(name)))
    drawn = rng.choice(n, size=min(44, n), replace=False)
    src = np.concatenate([[int(np.argmax(deg))], drawn, drawn[:3]])
    return np.resize(src, 48).astype(np.int32)


def plan_graph(name):
    return next((ei, n) for nm, ei, n in spectral_ref.plan_family() if nm == name)


def boundary_sources(P, n):
    """P sources of irregular330: the two isolated nodes at the end, node 0 and a duplicate of each among them."""
    base = np.array([n - 1, 0, 0, n - 2, 17, n - 1, 5, 120, 17, 300, 44, 9, 201, 77, 3, 150, 260, 0, 88, 199, 31, 12, 250, 66, 101, 8, 311,
                     42, 170, 23, 290, 55, n - 2], dtype=np.int32)
    return base[:P]


def cases():
    """(name, edge_index, n, sources) of every graph tests/test_betweenness_gpu.py uses below the scale test; sources None: all."""
    out = [(name, ei, n, None) for name, ei, n in hops_ref.degenerate()]
    out += [('path300', *spectral_ref.path(300), None), ('cycle257', *spectral_ref.cycle(257), None), ('cycle64', *spectral_ref.cycle(64), None),
            ('hub_star2100', *hops_ref.hub_star(2100), None), ('irregular330', *hops_ref.irregular330(), None),
            ('diamonds60', *diamonds(60), np.array([0, 180, 90], dtype=np.int32))]
    out += [(name, *plan_graph(name), plan_sources(name)) for name in spectral_ref.PLAN_NAMES]
    return out


def scale_case():
    """16 sources of scale_ref.whole_small(): 70,001 nodes, more than a thousand workgroups of the row kernels and a second trip of
    the capped element-wise kernel."""
    import scale_ref
    ei, n = scale_ref.whole_small()
    return ei, n, scale_ref.hop_sources_small()[:16]
