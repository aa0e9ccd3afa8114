"""Dense numpy / scipy restatement of what DcrGraph.spectral_gap computes (host only, for graphs of a few thousand nodes):
the normalised adjacency from an edge index, the connected components, and the (c+1)-th smallest eigenvalue of
L = I - D^-1/2 A D^-1/2, c the number of components.  An isolated node has D^-1/2 = 0 (its row of L is zero), as
networkx.normalized_laplacian_matrix has it."""
import numpy as np
import scipy.linalg
import scipy.sparse
import scipy.sparse.csgraph

EPS = 2.0 ** -52


def adjacency(edge_index, n):
    """Symmetric 0/1 scipy CSR matrix of the undirected simple graph of an edge index [2, M] (either or both directions)."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    a = scipy.sparse.coo_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n)).tocsr()
    a = a + a.T
    a.data[:] = 1.0
    return a


def normalised_adjacency(edge_index, n):
    """(Â as scipy CSR, degrees)."""
    a = adjacency(edge_index, n)
    deg = np.asarray(a.sum(axis=1)).ravel()
    s = np.zeros(n)
    s[deg > 0] = 1.0 / np.sqrt(deg[deg > 0])
    d = scipy.sparse.diags(s)
    return (d @ a @ d).tocsr(), deg


def laplacian(edge_index, n):
    """L = I - Â as scipy CSR, with zero rows at isolated nodes."""
    ahat, deg = normalised_adjacency(edge_index, n)
    return (scipy.sparse.diags((deg > 0).astype(np.float64)) - ahat).tocsr()


def components(edge_index, n):
    """(count, labels): the label of a node is the smallest node id of its component."""
    c, lab = scipy.sparse.csgraph.connected_components(adjacency(edge_index, n), directed=False)
    smallest = np.full(c, n, dtype=np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    return int(c), smallest[lab].astype(np.int32)


def eigenvalues(edge_index, n):
    return scipy.linalg.eigh(laplacian(edge_index, n).toarray(), eigvals_only=True)


def lambda1(edge_index, n):
    """The (c+1)-th smallest eigenvalue of L."""
    c, _ = components(edge_index, n)
    lam = eigenvalues(edge_index, n)
    if c >= n:
        raise ValueError('no positive eigenvalue')
    return float(lam[c])


def null_vectors(edge_index, n):
    """[c, n]: the orthonormal null vectors of L, D^1/2 1_C / sqrt(vol C) per component with an edge and e_v per isolated v."""
    _, deg = normalised_adjacency(edge_index, n)
    _, lab = components(edge_index, n)
    out = []
    for root in np.unique(lab):
        k = np.where(lab == root, np.sqrt(deg), 0.0)
        if not k.any():
            k[root] = 1.0
        out.append(k / np.linalg.norm(k))
    return np.array(out)


def bound(residual, n):
    """|Ritz value - eigenvalue| <= residual, plus the dense reference's own backward error 8 n eps at |L| <= 2."""
    return residual + 8 * n * EPS


def bounds_strings(lam):
    return f'{lam / 2: .2e}', f'{np.sqrt(2 * lam): .2e}'


# ---- graphs with a closed-form gap -----------------------------------------------------------------------------------------
def _und(pairs, n):
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ei = np.concatenate([p.T, p.T[::-1]], axis=1)
    order = np.lexsort((ei[1], ei[0]))
    return ei[:, order], n


def path(n):
    return _und([(i, i + 1) for i in range(n - 1)], n)


def cycle(n):
    return _und([(i, (i + 1) % n) for i in range(n)], n)


def complete(n):
    return _und([(i, j) for i in range(n) for j in range(i + 1, n)], n)


def star(n):
    return _und([(0, i) for i in range(1, n)], n)


def hypercube(d):
    return _und([(v, v ^ (1 << b)) for v in range(1 << d) for b in range(d) if v < v ^ (1 << b)], 1 << d)


def barbell(m1, m2):
    """Two K_m1 joined by a path of m2 nodes, numbered as networkx.barbell_graph numbers them."""
    left = [(i, j) for i in range(m1) for j in range(i + 1, m1)]
    chain = [(i, i + 1) for i in range(m1 - 1, m1 + m2)]
    right = [(i, j) for i in range(m1 + m2, 2 * m1 + m2) for j in range(i + 1, 2 * m1 + m2)]
    return _und(left + chain + right, 2 * m1 + m2)


def row_classes_graph():
    """Rows on both sides of both degree limits of the kernels that walk the rows by class (32 and 2,048), in three components:
    hubs 0..3 of degree 32, 33, 2,048 and 2,049, not adjacent to each other, each joined to the first d of the 2,049 leaves
    4..2052 (a leaf has degree 1 to 4); the triangle 2053-2054-2055; the isolated node 2056."""
    hubs = (32, 33, 2048, 2049)
    pairs = [(h, 4 + i) for h, d in enumerate(hubs) for i in range(d)]
    t = 4 + max(hubs)
    return _und(pairs + [(t, t + 1), (t, t + 2), (t + 1, t + 2)], t + 4)


def closed_forms():
    """(name, (edge_index, n), lambda_1)"""
    return [
        ('path200', path(200), 1 - np.cos(np.pi / 199)),
        ('path7', path(7), 1 - np.cos(np.pi / 6)),
        ('cycle9', cycle(9), 1 - np.cos(2 * np.pi / 9)),
        ('cycle300', cycle(300), 1 - np.cos(2 * np.pi / 300)),
        ('complete5', complete(5), 5 / 4),
        ('complete40', complete(40), 40 / 39),
        ('star6', star(6), 1.0),
        ('star500', star(500), 1.0),
        ('hypercube3', hypercube(3), 2 / 3),
        ('hypercube8', hypercube(8), 2 / 8),
        ('two_nodes', path(2), 2.0),
    ]
