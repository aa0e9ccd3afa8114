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


def csr_matvec_long(a, x):
    """a @ x in np.longdouble for a scipy CSR matrix: the products of a row added from left to right.  (scipy's own product stops
    at float64.)"""
    x = np.asarray(x, dtype=np.longdouble)
    out = np.zeros(a.shape[0], dtype=np.longdouble)
    if a.nnz:
        full = np.flatnonzero(np.diff(a.indptr) > 0)     # reduceat returns an element, not 0, for an empty row
        out[full] = np.add.reduceat(a.data.astype(np.longdouble) * x[a.indices], a.indptr[full])
    return out


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


# ---- the row plan of the analysis kernels, and graphs with planned class counts ------------------------------------------------
SHORT_DEG = 32     # csrc/dcr_analysis.h: SP_SHORT_DEG, rows up to this degree are short
LONG_DEG = 2048    # SP_LONG_DEG, rows above this degree are long (tests/test_row_classes_cpu.py reads both out of the source)


def row_plan(edge_index, n):
    """((n_long, n_mid, n_short), rows): what csrc/dcr_analysis.hip::classify_rows makes of the graph; rows holds the long rows,
    then the medium ones, then the short ones, each by node id."""
    _, deg = normalised_adjacency(edge_index, n)
    long_, short = deg > LONG_DEG, deg <= SHORT_DEG
    classes = [np.flatnonzero(long_), np.flatnonzero(~long_ & ~short), np.flatnonzero(short)]
    return tuple(int(c.size) for c in classes), np.concatenate(classes).astype(np.int32)


def planned_graph(hub_degrees, hub_edges=(), n_short=None, isolated=0, seed=0):
    """Hubs over shared leaves, as row_classes_graph: hub h has degree hub_degrees[h], of which its edges in hub_edges (pairs of
    hubs) come first and the rest go to the first leaves, so a leaf has the degree of the number of hubs that reach it.  Then
    `isolated` nodes, then as many filler nodes as make n_short short rows in all (every hub above SHORT_DEG): filler k hangs off
    leaf k % leaves.  The node ids are then permuted by Generator(PCG64(seed)), with the last isolated node moved to the highest id,
    the end of the short list.  Returns (edge_index, n, names): names maps 'hub0', ..., 'leaf_first', 'leaf_last' (the leaf of
    the smallest degree), 'isolated' (when there is one) to the permuted ids."""
    H = len(hub_degrees)
    to_leaves = [d - sum(h in e for e in hub_edges) for h, d in enumerate(hub_degrees)]
    L = max(to_leaves)
    assert min(hub_degrees) > SHORT_DEG and min(to_leaves) >= 1 and H < SHORT_DEG
    fillers = 0 if n_short is None else n_short - L - isolated
    assert fillers >= 0 and H + 1 + -(-fillers // L) <= SHORT_DEG, 'the leaves must stay short rows'
    n = H + L + isolated + fillers
    pairs = [tuple(e) for e in hub_edges]
    pairs += [(h, H + i) for h, d in enumerate(to_leaves) for i in range(d)]
    f0 = H + L + isolated
    pairs += [(f0 + k, H + k % L) for k in range(fillers)]
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(n)
    if isolated:
        last = H + L + isolated - 1
        at = int(np.flatnonzero(perm == n - 1)[0])
        perm[at], perm[last] = perm[last], perm[at]
    ei, _ = _und(perm[np.asarray(pairs, dtype=np.int64)], n)
    names = {f'hub{h}': int(perm[h]) for h in range(H)}
    names.update(leaf_first=int(perm[H]), leaf_last=int(perm[H + L - 1]))
    if isolated:
        names['isolated'] = int(perm[H + L + isolated - 1])
    return ei, n, names


def plan_family():
    """(name, edge_index, n) of graphs whose counts of long, medium and short rows sit at and either side of the limits of
    csrc/dcr_analysis.h::walk_rows and row_grid: a medium workgroup takes 4 rows, a short workgroup 32 (RowGeom<>) or 64 in 8
    turns of 8 (the resistance geometry).  tests/test_row_classes_cpu.py asserts what each graph is here for.  A graph has a long
    row only where the plan needs one: the others stay small."""
    return [(name, ei, n) for name, (ei, n, _) in _plan_family().items()]


def plan_nodes(name):
    """The named nodes of ONE graph of plan_family, as planned_graph returns them; {} for the two that are not hub graphs."""
    return _plan_family()[name][2]


# the graphs of plan_family, for parametrising without building them
PLAN_NAMES = ('long3_mid9_short63', 'long1_mid0_short0', 'mid1_short7', 'mid4_short8', 'mid5_short9', 'mid8_short1', 'mid34_short0',
              'mid0_short257')
_FAMILY = {}


def _plan_family():
    if _FAMILY:
        return _FAMILY
    M = LONG_DEG   # a medium row at the limit
    f = _FAMILY
    # three long workgroups, three medium ones (the last with one row), a partial last short workgroup in both geometries;
    # hub0 - hub1 joins two long rows, hub2 - hub3 a long and a medium one
    f['long3_mid9_short63'] = planned_graph([M + 1, M + 2, 2100, 33, M, 33, 34, 40, 64, 65, 100, 500], [(0, 1), (2, 3)],
                                            n_short=33 * 64 - 1, isolated=2, seed=1)
    f['long1_mid0_short0'] = planned_graph([M + 1], n_short=33 * 64, isolated=2, seed=2)     # long rows, no medium rows
    f['mid1_short7'] = planned_graph([33], n_short=64 + 7, isolated=2, seed=3)
    f['mid4_short8'] = planned_graph([33, 33, 35, 64], [(0, 1)], n_short=64 + 8, seed=4)
    f['mid5_short9'] = planned_graph([33, 34, 36, 38, 40], [(1, 4)], n_short=64 + 9, seed=5)
    f['mid8_short1'] = planned_graph([33, 33, 34, 35, 37, 41, 48, 48], [(0, 7), (2, 3)], n_short=64 + 1, isolated=2, seed=6)
    f['mid34_short0'] = complete(34) + ({},)     # no short rows at all
    f['mid0_short257'] = cycle(257) + ({},)      # no long and no medium rows; one row into the next workgroup, wave and turn
    assert tuple(f) == PLAN_NAMES
    return f


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
