"""Dense numpy restatement of what DcrGraph.effective_resistance computes (host only, graphs of a few thousand nodes at most):
R(u, v) = (e_u - e_v)^T pinv(D - A) (e_u - e_v), the spectral gap lambda_1 of the normalised Laplacian by ``eigvalsh``, and the
same conjugate-gradient iteration as csrc/dcr_resistance.hip, column by column: on L' = I - D^-1/2 A D^-1/2 with
c = s_u e_u - s_v e_v from y = 0, returning ``lower = 2 c.y - y.L'y`` and the true residual ``|c - L'y|``.  For tens of thousands
of nodes: ``sparse_resistance`` (grounded Laplacian, sparse LU) and ``lambda1_lower`` (shift-invert Lanczos).  Nothing here imports
the package under test."""
import numpy as np

EPS = 2.0 ** -52


# ---- graphs ------------------------------------------------------------------------------------------------------------------
def _und(pairs, n):
    """Edge index [2, 2E] with both directions, sorted by (source, target)."""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ei = np.concatenate([p.T, p.T[::-1]], axis=1)
    order = np.lexsort((ei[1], ei[0]))
    return ei[:, order], n


def path(n):
    return _und([(i, i + 1) for i in range(n - 1)], n)


def cycle(n):
    return _und([(i, (i + 1) % n) for i in range(n)], n)


def star(n):
    """Centre 0 and n - 1 leaves."""
    return _und([(0, i) for i in range(1, n)], n)


def complete(n):
    return _und([(i, j) for i in range(n) for j in range(i + 1, n)], n)


def barbell(k, p):
    """K_k, a path of p nodes, K_k, numbered as networkx.barbell_graph numbers them."""
    left = [(i, j) for i in range(k) for j in range(i + 1, k)]
    chain = [(i, i + 1) for i in range(k - 1, k + p)]
    right = [(i, j) for i in range(k + p, 2 * k + p) for j in range(i + 1, 2 * k + p)]
    return _und(left + chain + right, 2 * k + p)


def random_graph(n=300, seed=5):
    """Connected: every node v >= 1 is linked to two earlier nodes drawn by default_rng(seed) (one link where the two coincide)."""
    rng = np.random.default_rng(seed)
    edges = set()
    for v in range(1, n):
        for w in rng.integers(0, v, size=2):
            edges.add((int(w), v))
    return _und(sorted(edges), n)


def triangle_star_isolated():
    """Nine nodes, three components: the triangle 0-1-2, the star with centre 3 and leaves 4..7, the isolated node 8."""
    return _und([(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (3, 6), (3, 7)], 9)


def hub_with_tail(leaves=2100):
    """A star of `leaves` leaves (centre 0, leaves 1..leaves) and a path of three nodes hanging off leaf 1."""
    t = leaves + 1
    return _und([(0, i) for i in range(1, leaves + 1)] + [(1, t), (t, t + 1), (t + 1, t + 2)], leaves + 4)


# ---- dense quantities ----------------------------------------------------------------------------------------------------------
def adjacency(edge_index, n):
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    a = np.zeros((n, n))
    a[ei[0], ei[1]] = 1.0
    a[ei[1], ei[0]] = 1.0
    np.fill_diagonal(a, 0.0)
    return a


def edges(edge_index):
    """The undirected edges a < b as [E, 2], sorted."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    lo, hi = np.minimum(ei[0], ei[1]), np.maximum(ei[0], ei[1])
    return np.unique(np.stack([lo, hi], axis=1)[lo != hi], axis=0)


def components(edge_index, n):
    """(count, labels): the label of a node is the smallest node id of its component."""
    lab = np.arange(n)
    e = edges(edge_index)
    for _ in range(n):
        new = lab.copy()
        np.minimum.at(new, e[:, 0], lab[e[:, 1]])
        np.minimum.at(new, e[:, 1], lab[e[:, 0]])
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return int(np.unique(lab).size), lab


class Dense:
    """pinv(D - A), the degrees, the components and lambda_1 of one graph, computed once."""

    def __init__(self, edge_index, n):
        self.n = n
        self.a = adjacency(edge_index, n)
        self.deg = self.a.sum(axis=1)
        self._pinv = None
        self.count, self.labels = components(edge_index, n)
        self.s = np.zeros(n)
        self.s[self.deg > 0] = 1.0 / np.sqrt(self.deg[self.deg > 0])
        self.lap = np.diag((self.deg > 0).astype(np.float64)) - self.s[:, None] * self.a * self.s[None, :]
        lam = np.linalg.eigvalsh(self.lap)
        self.lambda1 = float(lam[self.count]) if self.count < n else float('nan')

    @property
    def pinv(self):
        # np.linalg.pinv(hermitian=True) with the null space cut by its known dimension, one eigenvalue per component, where
        # numpy cuts at 1e-15 max|w|: with a hub of degree 2,049 a zero eigenvalue came out as -4.9e-12, above that cut-off,
        # and its reciprocal put 3e-8 into the resistances (tests/test_row_classes_gpu.py has the graph)
        if self._pinv is None:
            w, v = np.linalg.eigh(np.diag(self.deg) - self.a)
            keep = np.sort(np.argsort(np.abs(w), kind='stable')[self.count:])
            self._pinv = (v[:, keep] / w[keep]) @ v[:, keep].T
        return self._pinv

    def resistance(self, pairs):
        """float64 [P]: 0 for u == v, inf across components."""
        pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        u, v = pr[:, 0], pr[:, 1]
        r = self.pinv[u, u] + self.pinv[v, v] - 2.0 * self.pinv[u, v]
        r = np.where(u == v, 0.0, r)
        return np.where(self.labels[u] != self.labels[v], np.inf, r)

    def cg(self, u, v, tol=1e-10, max_steps=20000):
        """(lower, residual, steps) of one pair: the iteration of csrc/dcr_resistance.hip."""
        if u == v:
            return 0.0, 0.0, 0
        if self.labels[u] != self.labels[v]:
            return float('inf'), 0.0, 0
        c = np.zeros(self.n)
        c[u], c[v] = self.s[u], -self.s[v]
        y = np.zeros(self.n)
        r, p = c.copy(), c.copy()
        rr = cc = float(c @ c)
        steps = 0
        while steps < max_steps:
            q = self.lap @ p
            pq = float(p @ q)
            if not (pq > 0.0 and np.isfinite(pq)):
                break
            alpha = rr / pq
            y += alpha * p
            r -= alpha * q
            new = float(r @ r)
            beta = new / rr
            rr = new
            steps += 1
            if not np.isfinite(rr) or np.sqrt(rr) <= tol * np.sqrt(cc):
                break
            p = r + beta * p
        w = self.lap @ y
        return float(2.0 * (c @ y) - y @ w), float(np.linalg.norm(c - w)), steps

    def curvature(self):
        """(p, edges [E, 2], kappa): p_u = 1 - 1/2 sum_{v ~ u} R_uv, kappa_uv = 2 (p_u + p_v) / R_uv."""
        e = edges(np.stack(np.nonzero(self.a)))
        r = self.resistance(e)
        p = np.ones(self.n)
        np.subtract.at(p, e[:, 0], 0.5 * r)
        np.subtract.at(p, e[:, 1], 0.5 * r)
        return p, e, 2.0 * (p[e[:, 0]] + p[e[:, 1]]) / r


# ---- without a dense matrix: the reference of tests/test_resistance_gpu.py at 33,000 nodes -----------------------------------------
def _sparse_adjacency(edge_index, n):
    import scipy.sparse
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    ei = ei[:, ei[0] != ei[1]]
    a = scipy.sparse.coo_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n)).tocsr()
    a = a + a.T
    a.data[:] = 1.0
    return a


def _matvec_long(m, x):
    """m @ x in np.longdouble for a scipy CSR matrix with no empty row, x [k, columns]."""
    prod = m.data.astype(np.longdouble)[:, None] * x[m.indices]
    return np.add.reduceat(prod, m.indptr[:-1], axis=0)


def sparse_resistance(edge_index, n, pairs, ground='smallest'):
    """float64 [P]: R(u, v) from the grounded Laplacian, component by component.  In a component C with the node g removed
    (``ground``: its 'smallest' or its 'largest' id), L_g = (D - A)[C - g, C - g] is positive definite and x = L_g^-1 (e_u - e_v),
    with x_g = 0 and the entry of g dropped from the right-hand side, gives R = x_u - x_v.  ``scipy.sparse.linalg.splu``, then one
    step of refinement with the residual e_u - e_v - L_g x formed in np.longdouble.  0 for u == v, inf across components."""
    import scipy.sparse.csgraph
    import scipy.sparse.linalg
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    a = _sparse_adjacency(edge_index, n)
    lap = (scipy.sparse.diags(np.asarray(a.sum(axis=1)).ravel()) - a).tocsr()
    _, labels = scipy.sparse.csgraph.connected_components(a, directed=False)
    out = np.where(pr[:, 0] == pr[:, 1], 0.0, np.inf)
    todo = np.flatnonzero((pr[:, 0] != pr[:, 1]) & (labels[pr[:, 0]] == labels[pr[:, 1]]))
    for comp in np.unique(labels[pr[todo, 0]]):
        mine = todo[labels[pr[todo, 0]] == comp]
        nodes = np.flatnonzero(labels == comp)
        g = nodes[0] if ground == 'smallest' else nodes[-1]
        keep = nodes[nodes != g]
        at = np.full(n, -1, dtype=np.int64)          # position in the grounded system; -1: the ground
        at[keep] = np.arange(keep.size)
        m = lap[keep][:, keep].tocsr()
        m.sort_indices()
        rhs = np.zeros((keep.size, mine.size))
        for col, (u, v) in enumerate(pr[mine]):
            if at[u] >= 0:
                rhs[at[u], col] += 1.0
            if at[v] >= 0:
                rhs[at[v], col] -= 1.0
        lu = scipy.sparse.linalg.splu(m.tocsc())
        x = lu.solve(rhs)
        defect = rhs.astype(np.longdouble) - _matvec_long(m, x.astype(np.longdouble))
        x = (x.astype(np.longdouble) + lu.solve(defect.astype(np.float64))).astype(np.float64)
        x = np.concatenate([x, np.zeros((1, mine.size))])   # at == -1 reads the ground's 0
        cols = np.arange(mine.size)
        out[mine] = x[at[pr[mine, 0]], cols] - x[at[pr[mine, 1]], cols]
    return out


def lambda1_lower(edge_index, n, node):
    """(lam_lo, theta, ritz_residual): a lower bound of lambda_1 of the normalised Laplacian I - D^-1/2 A D^-1/2 of the component
    of ``node``.  ``scipy.sparse.linalg.eigsh`` in shift-invert mode just below 0 returns the two Ritz pairs nearest the shift: the
    null vector D^1/2 1 and (theta, w).  Some eigenvalue lies within |L' w - theta w| / |w| of theta, the residual evaluated with
    a plain sparse product; lam_lo = theta - that residual."""
    import scipy.sparse.csgraph
    import scipy.sparse.linalg
    a = _sparse_adjacency(edge_index, n)
    _, labels = scipy.sparse.csgraph.connected_components(a, directed=False)
    nodes = np.flatnonzero(labels == labels[node])
    a = a[nodes][:, nodes].tocsr()
    s = scipy.sparse.diags(1.0 / np.sqrt(np.asarray(a.sum(axis=1)).ravel()))
    lap = (scipy.sparse.identity(nodes.size) - s @ a @ s).tocsc()
    v0 = np.random.Generator(np.random.PCG64(1)).standard_normal(nodes.size)
    vals, vecs = scipy.sparse.linalg.eigsh(lap, k=2, sigma=-1e-3, which='LM', v0=v0, tol=1e-12)
    order = np.argsort(vals)
    theta, w = float(vals[order[1]]), vecs[:, order[1]]
    assert abs(vals[order[0]]) <= 1e-10 < theta, vals     # one null vector in a component, and theta is not it
    resid = float(np.linalg.norm(lap @ w - theta * w) / np.linalg.norm(w))
    return theta - resid, theta, resid


def allow(n, r_ref):
    """The rounding allowance of the acceptance rule: 64 n 2^-52 max(1, R_ref)."""
    return 64.0 * n * EPS * np.maximum(1.0, r_ref)
