"""Plain numpy restatement of DcrGraph.resistance_sketch (include/dcr.h has the rule), host only, graphs of a few thousand nodes:
the signs from the Philox family of tests/cheeger_ref.py, the right-hand sides b_j = B^T q_j, z_j = pinv(D - A) b_j through
resistance_ref.Dense, R~ for edges and pairs, and the same conjugate-gradient iteration column by column as resistance_ref.Dense.cg
runs it.  Nothing here imports the package under test.

The acceptance rule of tests/test_resistance_sketch_gpu.py.  With a_j = z_j[u] - z_j[v] of the reference, rho_j the true residual
of column j's solve, eps_j = rho_j / sqrt(lambda_1) and R~_ref = 1/k sum_j a_j^2:
    |R~ - R~_ref| <= 1/k sum_j (2 |a_j| eps_j sqrt(R~_ref) + eps_j^2 R~_ref) + ROUNDING_ALLOW max(1, R~_ref),
the first term from |c^T L'^+ r| <= sqrt(c^T L'^+ c) |r| / sqrt(lambda_1).  ROUNDING_ALLOW is 16 x ROUNDING_MEASURED, the largest
excess of the float64 CG replica below over that first term, relative to max(1, R~_ref), measured on the CPU over the graphs,
column counts of the GPU tests at tol 1e-6, 1e-12 and 1e-15 (tests/test_resistance_sketch_cpu.py measures it again and asserts
that the recorded figure still covers it); it is not tuned against the device.

For tens of thousands of nodes (tests/test_resistance_sketch_limits_gpu.py): sparse_diffs, a grounded sparse LU with its own error
e_a from two groundings; the windmill, whose differences have a closed form from pseudo-inverses of at most 5 x 5; cg_sparse, the
same iteration on a sparse operator; and the rounding term measured there (SCALE_ROUNDING_MEASURED)."""
import numpy as np

import cheeger_ref
import resistance_ref as ref

BATCH = 16
STREAM = 0x5253 << 48        # the Philox offset of batch b is STREAM | b

# measured by tests/test_resistance_sketch_cpu.py (float64 CG replica against pinv, beyond the residual bound): 2.363e-13, on
# barbell(20, 4) at k = 80 and tol 1e-15, where the gap of 2.8e-12 is the error of pinv itself (the same under any summation
# order of the replica) and the residual bound no longer hides it; below 4e-16 on the other three graphs
ROUNDING_MEASURED = 2.4e-13
ROUNDING_ALLOW = 16.0 * ROUNDING_MEASURED

# The same quantity at scale, for tests/test_resistance_sketch_limits_gpu.py: the sparse CG replica (cg_sparse) at tol 1e-12 against
# sparse_diffs (the windmill: against its closed form) over all edges and pairs_of(n) of the four large cases at their column
# counts, beyond the residual term with lam_lo of resistance_ref.lambda1_lower plus the e_a term, relative to max(1, R~_ref).
# Measured by tests/test_resistance_sketch_cpu.py: the largest excess is -1.918e-10, on diffusion_large() at k = 20 (-2.198e-10 on
# sketch_three_groups at k = 80, -2.268e-10 on sketch_two_groups at k = 48, -4.124e-10 on the windmill at k = 112).  It is negative:
# at tol 1e-12 the residual term is 1e-10 to 5e-9 on these graphs (residuals up to 1.8e-10, lam_lo 2e-3 to 2e-2) and the replica
# stays below a hundredth of it (largest gap / bound 1.0e-2), so nothing is left for rounding to explain and 16 x that allows
# nothing: the rule of the limit tests is the residual term plus the e_a term alone.
SCALE_ROUNDING_MEASURED = -1.9e-10
SCALE_ROUNDING_ALLOW = 16.0 * max(0.0, SCALE_ROUNDING_MEASURED)
# e_a, the largest difference between the two groundings of sparse_diffs over all columns, edges and pairs_of(n), per large graph
# (seed and columns of large_case): four and three units in the last place of differences up to 2
E_A_MEASURED = {'sketch_three_groups': 8.9e-16, 'sketch_two_groups': 8.9e-16, 'diffusion_large': 6.7e-16}
# Seen on the device (an MI355X; tests/test_resistance_sketch_limits_gpu.py prints them, nothing above was set from them): the
# largest gap / bound 3.3e-2 (barbell_20_4, k = 112, pairs, under ROUNDING_ALLOW); on the large graphs 7.8e-3, 9.5e-3 and 1.0e-2
# (edges of the three lattice graphs, the CPU replica's own figures), 1.3e-2 over the 32,798 solved pairs past the grid cap,
# 3.9e-3 on the windmill's edges and 1.1e-2 after the hub's row was relocated.


def batch_words(lo, hi, seed, batch):
    """uint64 [E]: output word 0 of philox4x32_10(index = lo | hi << 32, offset = STREAM | batch, seed) per edge."""
    offset = STREAM | int(batch)
    lo, hi = np.asarray(lo, dtype=np.uint64), np.asarray(hi, dtype=np.uint64)
    return cheeger_ref.philox4x32_10(lo, hi, np.uint64(offset & 0xFFFFFFFF), np.uint64(offset >> 32), seed & 0xFFFFFFFF,
                                     (seed >> 32) & 0xFFFFFFFF)[0]


def signs(edges, seed, first, count):
    """float64 [count, E] of +1 / -1: the sign of edge (lo, hi) in columns first .. first + count - 1 (bit 0: +1)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    q = np.empty((count, len(e)))
    cache = (None, None)
    for i in range(count):
        b, bit = divmod(first + i, BATCH)
        if cache[0] != b:
            cache = (b, batch_words(e[:, 0], e[:, 1], seed, b))
        q[i] = 1.0 - 2.0 * ((cache[1] >> np.uint64(bit)) & np.uint64(1)).astype(np.float64)
    return q


def rhs(edges, n, q):
    """float64 [k, n] of integers: b_j = B^T q_j, an edge leaving its smaller endpoint."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    b = np.zeros((q.shape[0], n))
    for j in range(q.shape[0]):
        np.add.at(b[j], e[:, 0], q[j])
        np.subtract.at(b[j], e[:, 1], q[j])
    return b


def batch_rhs(edge_index, n, seed, batch):
    """float64 [n, 16]: what dcr_resistance_sketch_rhs returns."""
    e = ref.edges(edge_index)
    return np.ascontiguousarray(rhs(e, n, signs(e, seed, BATCH * batch, BATCH)).T)


def cg_column(d, c, tol=1e-6, max_steps=20000):
    """(y, true residual, steps): the iteration of resistance_ref.Dense.cg on d.lap y = c from y = 0; an all-zero c takes no step."""
    y = np.zeros(d.n)
    r, p = c.copy(), c.copy()
    rr = cc = float(c @ c)
    steps = 0
    while cc > 0.0 and steps < max_steps:
        q = d.lap @ p
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
    return y, float(np.linalg.norm(c - d.lap @ y)), steps


class Sketch:
    """The k sign vectors of ``seed`` on one graph: edges [E, 2] (a < b, sorted), q [k, E], b [k, n] and the potentials z [k, n],
    by pinv or (``solver='cg'``) by the float64 CG replica with its residuals and steps."""

    def __init__(self, edge_index, n, columns, seed=0, dense=None, solver='pinv', tol=1e-6, max_steps=20000):
        self.d = dense if dense is not None else ref.Dense(edge_index, n)
        self.n, self.k = n, columns
        self.edges = ref.edges(edge_index)
        self.q = signs(self.edges, seed, 0, columns)
        self.b = rhs(self.edges, n, self.q)
        if solver == 'pinv':
            self.z = self.b @ self.d.pinv          # pinv is symmetric
            self.residual = self.steps = None
        else:
            out = [cg_column(self.d, self.d.s * self.b[j], tol, max_steps) for j in range(columns)]
            self.z = np.stack([self.d.s * y for y, _, _ in out])
            self.residual = np.array([r for _, r, _ in out])
            self.steps = np.array([s for _, _, s in out])

    def diffs(self, pairs):
        """float64 [k, P]: a_j = z_j[u] - z_j[v]."""
        pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        return self.z[:, pr[:, 0]] - self.z[:, pr[:, 1]]

    def values(self, pairs):
        """float64 [P]: R~; 0 for u == v, inf across components."""
        pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        r = (self.diffs(pr) ** 2).mean(axis=0)
        r = np.where(pr[:, 0] == pr[:, 1], 0.0, r)
        return np.where(self.d.labels[pr[:, 0]] != self.d.labels[pr[:, 1]], np.inf, r)

    def edge_values(self):
        return self.values(self.edges)


def residual_bound(a, residual, lambda1):
    """float64 [P]: 1/k sum_j (2 |a_j| eps_j sqrt(R~_ref) + eps_j^2 R~_ref) for a [k, P], eps_j = residual_j / sqrt(lambda_1)."""
    eps = (np.asarray(residual) / np.sqrt(lambda1))[:, None]
    r = (a ** 2).mean(axis=0)
    return (2.0 * np.abs(a) * eps * np.sqrt(r) + eps ** 2 * r).mean(axis=0)


def allow(r_ref):
    return ROUNDING_ALLOW * np.maximum(1.0, r_ref)


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------------
GENERAL = {'random300': ref.random_graph, 'barbell_20_4': lambda: ref.barbell(20, 4), 'cycle64': lambda: ref.cycle(64),
           'triangle_star_isolated': ref.triangle_star_isolated}
COLUMNS = (16, 20, 32, 80)   # one batch; padding columns; two batches; five batches, more than one launch of four groups


def pairs_of(n):
    """Twelve seeded pairs, then a node with itself twice and the first node with the last (across components where there are any)."""
    pr = np.random.default_rng(3).integers(0, n, size=(12, 2))
    return np.concatenate([pr, [(0, 0), (n - 1, n - 1), (0, n - 1)]])


# ---- references that do not grow with n^2: the cases of tests/test_resistance_sketch_limits_gpu.py ---------------------------------
class SparseOperator:
    """What cg_column reads of resistance_ref.Dense, with the normalised Laplacian as a scipy CSR matrix: n, s, lap, labels."""

    def __init__(self, edge_index, n):
        import scipy.sparse
        import scipy.sparse.csgraph
        self.n = n
        a = ref._sparse_adjacency(edge_index, n)
        self.deg = np.asarray(a.sum(axis=1)).ravel()
        self.s = np.zeros(n)
        self.s[self.deg > 0] = 1.0 / np.sqrt(self.deg[self.deg > 0])
        s = scipy.sparse.diags(self.s)
        self.lap = (scipy.sparse.diags((self.deg > 0).astype(np.float64)) - s @ a @ s).tocsr()
        self.count, self.labels = scipy.sparse.csgraph.connected_components(a, directed=False)


def cg_sparse(op, b, tol=1e-12, max_steps=20000):
    """(z [k, n], true residuals [k], steps [k]): cg_column, the same iteration, on the sparse operator for every row of b [k, n]."""
    out = [cg_column(op, op.s * b[j], tol, max_steps) for j in range(b.shape[0])]
    return np.stack([op.s * y for y, _, _ in out]), np.array([r for _, r, _ in out]), np.array([s for _, _, s in out])


def sparse_diffs(edge_index, n, b, pairs, ground='smallest'):
    """float64 [k, P]: a_j = z_j[u] - z_j[v] for (D - A) z_j = b_j, b [k, n] summing to zero on every component: component by
    component the grounded Laplacian by ``scipy.sparse.linalg.splu`` and one step of refinement with the defect formed in
    np.longdouble, as resistance_ref.sparse_resistance solves it; ``ground``: the component's 'smallest' or 'largest' id.  Inside
    a component the differences do not depend on the ground; across components they mean nothing and are NaN."""
    import scipy.sparse
    import scipy.sparse.csgraph
    import scipy.sparse.linalg
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    b = np.asarray(b, dtype=np.float64)
    a = ref._sparse_adjacency(edge_index, n)
    lap = (scipy.sparse.diags(np.asarray(a.sum(axis=1)).ravel()) - a).tocsr()
    _, labels = scipy.sparse.csgraph.connected_components(a, directed=False)
    z = np.zeros((n, b.shape[0]))
    sizes = np.bincount(labels)
    for comp in np.flatnonzero(sizes > 1):
        nodes = np.flatnonzero(labels == comp)
        g = nodes[0] if ground == 'smallest' else nodes[-1]
        keep = nodes[nodes != g]
        m = lap[keep][:, keep].tocsr()
        m.sort_indices()
        rhs = np.ascontiguousarray(b[:, keep].T)
        lu = scipy.sparse.linalg.splu(m.tocsc())
        x = lu.solve(rhs)
        defect = rhs.astype(np.longdouble) - ref._matvec_long(m, x.astype(np.longdouble))
        z[keep] = (x.astype(np.longdouble) + lu.solve(defect.astype(np.float64))).astype(np.float64)   # z[g] stays 0
    out = (z[pr[:, 0]] - z[pr[:, 1]]).T
    out[:, labels[pr[:, 0]] != labels[pr[:, 1]]] = np.nan
    return out


def ground_error(a_smallest, a_largest):
    """e_a: the largest |a(ground = smallest id) - a(ground = largest id)| over all columns and pairs."""
    return float(np.abs(a_smallest - a_largest).max())


def ground_term(a, e_a):
    """float64 [P]: 1/k sum_j (2 |a_j| e_a + e_a^2), what an error of e_a in every a_j can move R~_ref by."""
    return (2.0 * np.abs(a) * e_a + e_a ** 2).mean(axis=0)


# ---- a closed form without a linear solver: blades of at most five nodes on two centres ---------------------------------------------
# local edges of a blade; local node 0 is the centre (the wheel with the centre on its rim lists its hub as node 1).  Single edges,
# triangles, 4-cycles and K4 alone do not give the centre's row enough different values: a blade's currents are multiples of 1/3
# or 1/4 there, R~_ref is 1/k times a sum of k squares of such multiples, and however many blades there are it takes a few
# hundred values (371 among 2,000 such slots at k = 48).  Hence the diamonds (K4 less an edge, the centre at a node of degree 3 or
# 2: multiples of 1/8) and the blades of five nodes (pseudo-inverses of 5 x 5; multiples of 1/5, 1/11, 1/21, 1/24, ...).
BLADES = {'edge': [(0, 1)], 'triangle': [(0, 1), (0, 2), (1, 2)], 'cycle4': [(0, 1), (1, 2), (2, 3), (0, 3)],
          'k4': [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)], 'diamond3': [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)],
          'diamond2': [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)], 'cycle5': [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4)],
          'house_roof': [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (1, 4)], 'house_base': [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (2, 4)],
          'house_side': [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (0, 2)],
          'wheel_hub': [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4), (1, 4)],
          'wheel_rim': [(1, 0), (1, 2), (1, 3), (1, 4), (0, 2), (2, 3), (3, 4), (0, 4)],
          'k23': [(0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4)], 'k5': [(i, j) for i in range(5) for j in range(i + 1, 5)]}
# the first centre's row: 2,921 slots of blades and the bridge, above SP_LONG_DEG; the second centre: 42 blades, a medium row
WINDMILL_LONG = (('edge', 100), ('triangle', 150), ('cycle4', 150), ('k4', 100), ('diamond3', 100), ('diamond2', 100), ('cycle5', 100),
                 ('house_roof', 100), ('house_base', 100), ('house_side', 67), ('wheel_hub', 50), ('wheel_rim', 50), ('k23', 50), ('k5', 30))
WINDMILL_MID = tuple((kind, 3) for kind in BLADES)
WINDMILL_SMALL = (tuple((kind, 2) for kind in BLADES), tuple((kind, 1) for kind in BLADES))   # 143 nodes: pinned against pinv on the CPU
WINDMILL_COLUMNS = 112   # launches of 4 + 3 groups


def windmill(blades=(WINDMILL_LONG, WINDMILL_MID), seed=11):
    """Two centres joined by a bridge; centre i carries blades[i] = ((kind, count), ...), each blade sharing the centre alone
    with the rest of the graph.  The node ids are shuffled by default_rng(seed), so that a centre's row holds neighbours below
    and above it.  (edge_index, n, parts): parts is a list of (local edges, nodes int64 [count, blade nodes]) with the blade's
    centre in column 0, the bridge first, and parts of the first centre before those of the second."""
    total = 2 + sum(count * max(max(e) for e in BLADES[kind]) for side in blades for kind, count in side)
    parts, nxt = [([(0, 1)], np.array([[0, 1]], dtype=np.int64))], 2
    for centre, side in enumerate(blades):
        for kind, count in side:
            extra = max(max(e) for e in BLADES[kind])
            nodes = np.empty((count, extra + 1), dtype=np.int64)
            nodes[:, 0] = centre
            nodes[:, 1:] = nxt + np.arange(count * extra).reshape(count, extra)
            nxt += count * extra
            parts.append((BLADES[kind], nodes))
    assert nxt == total
    perm = np.random.default_rng(seed).permutation(total)
    low = int(np.flatnonzero(perm == total // 16)[0])         # the first centre gets a low id: k_sketch_accumulate keeps an edge at
    perm[[0, low]] = perm[[low, 0]]                           # the slot of its smaller endpoint, so 15 in 16 of its slots are its own
    parts =[(loc, perm[nodes]) for loc, nodes in parts]
    pairs = np.concatenate([np.stack([nodes[:, i], nodes[:, j]], axis=1) for loc, nodes in parts for i, j in loc])
    ei, n = ref._und(pairs, total)
    return ei, n, parts


def windmill_centres(parts):
    return int(parts[0][1][0, 0]), int(parts[0][1][0, 1])


def windmill_potentials(n, parts, seed, columns):
    """float64 [k, n]: z_j up to a constant per column, with the first centre at 0.  The unit current between two nodes of a
    blade flows inside it, so on a blade z_j = pinv(L_blade) B_blade^T q_blade + const: one pseudo-inverse of at most 5 x 5 per
    kind of blade, and the constants follow from the centres (the first at 0, the second through the bridge)."""
    phi = np.zeros((columns, n))
    c0, c1 = windmill_centres(parts)
    for loc, nodes in parts:
        m = nodes.shape[1]
        lap = np.zeros((m, m))
        for i, j in loc:
            lap[i, i] += 1.0
            lap[j, j] += 1.0
            lap[i, j] -= 1.0
            lap[j, i] -= 1.0
        pinv = np.linalg.pinv(lap, hermitian=True)
        b = np.zeros((columns, nodes.shape[0], m))
        for i, j in loc:
            u, v = nodes[:, i], nodes[:, j]
            lo, hi = np.minimum(u, v), np.maximum(u, v)
            q = signs(np.stack([lo, hi], axis=1), seed, 0, columns)            # [k, count]
            out = np.where(u < v, 1.0, -1.0) * q                               # the edge leaves its smaller endpoint
            b[:, :, i] += out
            b[:, :, j] -= out
        d = b @ pinv                                                           # [k, count, m]
        d -= d[:, :, :1]                                                       # relative to the blade's centre
        centre = nodes[0, 0]
        base = phi[:, centre].copy()[:, None, None] if centre == c1 else 0.0   # the bridge came first: phi[c1] is final
        phi[:, nodes[:, 1:]] = base + d[:, :, 1:]
    return phi


def windmill_diffs(n, parts, seed, columns, pairs):
    """float64 [k, P]: a_j = z_j[u] - z_j[v] of the closed form; inside a blade the blade's own term, across blades the
    differences to the centres added along the path."""
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    phi = windmill_potentials(n, parts, seed, columns)
    return phi[:, pr[:, 0]] - phi[:, pr[:, 1]]


def distinct_values(values, apart):
    """How many of ``values`` lie more than ``apart`` from the next smaller one, plus one: a lower count of distinct values."""
    return int((np.diff(np.sort(values)) > apart).sum()) + 1


# ---- the large cases, computed once for the CPU and the GPU tests --------------------------------------------------------------------
class Case:
    """One graph of the limit tests with its reference: e [E, 2] (ref.edges order), pairs = e then pairs_of(n), solved (neither
    u == v nor across components), a [k, solved] from sparse_diffs (or the windmill's closed form), e_a, lam_lo, the long row."""

    def __init__(self, name, ei, n, k, seed, hub, parts=None):
        self.name, self.ei, self.n, self.k, self.seed, self.hub, self.parts = name, ei, n, k, seed, hub, parts
        self.e = ref.edges(ei)
        self.pairs = np.concatenate([self.e, pairs_of(n)])
        self.op = SparseOperator(ei, n)
        self.labels = self.op.labels
        self.solved = (self.pairs[:, 0] != self.pairs[:, 1]) & (self.labels[self.pairs[:, 0]] == self.labels[self.pairs[:, 1]])
        self.b = rhs(self.e, n, signs(self.e, seed, 0, k))
        self.a, self.e_a = self.diffs(self.pairs[self.solved])
        self.lam_lo = ref.lambda1_lower(ei, n, hub)[0]
        self.hub_edges = np.flatnonzero((self.e[:, 0] == hub) | (self.e[:, 1] == hub))   # all solved: indices into a as well
        self.hub_kept = np.flatnonzero(self.e[:, 0] == hub)   # those k_sketch_accumulate adds up in the long row itself (hub < x)

    def diffs(self, pairs):
        """(a [k, P], e_a) for pairs inside components."""
        if self.parts is not None:
            return windmill_diffs(self.n, self.parts, self.seed, self.k, pairs), 0.0
        a = sparse_diffs(self.ei, self.n, self.b, pairs, 'smallest')
        return a, ground_error(a, sparse_diffs(self.ei, self.n, self.b, pairs, 'largest'))

    def replica(self):
        """(R~ [solved], true residuals [k], steps [k]) of the float64 CG replica at tol 1e-12, computed once."""
        if not hasattr(self, '_replica'):
            z, resid, steps = cg_sparse(self.op, self.b, tol=1e-12)
            pr = self.pairs[self.solved]
            self._replica = ((z[:, pr[:, 0]] - z[:, pr[:, 1]]) ** 2).mean(axis=0), resid, steps
        return self._replica

    def bound(self, residual, a=None, e_a=None):
        """The rule of tests/test_resistance_sketch_limits_gpu.py without its rounding term."""
        a = self.a if a is None else a
        return residual_bound(a, residual, self.lam_lo) + ground_term(a, self.e_a if e_a is None else e_a)


# the seed of the signs per large graph: the smallest one at which the hub row's 2,100 reference values lie more than 150 bounds
# apart pairwise, with the float64 CG replica's residuals in the bound (tests/test_scale_thresholds_cpu.py asserts 100; a
# condition on the reference alone, so that no two slots of the long row can be exchanged unseen).  2,100 values in a range of
# about 1 come as close as 1e-7 at most seeds and a bound there is 1e-9 to 3e-9: the ratios are 208, 247 and 170 at these seeds,
# and 70, 247 and 38 at seed 0.
LARGE_SEEDS = {'sketch_three_groups': 10, 'sketch_two_groups': 0, 'diffusion_large': 81}
_CASES = {}


def large_case(name):
    """'sketch_three_groups', 'sketch_two_groups', 'diffusion_large' (scale_ref.SKETCH_LARGE) or 'windmill'."""
    if name not in _CASES:
        if name == 'windmill':
            ei, n, parts = windmill()
            _CASES[name] = Case(name, ei, n, WINDMILL_COLUMNS, 0, windmill_centres(parts)[0], parts)
        else:
            import scale_ref
            build, k, _ = scale_ref.SKETCH_LARGE[name]
            ei, n, names = build()
            _CASES[name] = Case(name, ei, n, k, LARGE_SEEDS[name], names['hub0'])
    return _CASES[name]


LARGE_CASES = ('sketch_three_groups', 'sketch_two_groups', 'diffusion_large', 'windmill')
