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
that the recorded figure still covers it); it is not tuned against the device."""
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
