"""Numpy restatement of FoSR as include/dcr.h defines it (host only, small graphs): the power step, the pick as the rule states it
(per node, naively over the eligible nodes), the dense brute-force minimum over the free pairs, the loop free-running or
replaying a given sequence of picks, and the vectors the tests try the pick with."""
import numpy as np

import spectral_ref


def degrees_and_rows(edge_index, n):
    """(scipy CSR adjacency, degrees as int64, the neighbour set of every node)."""
    a = spectral_ref.adjacency(edge_index, n)
    deg = np.diff(a.indptr).astype(np.int64)
    rows = [set(a.indices[a.indptr[v]:a.indptr[v + 1]].tolist()) for v in range(n)]
    return a, deg, rows


# ---- the power step ------------------------------------------------------------------------------------------------------------
def power_step(a, deg, x):
    """One step on x, or None where |z| is 0 or not finite (the loop stops there)."""
    d = deg.astype(np.float64)
    r = np.sqrt(d)
    s = np.zeros_like(d)
    s[deg > 0] = 1.0 / np.sqrt(d[deg > 0])
    x = x - (np.dot(x, r) / d.sum()) * r
    z = x + s * (a @ (s * x))
    nrm = np.sqrt(np.dot(z, z))
    if not (nrm > 0 and np.isfinite(nrm)):
        return None
    return z / nrm


def power_step_long(a, deg, x):
    """power_step with every operation in np.longdouble; the result in np.longdouble.  What the float64 restatement is compared
    with to learn its own rounding."""
    L = np.longdouble
    d = deg.astype(L)
    r = np.sqrt(d)
    s = np.zeros_like(d)
    s[deg > 0] = L(1) / np.sqrt(d[deg > 0])
    x = np.asarray(x, dtype=L)
    x = x - (np.sum(x * r) / d.sum()) * r
    z = x + s * spectral_ref.csr_matvec_long(a, s * x)
    return z / np.sqrt(np.sum(z * z))


def own_rounding(a, deg, x0, steps):
    """The largest elementwise difference between `steps` power steps in float64 and the same in np.longdouble: the reference
    against itself."""
    x, xl = np.asarray(x0, dtype=np.float64), np.asarray(x0, dtype=np.longdouble)
    for _ in range(steps):
        x, xl = power_step(a, deg, x), power_step_long(a, deg, xl)
    return float(np.abs(x - xl).max())


# ---- the pick ------------------------------------------------------------------------------------------------------------------
def y_of(x, deg):
    return np.asarray(x, dtype=np.float64) / np.sqrt(deg + 1.0)


def order_of(y):
    return np.lexsort((np.arange(y.shape[0]), np.where(y == 0, 0.0, y)))


def row_products(y, rows):
    """p(u) and partner(u) of every node by the rule, written out: the first eligible node of the order, the last for y_u < 0;
    partner -1 and p = +inf where nothing is eligible (or the product is NaN)."""
    n = y.shape[0]
    order = order_of(y)
    p, partner = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    for u in range(n):
        for v in (order[::-1] if y[u] < 0 else order):
            if v != u and v not in rows[u]:
                prod = y[u] * y[v]
                if prod == prod:
                    p[u], partner[u] = prod, v
                break
    return p, partner


def row_products_fast(y, a):
    """row_products from the CSR adjacency `a` with array operations.  Counted from its end of the order (the top for y_u < 0), a
    row of degree d has itself and its neighbours on d + 1 distinct ranks, so the first rank that none of them has is the number of
    them that sit on the ranks 0, 1, ... without a gap: sorted by (row, rank), the entries whose rank equals their place in the row."""
    n = y.shape[0]
    order = order_of(y)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    deg = np.diff(a.indptr).astype(np.int64)
    top = y < 0
    row = np.concatenate([np.repeat(np.arange(n), deg), np.arange(n)])          # every neighbour, then the row itself
    q = rank[np.concatenate([a.indices.astype(np.int64), np.arange(n)])]
    q = np.where(top[row], n - 1 - q, q)
    near = q < deg[row] + 2
    key = np.sort(row[near] * np.int64(n + 1) + q[near])
    row, q = key // (n + 1), key % (n + 1)
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=start[1:])
    free = np.bincount(row[q == np.arange(key.shape[0]) - start[row]], minlength=n)   # the first free rank of every row
    has = deg < n - 1
    at = np.where(top, n - 1 - free, free)
    partner = np.where(has, order[np.where(has, at, 0)], -1)
    with np.errstate(invalid='ignore'):
        p = np.where(has, y * y[np.maximum(partner, 0)], np.inf)
    nan = p != p
    p[nan], partner[nan] = np.inf, -1
    return p, partner


def pick_of(p, partner):
    if not (partner >= 0).any():
        return None
    best = p[partner >= 0].min()
    u = int(np.flatnonzero((partner >= 0) & (p == best))[0])
    return u, int(partner[u]), float(p[u])


def pick(y, rows):
    """(u, partner(u), p(u)) of the smallest p(u), the smallest u among equal values; None where no node has a partner."""
    return pick_of(*row_products(y, rows))


def margin_of(y, p, partner):
    got = pick_of(p, partner)
    if got is None:
        return np.inf
    u, v, best = got
    others = (partner >= 0) & (np.arange(y.shape[0]) != u) & (np.arange(y.shape[0]) != v)
    if not others.any():
        return np.inf
    return float((p[others].min() - best) / np.max(np.abs(y)) ** 2)


def runner_up_margin(y, rows):
    """How far the pick is from the next best choice, relative to max |y|^2.  Both ends of the picked pair attain the minimum (p is
    symmetric in the pair), so the runner-up is the smallest p over the OTHER rows; inf where there is none."""
    return margin_of(y, *row_products(y, rows))


def brute_minimum(y, rows):
    """The smallest fl(y_u y_v) over all distinct non-adjacent pairs from the dense outer product; None where there is no pair."""
    n = y.shape[0]
    free = ~np.eye(n, dtype=bool)
    for u in range(n):
        free[u, list(rows[u])] = False
    prod = np.outer(y, y)
    free &= prod == prod
    return float(prod[free].min()) if free.any() else None


# ---- the loop ------------------------------------------------------------------------------------------------------------------
def loop_fast(edge_index, n, num_iterations, initial_power_iters, x0, replay=None):
    """loop with row_products_fast and a CSR adjacency rebuilt from the edge list at every iteration: no neighbour sets, no
    Python loop over the nodes.  Also returns the rule's own pick of every iteration: (edges, x, margins, picks)."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    a = spectral_ref.adjacency(ei, n)
    deg = np.diff(a.indptr).astype(np.int64)
    x = np.asarray(x0, dtype=np.float64).copy()
    for _ in range(initial_power_iters):
        x = power_step(a, deg, x)
        assert x is not None
    added, margins, picks = [], [], []
    for it in range(num_iterations):
        y = y_of(x, deg)
        p, partner = row_products_fast(y, a)
        got = pick_of(p, partner)
        if got is None:
            break
        margins.append(margin_of(y, p, partner))
        picks.append(got)
        u, v = (int(replay[0][it]), int(replay[1][it])) if replay is not None else got[:2]
        assert u != v and a[u, v] == 0
        added.append((u, v))
        ei = np.concatenate([ei, np.array([[u, v], [v, u]], dtype=np.int64)], axis=1)
        a = spectral_ref.adjacency(ei, n)
        deg = np.diff(a.indptr).astype(np.int64)
        x = power_step(a, deg, x)
        assert x is not None
    return np.array(added, dtype=np.int64).reshape(-1, 2).T, x, margins, picks


def loop(edge_index, n, num_iterations, initial_power_iters, x0, replay=None):
    """(added edges int64 [2, added], final x, the runner-up margin of every pick).  replay: int [2, k], the picks to take in
    place of the rule's own (the margins are then those of the rule on the replayed state)."""
    import scipy.sparse
    a, deg, rows = degrees_and_rows(edge_index, n)
    a = a.tolil()
    x = np.asarray(x0, dtype=np.float64).copy()
    stopped = False
    for _ in range(initial_power_iters):
        nxt = power_step(scipy.sparse.csr_matrix(a), deg, x)
        if nxt is None:
            stopped = True
            break
        x = nxt
    added, margins = [], []
    for it in range(num_iterations):
        if stopped:
            break
        y = y_of(x, deg)
        p, partner = row_products(y, rows)
        got = pick_of(p, partner)
        if got is None:
            break
        margins.append(margin_of(y, p, partner))
        u, v = (int(replay[0][it]), int(replay[1][it])) if replay is not None else got[:2]
        assert u != v and v not in rows[u]
        a[u, v] = a[v, u] = 1.0
        rows[u].add(v)
        rows[v].add(u)
        deg[u] += 1
        deg[v] += 1
        added.append((u, v))
        nxt = power_step(scipy.sparse.csr_matrix(a), deg, x)
        if nxt is None:
            stopped = True
        else:
            x = nxt
    return np.array(added, dtype=np.int64).reshape(-1, 2).T, x, margins


# ---- vectors -------------------------------------------------------------------------------------------------------------------
def vector_kinds(n, rng):
    """The vectors the pick is tried with: many ties, one sign only, all zero, both zeros."""
    x = rng.standard_normal(n)
    return {
        'normal': x,
        'small_integers': rng.integers(-2, 3, n).astype(np.float64),
        'positive': np.abs(x) + 0.5,
        'negative': -np.abs(x) - 0.5,
        'all_zero': np.zeros(n),
        'both_zeros': rng.choice(np.array([0.0, -0.0, 1.0, -1.0]), n),
        'two_values': np.where(rng.integers(0, 2, n) == 0, -0.75, 0.75),
    }


def packed_vector(deg, u, members, where):
    """x whose y = x / sqrt(deg + 1) makes row u the row that decides the pick, with its bitmap as full as it can be.  `members`
    are u and its neighbours.  'bottom': every y positive, u on rank 0 and its neighbours on the ranks above it, so u's first free
    rank is len(members); 'top': the mirror image, every y negative and u on the last rank; 'free0': as 'bottom' with one node
    outside below them all, so the first free rank is 0.  The node outside that u is paired with has the highest id, so that the
    tie between the two rows of the pair (equal products) goes to u."""
    n = deg.shape[0]
    inside = np.zeros(n, dtype=bool)
    inside[list(members)] = True
    y = np.empty(n)
    y[inside] = 0.1 + 0.1 * np.arange(inside.sum()) / n
    y[~inside] = 1.0 + np.arange((~inside).sum())[::-1] / n
    y[u] = 1e-3
    if where == 'free0':
        y[np.flatnonzero(~inside)[-1]] = 1e-4
    if where == 'top':
        y = -y
    return y * np.sqrt(deg + 1.0)


# ---- graphs --------------------------------------------------------------------------------------------------------------------
def random_graph(n, p, rng):
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < p]
    return (spectral_ref._und(pairs, n)[0] if pairs else np.zeros((2, 0), dtype=np.int64)), n


def irregular_graph(n, seed, components=1, isolated=0):
    """A graph of mixed degrees: per component a random tree (connected) plus random chords and a few hubs; then isolated nodes."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = n - isolated
    bounds = np.linspace(0, m, components + 1).astype(int)
    pairs = set()
    for c in range(components):
        lo, hi = int(bounds[c]), int(bounds[c + 1])
        for v in range(lo + 1, hi):
            pairs.add((int(rng.integers(lo, v)), v))
        for _ in range(2 * (hi - lo)):
            i, j = sorted(int(t) for t in rng.integers(lo, hi, 2))
            if i != j:
                pairs.add((i, j))
        for hub in range(lo, min(lo + 3, hi)):
            for j in rng.choice(np.arange(lo, hi), size=min(hi - lo, 40 + 30 * (hub - lo)), replace=False):
                if int(j) != hub:
                    pairs.add((min(hub, int(j)), max(hub, int(j))))
    return spectral_ref._und(sorted(pairs), n)[0], n


def two_cliques(m=20, chain=4):
    """Two K_m joined by a path of `chain` nodes (spectral_ref.barbell); (edge_index, n, left half, right half), the halves split
    by the middle of the path."""
    ei, n = spectral_ref.barbell(m, chain)
    half = m + chain // 2
    return ei, n, set(range(half)), set(range(half, n))


# the fixtures of the loop tests: (name, graph arguments, iterations, seed of x0); tests/test_fosr_cpu.py asserts their margins
LOOP_FIXTURES = [
    ('irregular200', dict(n=200, seed=1), 30, 11),
    ('two_components600', dict(n=600, seed=2, components=2), 40, 12),
    ('irregular2500', dict(n=2500, seed=3, isolated=1), 60, 13),
]
LOOP_INITIAL = 5
LOOP_LARGE_ITERS, LOOP_LARGE_SEED = 10, 14      # the loop on scale_ref.whole_small(): tests/test_fosr_cpu.py asserts its margins
_LOOPS = {}


def loop_fixture(name):
    """(edge_index, n, x0, iterations, the restatement's (edges, x, margins)), computed once."""
    if name not in _LOOPS:
        _, kw, iters, xseed = next(f for f in LOOP_FIXTURES if f[0] == name)
        ei, n = irregular_graph(**kw)
        x0 = np.random.Generator(np.random.PCG64(xseed)).standard_normal(n)
        _LOOPS[name] = (ei, n, x0, iters, loop(ei, n, iters, LOOP_INITIAL, x0))
    return _LOOPS[name]
