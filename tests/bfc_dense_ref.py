"""Host-side (numpy) companion of csrc/dcr_bfc_dense.hip for tests/test_bfc_dense_{cpu,gpu}.py — TEST INFRASTRUCTURE.

Three things live here:

  * ``curvature`` / ``post_delta``: the two formulas of csrc/dcr_bfc_dense.hip restated from that file's own comments —
    every per-``k`` term a float32 product of small integers (exact), the closing expression in float64 in the file's
    operation order, one rounding to float32 after the base expression and one after the 4-cycle term.  ``k_limit`` /
    ``z_limit`` cut the per-pair loop short: they model a kernel whose lanes lose the tail of the 64-wide stride loop,
    and the CPU test uses them to prove that the graphs below would catch such a kernel.
  * closed forms on K_n, S_n and C_n, each derived in its docstring;
  * seeded graph families built so that the deciding terms of many pairs sit at the LAST node ids, i.e. in the last
    (partial) trip of ``for (k = lane; k < N; k += 64)``.

Out of scope: non-integer weights in ``A``.  ``A2 = A·A`` comes from the GEMM library on the device and its bits are
pinned by nothing once the entries stop being small integers; every graph here has entries in {0, 1, 2}.
"""
import numpy as np

# trip counts of the 64-wide stride loop: 1, 1, 2 for lane 0 only, 2, 2, 3 for lane 0 only, 5 (lane 0 only for the last)
SIZES = [63, 64, 65, 127, 128, 129, 257]


# ---- the two formulas ---------------------------------------------------------------------------------------------------
def _closing(d_max, d_min, a2_xy, a_xy, sharp, lam):
    """dense_closing of csrc/dcr_bfc_dense.hip: float64, its operation order, two float32 stores."""
    d_max, d_min, a2_xy, a_xy = np.float64(d_max), np.float64(d_min), np.float64(a2_xy), np.float64(a_xy)
    r = np.float64(2.0) / d_max
    r = r + np.float64(2.0) / d_min
    r = r - np.float64(2.0)
    m = np.float64(2.0) / d_max + np.float64(1.0) / d_min
    m = m * a2_xy
    m = m * a_xy
    c = np.float32(r + m)
    if lam > 0:
        c = np.float32(np.float64(c) + np.float64(sharp) / (d_max * np.float64(lam)))
    return c


def _square(A):
    A = np.asarray(A, dtype=np.float32)
    A2 = (A.astype(np.float64) @ A.astype(np.float64)).astype(np.float32)     # small integers: exact in either type
    return A, A2


def _count_and_max(t1, t2):
    sharp = int(np.count_nonzero(t1 > 0)) + int(np.count_nonzero(t2 > 0))
    lam = np.float32(0.0)
    if t1.size:
        lam = max(lam, t1.max(), t2.max())
    return sharp, lam


def curvature(A, k_limit=None):
    """C[i, j] for every non-zero pair of ``A`` as k_bfc_dense computes it, 0 elsewhere.  ``k_limit``: the per-pair loop
    runs over ``k < k_limit`` only."""
    A, A2 = _square(A)
    N = A.shape[0]
    K = N if k_limit is None else max(0, min(int(k_limit), N))
    d_in, d_out = A.sum(axis=0, dtype=np.float64).astype(np.float32), A.sum(axis=1, dtype=np.float64).astype(np.float32)
    C = np.zeros((N, N), dtype=np.float32)
    for i, j in zip(*np.nonzero(A)):
        if d_in[i] > d_out[j]:
            d_max, d_min = d_in[i], d_out[j]
        else:
            d_max, d_min = d_out[j], d_in[i]
        if d_max * d_min == 0:
            continue
        a_ij = A[i, j]
        t1 = A[:K, j] * (A2[i, :K] - A[i, :K]) * a_ij
        t2 = A[i, :K] * (A2[:K, j] - A[:K, j]) * a_ij
        sharp, lam = _count_and_max(t1, t2)
        C[i, j] = _closing(d_max, d_min, A2[i, j], a_ij, sharp, lam)
    return C


def post_delta(A, x, y, i_nb, j_nb, z_limit=None):
    """D[I, J] as k_bfc_dense_post_delta computes it: the curvature of (x, y) once the edge (i_nb[I], j_nb[J]) is added;
    -1000 where the two nodes coincide or the edge exists.  ``z_limit``: the per-candidate loop runs over ``z < z_limit``."""
    A, A2 = _square(A)
    N = A.shape[0]
    Z = N if z_limit is None else max(0, min(int(z_limit), N))
    z = np.arange(Z)
    d_in_x0, d_out_y0 = np.float64(A[:, x].sum(dtype=np.float64)), np.float64(A[y].sum(dtype=np.float64))
    D = np.zeros((len(i_nb), len(j_nb)), dtype=np.float32)
    one = np.float32(1.0)
    for I, i in enumerate(i_nb):
        for J, j in enumerate(j_nb):
            if i == j or A[i, j] != 0:
                D[I, J] = -1000.0
                continue
            d_in_x, d_out_y = d_in_x0, d_out_y0
            if j == x:
                d_in_x = d_in_x + 1.0
            elif i == y:
                d_out_y = d_out_y + 1.0
            if d_in_x * d_out_y == 0:
                continue
            d_max, d_min = (d_in_x, d_out_y) if d_in_x > d_out_y else (d_out_y, d_in_x)
            a_xy, a_jy, a_xi = A[x, y], A[j, y], A[x, i]
            a2_xy = np.float64(A2[x, y])
            if x == i and a_jy != 0:
                a2_xy = a2_xy + np.float64(a_jy)
            elif y == j and a_xi != 0:
                a2_xy = a2_xy + np.float64(a_xi)
            a_zy, a_xz = A[:Z, y].copy(), A[x, :Z].copy()
            a2_zy, a2_xz = A2[:Z, y].copy(), A2[x, :Z].copy()
            if y == j:
                a_zy[z == i] += one
            if x == i:
                a_xz[z == j] += one
            if a_jy != 0:
                a2_zy[z == i] += a_jy
            if x == i:
                a2_xz += A[j, :Z]                      # adding the zeros changes nothing
            if y == j:
                a2_zy += A[:Z, i]
            if a_xi != 0:
                a2_xz[z == j] += a_xi
            t1 = a_zy * (a2_xz - a_xz) * a_xy
            t2 = a_xz * (a2_zy - a_zy) * a_xy
            sharp, lam = _count_and_max(t1, t2)
            D[I, J] = _closing(d_max, d_min, a2_xy, a_xy, sharp, lam)
    return D


def tail_limit(N):
    """The loop limit of a kernel that loses its last trip: the partial trip where N is no multiple of 64, the whole
    last trip where it is."""
    return N - 64 if N % 64 == 0 else 64 * ((N - 1) // 64)


# ---- closed forms -------------------------------------------------------------------------------------------------------
def complete_value(n):
    """Every edge of K_n, n > 3.  d = n - 1 at both ends, A2[i, j] = n - 2 (the common neighbours).  First term at k:
    A[k, j] * (A2[i, k] - A[i, k]): for the n - 2 other nodes it is (n - 2) - 1 = n - 3 > 0; at k = i it is
    A2[i, i] - A[i, i] = n - 1; at k = j it is 0 (A[j, j] = 0).  The second term mirrors it.  So sharp = 2(n - 1) and
    lambda = n - 1, and the value is float32(float32(4/d - 2 + 3(n - 2)/d) + (2n - 2) / (d (n - 1)))."""
    assert n > 3
    d = float(n - 1)
    return np.float32(np.float64(np.float32(4 / d - 2 + 3 * (n - 2) / d)) + (2 * n - 2) / (d * (n - 1)))


def star_value(n):
    """Every entry (leaf, hub) and (hub, leaf) of the star S_n on n >= 3 nodes (hub = node n - 1, h = n - 1 leaves).
    d_max = h, d_min = 1, A2[leaf, hub] = 0 (no triangle).  For (leaf l, hub c): the first term at k is
    A[k, c] * (A2[l, k] - A[l, k]), non-zero at the h leaves, where A2[l, k] = 1 (the path through the hub, k = l
    included) and A[l, k] = 0: h terms equal to 1.  The second term A[l, k] * (A2[k, c] - A[k, c]) is non-zero at k = c
    only: A2[c, c] = h.  So sharp = h + 1, lambda = h; (hub, leaf) mirrors it.  The base expression is 2/h + 2/1 - 2
    evaluated left to right in float64 (the +2 - 2 costs 2/h its last bits, as in the kernel), then rounded."""
    assert n >= 3
    h = float(n - 1)
    return np.float32(np.float64(np.float32((2 / h + 2 / 1.0) - 2)) + (h + 1) / (h * h))


def cycle_value(n):
    """Every edge of C_n, n >= 5.  d = 2 at both ends, A2[i, j] = 0.  For (i, j = i + 1): the first term
    A[k, j] * (A2[i, k] - A[i, k]) is non-zero at j's neighbours: k = i gives A2[i, i] = 2, k = i + 2 gives
    A2[i, i + 2] = 1 (one path; n >= 5 keeps it at one).  The second term mirrors it at k = j and k = i - 1.  So
    sharp = 4, lambda = 2: float32(2/2 + 2/2 - 2) + 4 / (2 * 2) = 1.0 at every n."""
    assert n >= 5
    return np.float32(np.float64(np.float32(2 / 2.0 + 2 / 2.0 - 2)) + 4 / (2.0 * 2.0))


def complete(n):
    return np.ones((n, n), dtype=np.float32) - np.eye(n, dtype=np.float32)


def star(n):
    A = np.zeros((n, n), dtype=np.float32)
    A[n - 1, :n - 1] = A[:n - 1, n - 1] = 1.0
    return A


def cycle(n):
    A = np.zeros((n, n), dtype=np.float32)
    v = np.arange(n)
    A[v, (v + 1) % n] = A[(v + 1) % n, v] = 1.0
    return A


# ---- families -----------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def hub_last(N, seed):
    """Sparse random undirected graph (average degree about 6) in which node N - 1 is joined to about a third of the nodes
    and node N - 2 to a quarter: for many pairs the largest term of the loop arises at k = N - 1 or k = N - 2."""
    rng = _rng(seed)
    m = np.triu(rng.random((N, N)) < 6.0 / (N - 1), 1)
    m[rng.choice(N - 1, size=N // 3, replace=False), N - 1] = True
    m[rng.choice(N - 2, size=N // 4, replace=False), N - 2] = True
    m = m | m.T
    return m.astype(np.float32)


def directed_tail(N, seed):
    """The directed counterpart (any nnz), plus three special entries.  Returns (A, special): ``special['source']`` is a
    node with out-edges and no in-edge (the d_max * d_min == 0 branch), ``special['two']`` a pair whose entry is 2 (what
    the dense loop's accumulate produces from a duplicated directed edge), ``special['diag']`` a node with a diagonal
    entry (a direct call computes it like any pair)."""
    rng = _rng(seed)
    m = rng.random((N, N)) < 3.0 / (N - 1)
    np.fill_diagonal(m, False)
    for hub, share in ((N - 1, 3), (N - 2, 4)):
        m[hub, rng.choice(hub, size=N // share, replace=False)] = True
        m[rng.choice(hub, size=N // share, replace=False), hub] = True
    s, q = N - 3, N - 4
    m[:, s] = False
    m[s, rng.choice(N - 4, size=3, replace=False)] = True
    m[s, N - 1] = True
    A = m.astype(np.float32)
    u = int(np.nonzero(A[:N - 4, N - 1])[0][0])          # an edge into the last-id hub, doubled
    A[u, N - 1] = 2.0
    A[q, q] = 1.0
    return A, {'source': s, 'two': (u, N - 1), 'diag': q}


def torus(a, b):
    """a x b torus, node r * b + c: every edge is equivalent to every other."""
    A = np.zeros((a * b, a * b), dtype=np.float32)
    for r in range(a):
        for c in range(b):
            for v in (((r + 1) % a) * b + c, r * b + (c + 1) % b):
                A[r * b + c, v] = A[v, r * b + c] = 1.0
    return A


def copies(A, m):
    """Disjoint union of m copies of the graph."""
    return np.kron(np.eye(m, dtype=np.float32), np.asarray(A, dtype=np.float32))


def family_graphs(sizes=SIZES):
    """[(name, A, special or None, directed)] — every family graph of the two test modules, seeded by its size."""
    out = []
    for N in sizes:
        out.append((f'hub_last-{N}', hub_last(N, N), None, False))
        A, sp = directed_tail(N, 1000 + N)
        out.append((f'directed_tail-{N}', A, sp, True))
    return out


def edge_index(A):
    """int64 [2, M] in row-major order of the non-zero entries; an entry equal to 2 is listed twice."""
    src, dst = np.nonzero(A)
    rep = A[src, dst].astype(np.int64)
    return np.stack([np.repeat(src, rep), np.repeat(dst, rep)]).astype(np.int64)


# ---- post-delta queries -------------------------------------------------------------------------------------------------
def neighbour_lists(A, x, y, directed):
    """The lists the dense loop builds: neighbours of x plus x and neighbours of y plus y; successors of x and
    predecessors of y for a directed graph."""
    i_nb = [int(t) for t in np.nonzero(A[x])[0]] + [int(x)]
    j_nb = [int(t) for t in np.nonzero(A[:, y] if directed else A[y])[0]] + [int(y)]
    return i_nb, j_nb


def base_queries(A, C, directed):
    """Three (x, y): the pair with the most negative curvature (first occurrence), and an edge at the last-id hub taken
    from both sides."""
    N = A.shape[0]
    nz = np.nonzero(A)
    t = int(np.argmin(C[nz]))
    hub = N - 1
    out_nb = int(np.nonzero(A[hub, :hub])[0][-1])
    in_nb = int(np.nonzero(A[:hub, hub])[0][0])
    return [(int(nz[0][t]), int(nz[1][t])), (hub, out_nb), (in_nb, hub)]


def directed_queries(A):
    """Two more for a directed graph: an edge (x, y) one of whose candidates has j == x (a successor i of x without the
    edge i -> x) and one with a candidate i == y (a predecessor j of y, j != x, without the edge y -> j)."""
    hit_jx = hit_iy = None
    for x, y in zip(*np.nonzero(A)):
        if x == y:
            continue
        succ = [i for i in np.nonzero(A[x])[0] if i != x]
        pred = [j for j in np.nonzero(A[:, y])[0] if j != y and j != x]
        if hit_jx is None and any(A[i, x] == 0 for i in succ):
            hit_jx = (int(x), int(y))
        elif hit_iy is None and (int(x), int(y)) != hit_jx and any(A[y, j] == 0 for j in pred):
            hit_iy = (int(x), int(y))
        if hit_jx and hit_iy:
            break
    assert hit_jx and hit_iy
    return [hit_jx, hit_iy]
