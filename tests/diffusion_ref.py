"""Dense numpy restatement of what DcrGraph.ppr and DcrGraph.diffusion compute (host only, graphs of a few thousand nodes at most):
S = alpha (I - (1 - alpha) D~^-1/2 (A + I) D~^-1/2)^-1 with D~ = D + I from ``numpy.linalg.solve``, the two per-column sparsifiers
with the device's tie-break (larger value first, among equal values the smaller node id first), and the column normalisation with
the sum taken in node-id order.  Nothing here imports the package under test."""
import os

import numpy as np

from resistance_ref import EPS, adjacency, barbell, complete, cycle, hub_with_tail, path, random_graph, star, triangle_star_isolated  # noqa: F401
from spectral_ref import PLAN_NAMES, plan_family, plan_nodes, row_plan  # noqa: F401

ALPHAS = (0.05, 0.15)


def operator(edge_index, n, alpha):
    """M = I - (1 - alpha) H, H = D~^-1/2 (A + I) D~^-1/2."""
    a = adjacency(edge_index, n) + np.eye(n)
    s = 1.0 / np.sqrt(a.sum(axis=1))
    return np.eye(n) - (1.0 - alpha) * (s[:, None] * a * s[None, :])


def ppr_matrix(edge_index, n, alpha):
    """S, dense: column j solves M x = alpha e_j."""
    return np.linalg.solve(operator(edge_index, n, alpha), alpha * np.eye(n))


def ppr_columns(edge_index, n, alpha, sources):
    """[len(sources), n]: row i is column sources[i] of S, without the other columns."""
    rhs = np.zeros((n, len(sources)))
    rhs[np.asarray(sources, dtype=np.int64), np.arange(len(sources))] = alpha
    return np.linalg.solve(operator(edge_index, n, alpha), rhs).T.copy()


# ---- without a dense matrix: the host certificate of tests/test_diffusion_gpu.py at 33,000 nodes ------------------------------------
def sparse_operator(edge_index, n, alpha):
    """(M as scipy CSC in float64, A + I as CSR, s~ = 1 / sqrt(deg + 1))."""
    import scipy.sparse
    from spectral_ref import adjacency as sparse_adjacency
    at = (sparse_adjacency(edge_index, n) + scipy.sparse.identity(n)).tocsr()
    s = 1.0 / np.sqrt(np.asarray(at.sum(axis=1)).ravel())
    d = scipy.sparse.diags(s)
    return (scipy.sparse.identity(n) - (1.0 - alpha) * (d @ at @ d)).tocsc(), at, s


def residual_long(at, x, source, alpha):
    """|alpha e_source - M x|_2 with M x = x - (1 - alpha) s~ (.) ((A + I) (s~ (.) x)) evaluated in np.longdouble from the degrees:
    no rounded matrix entry takes part."""
    from spectral_ref import csr_matvec_long
    L = np.longdouble
    s = L(1) / np.sqrt(np.asarray(at.sum(axis=1)).ravel().astype(L))
    x = np.asarray(x, dtype=L)
    e = -(x - L(1.0 - alpha) * (s * csr_matvec_long(at, s * x)))
    e[source] += L(alpha)
    return float(np.sqrt(np.sum(e * e)))


def matvec_error(M, x, d_max):
    """(d_max + 4) 2^-52 | |M| |x| |_2: the forward error of a float64 mat-vec whose longest row adds d_max + 1 products, in the
    2-norm.  What the residual a device reports may differ by from the residual of the same column computed exactly."""
    return (d_max + 4) * EPS * float(np.linalg.norm(abs(M) @ np.abs(x)))


def residual_long_rounding(M, at, x):
    """What residual_long's own arithmetic can be off by: row i of its mat-vec adds deg_i + 1 products and takes four more
    roundings, each within the spacing of np.longdouble: | (deg_i + 4) eps_long (|M| |x|)_i |_2.  2,048 times below matvec_error
    where np.longdouble has 64 bits of mantissa."""
    per_row = (at.getnnz(axis=1) - 1 + 4) * float(np.finfo(np.longdouble).eps)
    return float(np.linalg.norm(per_row * (abs(M) @ np.abs(x))))


def lu_columns(M, sources, alpha):
    """[len(sources), n] from scipy.sparse.linalg.splu."""
    import scipy.sparse.linalg
    rhs = np.zeros((M.shape[0], len(sources)))
    rhs[np.asarray(sources, dtype=np.int64), np.arange(len(sources))] = alpha
    return scipy.sparse.linalg.splu(M).solve(rhs).T.copy()


def allow(n):
    """The rounding allowance of the acceptance rule (resistance_ref.allow with entries <= 1): 64 n 2^-52."""
    return 64.0 * n * EPS


def top_k(column, k):
    """Sorted node ids of the k entries that come first by (larger value, smaller id); all of them where k >= n."""
    column = np.asarray(column)
    order = np.lexsort((np.arange(column.size), -column))
    return np.sort(order[:min(int(k), column.size)])


def threshold(column, eps):
    """Sorted node ids of the entries >= eps."""
    return np.flatnonzero(np.asarray(column) >= eps)


def ordered_sum(values):
    """The values added one after the other (numpy.sum adds in pairs)."""
    values = np.asarray(values, dtype=np.float64)
    return float(np.cumsum(values)[-1]) if values.size else 0.0


def normalise(values):
    """values / their sum in the order given; by 1 where the sum is not positive (as the reference's helpers divide)."""
    total = ordered_sum(values)
    return np.asarray(values, dtype=np.float64) / (total if total > 0.0 else 1.0)


def sparsify(S, k=None, eps=None, columns=None):
    """(ptr, row, weight, value) over the columns of S in the layout of DcrGraph.diffusion: grouped by column, by node id within."""
    assert (k is None) != (eps is None)
    cols = range(S.shape[1]) if columns is None else columns
    ptr, rows, weights, values = [0], [], [], []
    for j in cols:
        keep = top_k(S[:, j], k) if eps is None else threshold(S[:, j], eps)
        rows.append(keep)
        values.append(S[keep, j])
        weights.append(normalise(S[keep, j]))
        ptr.append(ptr[-1] + keep.size)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.empty(0, dtype=dt)   # noqa: E731
    return np.array(ptr, dtype=np.int64), cat(rows, np.int32), cat(weights, np.float64), cat(values, np.float64)


def recorded(golden_dir, fixture, name):
    """(ptr int64, rows int32, weights) of one helper's result in tests/golden/diffusion_reference.json's array file; name is
    case['top_k'] or case['clipped']."""
    with np.load(os.path.join(golden_dir, fixture['arrays']), allow_pickle=False) as z:
        return z[name + '_ptr'].astype(np.int64), z[name + '_rows'].astype(np.int32), z[name + '_weights']


def graphs():
    """name -> (edge_index, n): the graphs of the value and selection tests; the tie-rich ones are there on purpose."""
    return {'path8': path(8), 'cycle7': cycle(7), 'star6': star(6), 'barbell20_4': barbell(20, 4), 'random300': random_graph(300, 5),
            'hub2100': hub_with_tail(2100)}
