"""Host oracles of the heat-kernel diffusion (DcrGraph.heat, csrc/dcr_diffusion.hip): S = exp(-t (I - H)), H = D~^-1/2 (A + I) D~^-1/2,
D~ = D + I.  Two routes that share nothing but the graph: the Taylor recurrence of include/dcr.h in np.longdouble, which needs no
n x n array, and the spectral form from ``numpy.linalg.eigh``.  With theta_k = e^-t t^k / k! and rho_K = sum_{k > K} theta_k: the
rule that fixes the number of terms, restated, and the rounding allowance of the device's float64 recurrence, derived.  Nothing
here imports the package under test."""
import numpy as np

from diffusion_ref import adjacency, graphs  # noqa: F401
from resistance_ref import EPS
from spectral_ref import adjacency as sparse_adjacency, csr_matvec_long

L = np.longdouble
HEAT_TS = (0.5, 5.0, 20.0)
TOL = 1e-10
ORACLE_EXTRA = 40   # terms the longdouble oracle adds to the device's K: its own tail rho_{K + 40} is below 1e-30 for t <= 20
_EIGH = {}


def operator_long(edge_index, n):
    """(A + I as scipy CSR, s~ = 1 / sqrt(deg + 1) and r = sqrt(deg + 1) in np.longdouble, the degrees)."""
    import scipy.sparse
    at = (sparse_adjacency(edge_index, n) + scipy.sparse.identity(n)).tocsr()
    deg = at.getnnz(axis=1) - 1
    r = np.sqrt((deg + 1).astype(L))
    return at, L(1) / r, r, deg


def taylor_long(edge_index, n, t, sources, K):
    """[len(sources), n] in np.longdouble: x = sum_{k = 0 .. K} theta_k H^k e_j by v_0 = e^-t e_j,
    v_{k+1} = t / (k + 1) s~ (.) ((A + I)(s~ (.) v_k)), x += v_{k+1}; a row of the mat-vec is added from left to right."""
    at, s, _, _ = operator_long(edge_index, n)
    out = np.zeros((len(sources), n), dtype=L)
    for i, j in enumerate(sources):
        v = np.zeros(n, dtype=L)
        v[j] = np.exp(-L(t))
        x = v.copy()
        for k in range(int(K)):
            v = (L(t) / L(k + 1)) * (s * csr_matvec_long(at, s * v))
            x += v
        out[i] = x
    return out


def dense(edge_index, n, t, key=None):
    """S = V exp(-t (1 - lambda)) V^T from numpy.linalg.eigh of H, float64 [n, n] (symmetric: row j is column j).  `key`: a name
    under which the decomposition is kept for other t."""
    if key is None or key not in _EIGH:
        a = adjacency(edge_index, n) + np.eye(n)
        s = 1.0 / np.sqrt(a.sum(axis=1))
        lam, V = np.linalg.eigh(s[:, None] * a * s[None, :])
        if key is not None:
            _EIGH[key] = (lam, V)
    else:
        lam, V = _EIGH[key]
    return (V * np.exp(-t * (1.0 - lam))) @ V.T


def dense_allow(n):
    """What `dense` may be off by, entries being <= 1: 64 n 2^-52, the allowance of the dense PageRank reference
    (diffusion_ref.allow); tests/test_heat_cpu.py holds the two oracles to it against each other."""
    return 64.0 * n * EPS


def thetas(t):
    """theta_0, theta_1, ... in np.longdouble up to 300 terms past 2 t, where they halve at least from one to the next: what is
    left out is below 2^-300."""
    out = [np.exp(-L(t))]
    for k in range(1, int(2 * t) + 300):
        out.append(out[-1] * L(t) / L(k))
    return np.array(out, dtype=L)


def tail(t, K):
    """rho_K = sum_{k > K} theta_k in np.longdouble, the terms added from the small end; never 1 - the partial sum."""
    th = thetas(t)
    return L(0) if K + 1 >= th.size else np.cumsum(th[:K:-1])[-1]


def terms(t, tol, max_terms=4096):
    """K of the device, restated in its float64: theta_k by theta_k = theta_{k-1} t / k until it underflows to zero; from the last
    of them downwards the tail is added term by term, and K is the smallest count whose tail is <= tol / 2; max_terms where that
    is lower."""
    theta, th = [], float(np.exp(-np.float64(t)))
    while th > 0.0 and len(theta) < 65536:
        theta.append(th)
        th *= t / float(len(theta))
    K, rho = len(theta) - 1, 0.0
    while K > 0 and rho + theta[K] <= 0.5 * tol:
        rho += theta[K]
        K -= 1
    return min(K, int(max_terms))


def allow(K, d_max):
    """(K + 1)(d_max + 12) 2^-52: what the device's float64 partial sum of K terms after the first may differ by from the same sum
    in exact arithmetic, entry by entry.

    Every quantity of the recurrence is non-negative, so nothing cancels and each rounding is a relative error of at most
    u = 2^-53 of a quantity that only grows into the result: the errors add, componentwise and relative, so the bound is
    |x_i - X_i| <= allow X_i entry by entry (tests/heat_steps_ref.py::compare applies it so; as an absolute number it is only the
    weaker statement that follows from X_i <= 1).  It assumes that nothing underflows.

    One term, at a row of degree deg, counted from the z it reads to the z it writes.  The row's sum (A + I) z is a tree of
    additions over deg + 1 leaves, whatever its shape: the lanes of the row's scope add their slots one after the other, a
    butterfly adds the lanes of a wave, a long row's four wave sums are added in wave order, and the row's own z comes last.  An
    addition one of whose operands is 0.0 (a lane with no slot, a leaf outside the support) is exact, and a tree has at most
    (leaves - 1) additions both of whose operands hold a leaf, so an entry passes through at most deg of them that round; deg + 1
    is counted.  s~ carries two roundings of its own (the square root and the division) and is used twice, in v and in the z
    handed on, four in all; c = t / (k + 1) is one rounding; the scalings by s~ and by c in v are one each and the scaling by s~
    in z_out one more, three.  That is deg + 1 + 4 + 1 + 3 = deg + 9 <= d_max + 9 roundings from z to z, of which v has taken
    deg + 6 and z_out adds three; the first z = s~ e^-t carries one for e^-t, two for s~ and one for the product.  Term k
    therefore carries at most 4 + (k - 1)(d_max + 9) + d_max + 6 = k (d_max + 9) + 1 relative roundings, and x after K terms, with
    the K additions into x, at most K (d_max + 9) + 1 + K <= (K + 1)(d_max + 10) of them, times u (1 + O(K d_max u)).  Stated with
    2^-52 and d_max + 12 it has more than a factor of two in hand, which covers the second-order terms, a libm whose exp is a
    little more than half an ulp off, a device square root that is within one ulp and not half of one (two more roundings a
    term), and the np.longdouble arithmetic of the oracle it is compared with (2^-11 of it)."""
    return (K + 1) * (d_max + 12) * EPS
