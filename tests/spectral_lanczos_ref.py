"""Host replica of the Lanczos driver of csrc/dcr_spectral.hip (dcr_spectral_gap), step by step, for the tests to hold the kernels
to (numpy and scipy only; nothing here imports the package's device code).

At ``tol = 0`` the driver's control flow depends on the graph and the seed alone: nothing converges, no Lanczos-estimate restart
fires unless the estimate is exactly zero, and a restart is forced at ``total = max_steps - 1``.  What it returns is then defined
in exact arithmetic: the deflated, normalised top Ritz vector y of a Krylov space of P B P from the Philox start vector, the
Rayleigh quotient ``lambda1 = 2 - y . B y`` and the true residual ``|P(B y) - (y . B y) y|`` of the closing step.  None of the three
depends on how the orthogonalisation is organised, so `schedule` walks the same schedule with full reorthogonalisation in
np.longdouble and states them; ``dtype=np.float64`` runs the same code in the device's precision, and the distance between the two
runs is what the allowance of the GPU test rests on (`allow`).

B = I + D^-1/2 A D^-1/2 (spectrum in [0, 2]), P the projector off the null space of L = 2 - B: k_C = D^1/2 1_C / sqrt(vol C) per
component with an edge.  Every vector is zero on the isolated nodes, whose scale D^-1/2 is 0."""
import os
import re

import numpy as np

import cheeger_ref
import spectral_ref
from conftest import PKG

L = np.longdouble
_M64, _M32 = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF
_U32 = np.uint64(32)


def _source(name):
    with open(os.path.join(PKG, 'csrc', name)) as f:
        return f.read()


def _int_constant(text, name):
    m = re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, text)
    assert m, name + ' not found'
    return int(m.group(1))


_HIP = _source('dcr_spectral.hip')
SP_CHECK_EVERY = _int_constant(_source('dcr_analysis.h'), 'SP_CHECK_EVERY')     # solver steps between host synchronisations
SP_WAVE_ELEMS = _int_constant(_HIP, 'SP_WAVE_ELEMS')                           # elements of w a wave of k_spec_gs_coef holds
SP_CHUNK = _int_constant(_HIP, 'SP_CHUNK')                                     # nodes per deflation chunk
_m = re.search(r'constexpr\s+double\s+SP_BREAKDOWN\s*=\s*0x1p-(\d+)\s*;', _HIP)
assert _m, 'SP_BREAKDOWN not found'
SP_BREAKDOWN = 2.0 ** -int(_m.group(1))
assert re.search(r'early\s*=\s*j \+ 1 < SP_CHECK_EVERY && \(\(j \+ 1\) & j\) == 0;\s*if \(!\(early \|\| \(j \+ 1\) % SP_CHECK_EVERY == 0 \|\| '
                 r'j \+ 1 == m \|\| forced\)\) continue;', _HIP), 'the steps at which the driver looks at its coefficients'
BASIS_BYTES = 4 << 30      # spectral_solve: by_memory = (4 << 30) / (8 n) columns
assert re.search(r'by_memory\s*=\s*\(\(int64_t\)4\s*<<\s*30\)\s*/\s*\(8\s*\*\s*n\)', _HIP), 'the basis capacity of spectral_solve'


# ---- the start vector ---------------------------------------------------------------------------------------------------------------
def start_values(nodes, seed, restart=0):
    """float64 array: what k_spec_start draws for the node ids `nodes` (any uint64 values): Philox-4x32-10 with counter
    {node lo, node hi, restart lo, restart hi} and key {seed lo, seed hi}; bits = (r0 | r1 << 32) >> 11;
    ((float64)bits + 0.5) * 2^-52 - 1.0 evaluated in float64 in that order (bits + 0.5 rounds to even once bits >= 2^52)."""
    v = np.asarray(nodes, dtype=np.uint64)
    seed, restart = int(seed) & _M64, int(restart) & _M64
    r = cheeger_ref.philox4x32_10(v & np.uint64(_M32), v >> _U32, np.full(v.shape, restart & _M32, dtype=np.uint64),
                                  np.full(v.shape, restart >> 32, dtype=np.uint64), seed & _M32, seed >> 32)
    bits = (r[0] | (r[1] << _U32)) >> np.uint64(11)
    return (bits.astype(np.float64) + np.float64(0.5)) * np.float64(2.0 ** -52) - np.float64(1.0)


def start_vector(deg, seed, restart=0):
    """float64 [n]: the vector of k_spec_start; 0 on nodes of degree 0."""
    deg = np.asarray(deg)
    return np.where(deg > 0, start_values(np.arange(deg.shape[0], dtype=np.uint64), seed, restart), 0.0)


# ---- the operator -------------------------------------------------------------------------------------------------------------------
class Replica:
    """B and P of one graph in `dtype`.  K holds the k_C of spectral_ref.null_vectors that belong to a component with an edge,
    formed in `dtype` as the device forms them in float64: sqrt(deg) / sqrt(vol C); `roots` their components' smallest node ids,
    ascending, which is the order the device numbers the components in."""

    def __init__(self, edge_index, n, dtype=L):
        self.n, self.dtype = int(n), dtype
        self.a = spectral_ref.adjacency(edge_index, n)
        self.deg = np.diff(self.a.indptr).astype(np.int64)
        self.components, self.labels = spectral_ref.components(edge_index, n)
        d = self.deg.astype(dtype)
        self.s = np.zeros(n, dtype=dtype)
        self.s[self.deg > 0] = dtype(1) / np.sqrt(d[self.deg > 0])
        self.roots = np.array([r for r in np.unique(self.labels) if self.deg[r] > 0], dtype=np.int64)
        self.K = np.zeros((len(self.roots), n), dtype=dtype)
        for i, r in enumerate(self.roots):
            inside = self.labels == r
            self.K[i, inside] = np.sqrt(d[inside]) / np.sqrt(dtype(int(self.deg[inside].sum())))

    def project(self, w):
        """w - sum_C (k_C . w) k_C"""
        w = np.asarray(w, dtype=self.dtype)
        return w - self.K.T @ (self.K @ w)

    def apply_B(self, v):
        """v + s (.) A (s (.) v); a row of the mat-vec is added from left to right (in float64: in scipy's order)."""
        v = np.asarray(v, dtype=self.dtype)
        z = self.s * v
        az = spectral_ref.csr_matvec_long(self.a, z) if self.dtype is L else self.a @ z
        return v + self.s * az

    def chunks(self):
        """[(first position, end position, first chunk of its component, chunks of its component)] as spectral_solve lays the
        deflation chunks out, and whether it takes the one-component path."""
        if len(self.roots) == 1:
            nc = -(-self.n // SP_CHUNK)
            return [(c * SP_CHUNK, min(self.n, (c + 1) * SP_CHUNK), 0, nc) for c in range(nc)], True
        out, b = [], 0
        for r in self.roots:
            size = int((self.labels == r).sum())
            nc, c0 = -(-size // SP_CHUNK), len(out)
            out += [(b + i * SP_CHUNK, min(b + size, b + (i + 1) * SP_CHUNK), c0, nc) for i in range(nc)]
            b += size
        return out, False


def replica(graph, dtype=L):
    if isinstance(graph, Replica):
        assert graph.dtype is dtype, 'a Replica is built for one dtype'
        return graph
    return Replica(graph[0], graph[1], dtype)


def project(graph, w, dtype=L):
    return replica(graph, dtype).project(w)


def apply_B(graph, v, dtype=L):
    return replica(graph, dtype).apply_B(v)


def basis_columns(n, components, max_basis=None):
    """m of spectral_solve: min(basis, n - components)."""
    by_memory = BASIS_BYTES // (8 * n)
    m = min(int(max_basis), max(by_memory, 16)) if max_basis else max(min(256, by_memory), 16)
    return max(1, min(max(m, 2), n - components))


def top_ritz(alpha, beta, k):
    """(theta, y, gap) of T_k: the largest eigenvalue, its eigenvector, and its distance to the second largest (inf at k = 1),
    from numpy.linalg.eigh of the float64 tridiagonal."""
    a = np.array([float(x) for x in alpha[:k]])
    b = np.array([float(x) for x in beta[:k - 1]])
    lam, Z = np.linalg.eigh(np.diag(a) + np.diag(b, 1) + np.diag(b, -1))
    return lam[-1], Z[:, -1], (lam[-1] - lam[-2] if k > 1 else np.inf)


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
def schedule(graph, seed, max_steps, max_basis=None, dtype=L, trace=None):
    """(lambda1, residual, vector, steps, restarts) of dcr_spectral_gap at tol = 0 on `graph` = (edge_index, n) or a Replica.

    The driver's own schedule: cycles of Lanczos steps j = 0, 1, ...; the host looks at alpha and beta after steps 1, 2 and 4 of a
    cycle (the powers of two below SP_CHECK_EVERY), every SP_CHECK_EVERY steps, at j + 1 == m and when forced
    (total >= max_steps - 1); m = min(basis, n - components).  At j == 0 it
    takes the pair of column 0 (alpha_0, beta_0) and stops if this was the last cycle or the steps are used up.  It restarts from
    the top Ritz vector of T_k on breakdown (a beta < SP_BREAKDOWN: k stops there), at k == m, when forced, and when the Lanczos
    estimate beta_{k-1} |y_k| is exactly 0.  Each step: w = B v_j, alpha_j = v_j . w, w = P w, classical Gram-Schmidt against all
    columns twice, w = P w, beta_j = |w|, v_{j+1} = w / beta_j.

    `trace`, a dict, receives 'gap' (of the last T_k a restart used), 'betas' (every beta the breakdown test looked at, but for
    beta_{m-1} where m = n - components, which is zero in exact arithmetic) and 'ritz' (the k of every restart)."""
    R = replica(graph, dtype)
    n = R.n
    m = basis_columns(n, R.components, max_basis)
    capped = m == n - R.components
    zero = np.zeros(n, dtype=dtype)

    def first_column(w):
        w = R.project(w)
        b = np.sqrt(w @ w)
        return w / b if b >= SP_BREAKDOWN else zero

    V = [first_column(start_vector(R.deg, seed).astype(dtype))]
    total = restarts = 0
    last_cycle = False
    theta = residual = None
    info = dict(gap=np.inf, betas=[], ritz=[])
    while True:
        alpha, beta, j = [], [], 0
        while True:
            w = R.apply_B(V[j])
            alpha.append(V[j] @ w)
            w = R.project(w)
            basis = np.array(V[:j + 1])
            for _ in range(2):
                w = w - basis.T @ (basis @ w)
            w = R.project(w)
            beta.append(np.sqrt(w @ w))
            if j + 1 < m:
                V.append(w / beta[j] if beta[j] >= SP_BREAKDOWN else zero)
            total += 1
            forced = total >= max_steps - 1
            early = j + 1 < SP_CHECK_EVERY and (j + 1) & j == 0
            if not (early or (j + 1) % SP_CHECK_EVERY == 0 or j + 1 == m or forced):
                j += 1
                continue
            if j == 0:
                theta, residual = alpha[0], beta[0]
                if residual <= 0 or last_cycle or total >= max_steps:
                    if trace is not None:
                        trace.update(info)
                    return dtype(2) - theta, residual, V[0], total, restarts
            k, breakdown = j + 1, False
            info['betas'] += [float(b) for i, b in enumerate(beta) if not (capped and i == m - 1)]
            for i in range(j + 1):
                if not beta[i] >= SP_BREAKDOWN:
                    k, breakdown = i + 1, True
                    break
            restart = breakdown or k == m or forced
            if not restart:
                _, y, _ = top_ritz(alpha, beta, k)
                restart = float(beta[k - 1]) * y[k - 1] == 0.0
            if not restart:
                j += 1
                continue
            _, y, info['gap'] = top_ritz(alpha, beta, k)
            info['ritz'].append(k)
            V = [first_column(np.array(V[:k]).T @ y.astype(dtype))]
            restarts += 1
            last_cycle = breakdown or forced
            break


# ---- the allowance ------------------------------------------------------------------------------------------------------------------
def counted(n, d_max, steps, basis):
    """2 |B| steps [2 (d_max + 4) + (2 basis + 4)(n + 2)] 2^-53: the first-order bound on what the float64 roundings of `steps`
    solver steps, each against at most `basis` columns, put into a Ritz value or a residual norm.

    One step, in units of u = 2^-53 relative to the vector it works on, which is at most |B| <= 2 long (the columns are unit
    vectors, B v is at most |B|, and projections and Gram-Schmidt only shorten):
      * the mat-vec: a row adds at most d_max terms (in any order an entry passes through at most d_max additions), z = s v and
        s (.) (A z) one rounding each, s itself two (the square root and the division): d_max + 4; the same again for the z the
        next step reads and the addition of v: 2 (d_max + 4) covers both;
      * every inner product is over at most n entries: in any summation order an entry passes through at most n additions and its
        product is one more rounding, and the update w -= c k it feeds is two more: n + 2 per inner product.  A step takes alpha,
        two deflations (a node lies in one component, so the k_C together are one inner product of length n), the norm, and
        Gram-Schmidt against jc <= basis columns twice: 2 basis + 4 of them.
    The roundings of different steps add (first order); the small tridiagonal problem adds 8 k u |T| <= 16 basis u (numpy's eigh,
    and the device's QL, are backward stable), which the (2 basis + 4)(n + 2) of any one step exceeds.  Stated with the factor 2 in
    front it has a factor of two in hand for the second-order terms.

    What this does NOT bound is how Lanczos amplifies a perturbation of an early column into the later T_k: that has no a priori
    bound short of the condition of the Krylov basis.  The measured distance between the float64 and the longdouble run of
    `schedule` stands in for it (`allow`)."""
    return 2.0 * 2.0 * steps * (2.0 * (d_max + 4) + (2.0 * basis + 4.0) * (n + 2.0)) * 2.0 ** -53


def counted_vector(value, gap):
    """The same for the entries of the Ritz vector: the top eigenvector of T_k moves by at most |dT| / gap, gap the distance of
    the two largest Ritz values of the last T_k; the columns it combines are bounded by `value` already.  No gap at k = 1 (inf),
    and none wider than the spectrum helps: divided by min(gap, 1)."""
    return value / min(float(gap), 1.0)


ORDER_FACTOR = 16.0


def allow(counted_bound, measured):
    """What the device may differ by from the longdouble replica: 16 times the larger of the counted bound and the distance
    measured ON THE CPU between the float64 and the longdouble run of `schedule`.  The device is a float64 evaluation of the same
    quantities in another summation order: it obeys the same error law as the float64 run, and the factor covers the order.  The
    factor is not tuned against the device."""
    return ORDER_FACTOR * max(float(counted_bound), float(measured))


def vector_distance(a, b, signed=True):
    """max |a -+ b| over the better of the two signs (`signed`), or of a - b alone."""
    a, b = np.asarray(a, dtype=L), np.asarray(b, dtype=L)
    d = float(np.abs(a - b).max())
    return min(d, float(np.abs(a + b).max())) if signed else d


# ---- the graphs and cases of tests/test_spectral_steps_{cpu,gpu}.py -------------------------------------------------------------------
SEED = 5
MULTI_SIZES = (1024, 1025, 2049, 2)     # components with an edge, in the order of their smallest node ids; then three isolated nodes
_GRAPHS, _REFS = {}, {}


def union(parts, isolated, perm_seed, first=None):
    """The disjoint union of the graphs `parts` ((edge_index, n) each) and `isolated` more nodes, the node ids permuted by
    Generator(PCG64(perm_seed)).  `first`: the components' ranks by smallest permuted id (part i holds the first[i]-th smallest):
    the permutation is patched by swapping ids 0 .. len(parts) - 1 into place."""
    sizes = [g[1] for g in parts]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    n = int(offs[-1]) + isolated
    perm = np.random.Generator(np.random.PCG64(perm_seed)).permutation(n)
    if first is not None:
        for i, rank in enumerate(first):    # old node offs[i] takes id `rank`; the node that had it takes the id given up
            at = int(np.flatnonzero(perm == rank)[0])
            perm[at], perm[offs[i]] = perm[offs[i]], perm[at]
    ei = np.concatenate([np.asarray(g[0]) + offs[i] for i, g in enumerate(parts)], axis=1)
    out = perm[ei]
    order = np.lexsort((out[1], out[0]))
    return out[:, order], n


def graph(key):
    """(edge_index, n) of a case's graph, built once."""
    if key in _GRAPHS:
        return _GRAPHS[key]
    import fosr_ref
    import scale_ref
    if key.startswith('irregular'):
        n = int(key[len('irregular'):])
        g = fosr_ref.irregular_graph(n, seed=n)
    elif key == 'multi':
        parts = [fosr_ref.irregular_graph(k, seed=100 + k) for k in MULTI_SIZES[:3]] + [spectral_ref.path(2)]
        g = union(parts, 3, perm_seed=4103, first=(0, 1, 2, 3))
    elif key == 'lattice':
        g = scale_ref.diffusion_large()[:2]
    elif key in spectral_ref.PLAN_NAMES:
        g = next((ei, n) for name, ei, n in spectral_ref.plan_family() if name == key)
    elif key == 'path3':
        g = spectral_ref.path(3)
    elif key == 'path4_iso2':
        g = (spectral_ref.path(4)[0], 6)
    elif key == 'k5_k7_iso':
        g = union([spectral_ref.complete(5), spectral_ref.complete(7)], 1, perm_seed=13)
    else:
        raise KeyError(key)
    _GRAPHS[key] = g
    return g


def _cases():
    out = []
    for n in (511, 512, 513, 1024, 1025, 2049):
        for ms in ((1, 2, 3, 8, 9, 10, 25) if n in (513, 2049) else (1, 3, 9)):
            out.append((f'irregular{n}', ms, None))
    out += [('multi', ms, None) for ms in (1, 2, 9, 25)]
    out += [('lattice', ms, None) for ms in (1, 9)]
    out += [(key, ms, None) for key in ('long3_mid9_short63', 'mid34_short0') for ms in (1, 3)]
    out += [('irregular513', 11, 4), ('irregular513', 41, 16)]
    out += [('path3', 3, None), ('path4_iso2', 4, None)]
    return out


CASES = _cases()     # (graph key, max_steps, max_basis)
# complete(34): P B P is a multiple of the identity on the deflated space, so beta_0 is 0 in exact arithmetic: the one graph of the
# cases on which the driver breaks down (at once, and in both precisions: tests/test_spectral_steps_cpu.py asserts how far below
# SP_BREAKDOWN it lands).  Its cases with a restart return after two steps whatever max_steps says.
BREAKS_DOWN = ('mid34_short0',)


def case_id(case):
    key, ms, mb = case
    return f'{key}-steps{ms}' + (f'-basis{mb}' if mb else '')


def operators(key):
    """dict(long=, f64=): the Replica of a case's graph in either precision, built once."""
    ops = _REFS.setdefault(('ops', key), {})
    if not ops:
        ei, n = graph(key)
        ops['long'], ops['f64'] = Replica(ei, n, L), Replica(ei, n, np.float64)
    return ops


def reference(case):
    """The replica's two runs of a case, computed once and shared: dict(long=(lambda1, residual, vector, steps, restarts),
    f64=the same in float64, trace=the longdouble run's, trace64, dist=(|d lambda1|, |d residual|, max |d vector| up to sign),
    n, d_max, basis, counted, counted_vector)."""
    if case in _REFS:
        return _REFS[case]
    key, ms, mb = case
    ops = operators(key)
    tl, t64 = {}, {}
    long_ = schedule(ops['long'], SEED, ms, mb, L, tl)
    f64 = schedule(ops['f64'], SEED, ms, mb, np.float64, t64)
    R = ops['long']
    basis = min(basis_columns(R.n, R.components, mb), max(ms - 1, 1))
    c = counted(R.n, int(R.deg.max()), long_[3], basis)
    _REFS[case] = dict(long=long_, f64=f64, trace=tl, trace64=t64, n=R.n, d_max=int(R.deg.max()), basis=basis,
                       dist=(abs(float(long_[0] - L(f64[0]))), abs(float(long_[1] - L(f64[1]))),
                             vector_distance(long_[2], f64[2], signed=ms > 1)),
                       counted=c, counted_vector=counted_vector(c, tl['gap']))
    return _REFS[case]
