"""Host replica of the batched column conjugate gradients of csrc/dcr_analysis.h (k_col_start, k_col_matvec<P, 0 / 1>, k_col_update,
k_col_direction, k_col_scale and col_cg_solve), step by step, for the tests to hold the kernels to (numpy, and scipy where
resistance_ref uses it; nothing here imports the package's device code).

The device solves COL_B independent CGs in step, and a column's arithmetic is its own: `cg` restates ONE column.  Cut at
``max_steps = k`` the public calls return the whole state after k steps: ``DcrGraph.ppr`` the iterate x_k, the TRUE residual
|alpha e_j - M x_k| of the closing mat-vec and the step count; ``DcrGraph.effective_resistance`` lower_k = 2 c.y_k - y_k.L'y_k, the
true |c - L' y_k| and the step count.  In exact arithmetic these are functions of the graph, the right-hand side and k alone, and the
replica states them in np.longdouble; ``dtype=np.float64`` runs the same code in the device's precision, and the distance between the
two runs is what the allowance of the GPU test rests on (`allow`).

The operators (`Operator`), from an (edge_index, n), as the device applies them:
  PageRank     M = I - (1 - alpha) D~^-1/2 (A + I) D~^-1/2: q = v - damp (s~ (.) (A z + z)), z = s~ (.) v, s~ = 1 / sqrt(deg + 1);
               rhs alpha e_j, |rhs|^2 = alpha^2, stop = tol alpha
  resistance   L' = I - D^-1/2 A D^-1/2: q = v - s (.) (A z), z = s (.) v, s = 1 / sqrt(deg); a zero row and s = 0 at an isolated node;
               rhs c = s_u e_u - s_v e_v, |c|^2 = s_u^2 + s_v^2, stop = tol sqrt(|c|^2).  u == v and pairs in different components are
               decided by the host without a solve, as dcr_effective_resistance decides them (`host_decided`).
A is a dense 0/1 matrix up to DENSE_MAX nodes and the scipy CSR matrix above (in np.longdouble through
spectral_ref.csr_matvec_long, a row's products added from left to right)."""
import os
import re
import time

import numpy as np

import hops_ref
import resistance_ref
import scale_ref
import spectral_ref
from conftest import PKG
from spectral_lanczos_ref import ORDER_FACTOR

L = np.longdouble
U = 2.0 ** -53
DENSE_MAX = 4096
DEFAULT_MAX_STEPS = 20000    # dcr_resistance_opts / dcr_diffusion_opts


def _source(name):
    with open(os.path.join(PKG, 'csrc', name)) as f:
        return f.read()


def _int_constant(text, name):
    m = re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, text)
    assert m, name + ' not found'
    return int(m.group(1))


_HEADER = _source('dcr_analysis.h')
SP_CHECK_EVERY = _int_constant(_HEADER, 'SP_CHECK_EVERY')     # solver steps between host synchronisations
# the two lines of col_cg_solve that decide when the host looks at the control blocks, and that it stops only then
HOST_LOOKS = (r'if \(\(step \+ 1\) % SP_CHECK_EVERY != 0 && step \+ 1 != max_steps\) continue;',
              r'for \(int i = 0; i < ng; \+\+i\) active \+= host\[i\]\.cg\.active;\s*if \(active == 0\) break;')
for _pattern in HOST_LOOKS:
    assert re.search(_pattern, _HEADER), 'the steps at which col_cg_solve looks at its control blocks'


# ---- one column -----------------------------------------------------------------------------------------------------------------
class Run:
    """What `cg` returns.  iterates[i] and rnorm[i]: x and the recurrence's |r| after i counted steps (iterates[0] = 0,
    rnorm[0] = |rhs|); steps: the steps counted; launch: the 1-based solver step in which the column froze, None while it runs;
    reason: 'converged', 'not finite' (both in the update: launch == steps) or 'breakdown' (in the mat-vec: launch == steps + 1)."""

    def __init__(self):
        self.iterates, self.rnorm, self.steps, self.launch, self.reason = [], [], 0, None, None

    def x(self, k):
        """The iterate after k solver steps: a frozen column stays put."""
        return self.iterates[min(k, self.steps)]

    def steps_at(self, k):
        return min(k, self.steps)

    def frozen_at(self, k):
        return self.launch is not None and k >= self.launch


MUTATIONS = ('stale beta', 'stale gain', 'late freeze', 'counted breakdown')


def cg(apply, rhs, stop, max_steps, dtype, rr0=None, mutate=None):
    """One column of col_cg_solve, literally: x = 0, r = p = rhs, rr = |rhs|^2 (rr0 where the start kernel forms it from the
    right-hand side's entries alone).  Per step q = apply(p) (k_col_matvec<P, 0>); p.q not a positive finite number: the column
    freezes with gain 0 and NO step is counted; else gain = rr / p.q, x += gain p, r -= gain q (k_col_update), beta = rr_new / rr,
    rr = rr_new, steps += 1, and the column freezes when rr_new is not finite or sqrt(rr_new) <= stop; only a column that is not
    frozen forms p = r + beta p (k_col_direction).  A frozen column is no longer written, so the loop ends there.

    `mutate` breaks the recurrence on purpose, for tests/test_column_cg_cpu.py to show that the comparison notices:
    'stale beta' (beta from the rr of the step before), 'stale gain' (gain from the rr of the step before), 'late freeze'
    (sqrt(rr) <= stop / 16), 'counted breakdown' (the step counted in the p.q branch)."""
    assert mutate is None or mutate in MUTATIONS
    rhs = np.asarray(rhs, dtype=dtype)
    x, r, p = np.zeros_like(rhs), rhs.copy(), rhs.copy()
    rr = dtype(rhs @ rhs if rr0 is None else rr0)
    stop = dtype(stop)
    out = Run()
    out.iterates.append(x.copy())
    out.rnorm.append(np.sqrt(rr))
    rr_before = rr      # the rr of the step before: what a stale read would see
    for launch in range(1, int(max_steps) + 1):
        q = apply(p)
        pq = dtype(p @ q)
        if not (pq > 0 and np.isfinite(pq)):
            out.launch, out.reason = launch, 'breakdown'
            if mutate == 'counted breakdown':
                out.steps += 1
                out.iterates.append(x.copy())
                out.rnorm.append(np.sqrt(rr))
            break
        gain = (rr_before if mutate == 'stale gain' else rr) / pq
        x = x + gain * p
        r = r - gain * q
        rr_new = dtype(r @ r)
        beta = rr / rr_before if mutate == 'stale beta' else rr_new / rr
        rr_before, rr = rr, rr_new
        out.steps += 1
        out.iterates.append(x.copy())
        out.rnorm.append(np.sqrt(rr))
        if not np.isfinite(rr):
            out.launch, out.reason = launch, 'not finite'
            break
        if np.sqrt(rr) <= (stop / 16 if mutate == 'late freeze' else stop):
            out.launch, out.reason = launch, 'converged'
            break
        p = r + beta * p
    return out


# ---- the operators ----------------------------------------------------------------------------------------------------------------
class Operator:
    """M ('ppr', with alpha) or L' ('resistance') of one graph in `dtype`; see the module docstring."""

    def __init__(self, edge_index, n, kind, dtype=L, alpha=None):
        assert kind in ('ppr', 'resistance')
        self.n, self.kind, self.dtype = int(n), kind, dtype
        self.csr = resistance_ref._sparse_adjacency(edge_index, n)
        self.csr.sort_indices()
        self.deg = np.diff(self.csr.indptr).astype(np.int64)
        self.d_max = int(self.deg.max())
        self.dense = self.csr.toarray().astype(dtype) if n <= DENSE_MAX else None
        d = self.deg.astype(dtype)
        if kind == 'ppr':
            self.alpha = dtype(alpha)       # the float64 the caller passes, exactly
            self.damp = dtype(1) - self.alpha
            self.s = dtype(1) / np.sqrt(d + dtype(1))
        else:
            self.s = np.zeros(n, dtype=dtype)
            self.s[self.deg > 0] = dtype(1) / np.sqrt(d[self.deg > 0])
        self.labels = None

    def _adj(self, z):
        if self.dense is not None:
            return self.dense @ z
        return spectral_ref.csr_matvec_long(self.csr, z) if self.dtype is L else self.csr @ z

    def apply(self, v):
        z = self.s * v
        if self.kind == 'ppr':
            return v - self.damp * (self.s * (self._adj(z) + z))
        return np.where(self.deg > 0, v - self.s * self._adj(z), self.dtype(0))

    def rhs(self, column):
        """(rhs, |rhs|^2 as the start kernel forms it) of a source node or a pair (u, v)."""
        c = np.zeros(self.n, dtype=self.dtype)
        if self.kind == 'ppr':
            c[int(column)] = self.alpha
            return c, self.alpha * self.alpha
        u, v = (int(t) for t in column)
        c[u], c[v] = self.s[u], -self.s[v]
        return c, self.s[u] * self.s[u] + self.s[v] * self.s[v]

    def stop(self, column, tol):
        """The threshold of the column's recurrence: tol alpha, or tol sqrt(|c|^2)."""
        tol = self.dtype(tol)
        return tol * self.alpha if self.kind == 'ppr' else tol * np.sqrt(self.rhs(column)[1])

    def closing(self, x, column):
        """(|rhs - (operator) x|, lower): what the closing mat-vec makes of an iterate, in this operator's dtype (np.longdouble for
        the reference); lower = 2 c.x - x.(L' x) for the resistance, None for PageRank."""
        x = np.asarray(x, dtype=self.dtype)
        c, _ = self.rhs(column)
        w = self.apply(x)
        e = c - w
        resid = np.sqrt(e @ e)
        if self.kind == 'ppr':
            return resid, None
        u, v = (int(t) for t in column)
        return resid, self.dtype(2) * (self.s[u] * x[u] - self.s[v] * x[v]) - x @ w

    def solve(self, column, tol, max_steps, mutate=None):
        c, rr0 = self.rhs(column)
        return cg(self.apply, c, self.stop(column, tol), max_steps, self.dtype, rr0=rr0, mutate=mutate)

    def components(self):
        if self.labels is None:
            import scipy.sparse.csgraph
            self.labels = scipy.sparse.csgraph.connected_components(self.csr, directed=False)[1]
        return self.labels

    def host_decided(self, column):
        """None, or the `lower` of a pair that takes no column: 0.0 for u == v, inf across components."""
        if self.kind == 'ppr':
            return None
        u, v = (int(t) for t in column)
        if u == v:
            return 0.0
        return float('inf') if self.components()[u] != self.components()[v] else None


# ---- the allowance ------------------------------------------------------------------------------------------------------------------
def counted(n, d_max, k, scale):
    """2 scale k [(d_max + 7) + 2 (n + 1) + 4] 2^-53: the first-order bound on what the float64 roundings of `k` solver steps put
    into an entry of x_k, whose vector is at most `scale` long; with the scale of `lower_k` or of the residual norm, and k + 1 for
    the closing mat-vec, into those.

    One step, in units of u = 2^-53 relative to the vector it works on:
      * the mat-vec: a row adds at most d_max neighbours and its own z (in any order an entry passes through at most d_max + 1
        additions); z = s p, s (.) (A z), the factor 1 - alpha and the subtraction from p one rounding each, s itself two (the
        square root and the division): d_max + 7;
      * two inner products over n entries, p.q and |r|^2: in any summation order an entry passes through at most n additions and
        its product is one more rounding: n + 1 each.  They reach x through the step length rr / p.q, a relative error of the
        update gain p, which is no longer than x's bound;
      * the two updates x += gain p and r -= gain q: two roundings each, 4.
    The roundings of different steps add (first order), and the factor 2 in front is in hand for the second-order terms.  `scale`
    is the size of what is bounded: |x| <= |rhs| / lambda_min(M) = alpha / alpha = 1 for PageRank and |y| <= |c| / lambda_1 for the
    resistance (lambda_1 from resistance_ref.Dense or resistance_ref.lambda1_lower); the residual norm moves by at most
    |operator| <= 2 times what x moves by.  lower = 2 c.y - y.L'y is stationary in y up to the residual: it moves by 2 r.dy,
    r = c - L'y, at most 2 rmax times what y moves by, rmax the largest |r_j| of the longdouble recurrence up to the last cut
    (>= |c| = |r_0|; CG's residual norm is not monotone: 3.1 |c| on the barbell); its own two inner products add
    (n + 1) u (2 |c| |y| + |y| |L'y|) <= (n + 1) u |y| (3 |c| + rmax), which (|c| + rmax) times the counted bound of y covers:
    4 rmax |y| in all.  `scales` states the three.

    What this does NOT bound is how CG amplifies an early perturbation: a rounding of step i changes the direction p_i and through
    it every later gain and beta, and after the exact arithmetic would have terminated (the barbell's columns) the iterate moves
    by the condition number times the recurrence's residual.  There is no a priori bound for that short of the operator's
    condition; the measured distance between the float64 and the longdouble run of `cg` stands in for it (`allow`)."""
    return 2.0 * float(scale) * k * ((d_max + 7.0) + 2.0 * (n + 1.0) + 4.0) * U


def scales(kind, cnorm=None, lambda1=None, rmax=None):
    """dict(x=, residual=, lower=): the `scale` of `counted` for each pinned quantity."""
    if kind == 'ppr':
        return dict(x=1.0, residual=2.0, lower=None)
    y = float(cnorm) / float(lambda1)
    return dict(x=y, residual=2.0 * y, lower=4.0 * float(rmax) * y)


def allow(counted_bound, measured):
    """What the device may differ by from the longdouble replica: ORDER_FACTOR (spectral_lanczos_ref's 16) times the larger of
    the counted bound and the distance measured ON THE CPU between the float64 and the longdouble run of `cg` at the same step.
    The device is a float64 evaluation of the same quantities in another summation order: it obeys the same error law as the
    float64 run, and the factor covers the order.  Nothing is tuned against the device."""
    return ORDER_FACTOR * max(float(counted_bound), float(measured))


# ---- the graphs and the case table of tests/test_column_cg_{cpu,gpu}.py ---------------------------------------------------------------
def two_cycles(m=22):
    """The disjoint union of two m-node cycles: node i of a cycle is joined to i +- 1 (mod m); 2 m nodes in two components."""
    i = np.arange(m, dtype=np.int64)
    one = np.stack([np.concatenate([i, (i + 1) % m]), np.concatenate([(i + 1) % m, i])])
    ei = np.concatenate([one, one + m], axis=1)
    return ei[:, np.lexsort((ei[1], ei[0]))], 2 * m


_GRAPHS, _REFS = {}, {}


def graph(key):
    """(edge_index, n) of a case's graph, built once."""
    if key not in _GRAPHS:
        if key == 'irregular330':
            g = hops_ref.irregular330()
        elif key == 'long3_mid9_short63':
            g = next((ei, n) for name, ei, n in spectral_ref.plan_family() if name == key)
        elif key == 'barbell20_4':
            g = resistance_ref.barbell(20, 4)
        elif key == 'lattice':
            g = scale_ref.diffusion_large()[:2]
        elif key == 'two_cycles22':
            g = two_cycles(22)
        else:
            raise KeyError(key)
        _GRAPHS[key] = (np.asarray(g[0], dtype=np.int64), int(g[1]))
    return _GRAPHS[key]


def _degrees(key):
    ei, n = graph(key)
    return np.bincount(ei[0], minlength=n)


def _columns_A():
    """Node 0, the maximum-degree node, node n - 1 (isolated), and 37 nodes spread by a fixed stride: 40 sources, three batches."""
    n = graph('irregular330')[1]
    top = int(np.argmax(_degrees('irregular330')))
    assert top == 2
    rest = [6 + 8 * i for i in range(37)]
    out = [0, top, n - 1] + rest
    assert len(set(out)) == 40
    return out


def _columns_B():
    """A hub (degree > 2,048: a workgroup a row), a wave-class node, a short row, a leaf of a hub, the isolated node."""
    names = spectral_ref.plan_nodes('long3_mid9_short63')
    return [names['hub0'], names['hub7'], names['leaf_first'], names['leaf_last'], names['isolated']]


def _pairs_C():
    """(3, 30), (0, 43), (0, 1), (20, 21), a same-node pair, and 13 more pairs: 17 that take a column, so the second batch holds
    one pair and 15 padding columns."""
    return [(3, 30), (0, 43), (0, 1), (20, 21), (7, 7), (19, 20), (19, 24), (21, 22), (22, 23), (5, 22), (23, 40), (24, 43), (0, 19),
            (19, 5), (20, 22), (23, 20), (12, 21), (41, 22)]


def _pairs_D():
    """Six pairs that take a column, one of them with a degree-1 endpoint, and one across components (node n - 1 is isolated)."""
    deg = _degrees('irregular330')
    leaf = int(np.flatnonzero(deg == 1)[0])
    return [(0, 2), (leaf, 0), (1, 200), (100, 326), (50, 51), (2, 300), (4, 329)]


def _lattice_sources():
    names = scale_ref.diffusion_large()[2]
    return [names['hub0'], 33_000, names['isolated']]


def _all_to(last):
    return list(range(1, last + 1))


_E_CUTS = [1, 2, 3, SP_CHECK_EVERY + 1]
_B_CUTS = [1, 2, 3, SP_CHECK_EVERY - 1, SP_CHECK_EVERY, SP_CHECK_EVERY + 1, 2 * SP_CHECK_EVERY, 2 * SP_CHECK_EVERY + 1]

# name -> graph key, operator, parameters, columns and the cut steps k.  cuts: a function of the largest freeze step of the case's
# columns (the longdouble replica's), or None where the columns are run to fixed cuts only.  `full`: one more call at the default
# max_steps.  `asserted_freeze`: whether the GPU test asserts steps == min(k, f), which the threshold condition of
# tests/test_column_cg_cpu.py licenses column by column.
CASES = {
    'A': dict(graph='irregular330', kind='ppr', alpha=0.15, tol=1e-10, columns=_columns_A,
              cuts=lambda f: _all_to(f + SP_CHECK_EVERY), full=False),
    'B': dict(graph='long3_mid9_short63', kind='ppr', alpha=0.15, tol=1e-10, columns=_columns_B,
              cuts=lambda f: sorted(set(_B_CUTS)), freeze_cuts=True, full=True),
    'C': dict(graph='barbell20_4', kind='resistance', tol=1e-10, columns=_pairs_C, cuts=lambda f: _all_to(f + 2), full=False),
    'D': dict(graph='irregular330', kind='resistance', tol=1e-10, columns=_pairs_D, cuts=lambda f: _all_to(f), full=False),
    'E-ppr': dict(graph='lattice', kind='ppr', alpha=0.15, tol=1e-10, columns=_lattice_sources, cuts=lambda f: list(_E_CUTS),
                  run_to=max(_E_CUTS), full=False),
    'E-resistance': dict(graph='lattice', kind='resistance', tol=1e-10, columns=lambda: [(33_000, 33_100)],
                         cuts=lambda f: list(_E_CUTS), run_to=max(_E_CUTS), full=False),
    # tol = 0: stop = 0, so the column freezes only in the mat-vec's p.q branch or at an exact rr == 0.  c = s (e_0 - e_11) has
    # components along six distinct eigenvalues of the 22-cycle's L', so CG terminates after 6 steps in exact arithmetic and what
    # follows is rounding (|r| of the float64 recurrence: 2.4e-16 after step 6, 1.7e-31 after step 12; neither precision freezes
    # within F_PROBED steps).  The replica runs every cut 1 .. F_PROBED, two windows of the host and one step; the GPU test pins
    # F_CUTS, the cuts among them at which the CPU-measured distance keeps every allowance below F_ALLOWANCE_CAP: all of them,
    # k = 1 .. 17 (the largest allowance, the residual's at k = 17, is 3.3e-10; tests/test_column_cg_cpu.py asserts that F_CUTS
    # are exactly those cuts).
    'F': dict(graph='two_cycles22', kind='resistance', tol=0.0, columns=lambda: [(0, 11)], cuts=lambda f: _all_to(F_PROBED),
              run_to=None, full=False),
}
F_PROBED = 2 * SP_CHECK_EVERY + 1
F_CUTS = tuple(range(1, 2 * SP_CHECK_EVERY + 2))
F_ALLOWANCE_CAP = 1e-9
CASES['F']['run_to'] = F_PROBED
CASES['F']['pinned'] = F_CUTS


def operators(name):
    """dict(long=, f64=): the Operator of a case in either precision, built once per (graph, kind, alpha)."""
    case = CASES[name]
    key = ('ops', case['graph'], case['kind'], case.get('alpha'))
    if key not in _REFS:
        ei, n = graph(case['graph'])
        _REFS[key] = dict(long=Operator(ei, n, case['kind'], L, case.get('alpha')),
                          f64=Operator(ei, n, case['kind'], np.float64, case.get('alpha')))
    return _REFS[key]


def lambda1(name):
    """lambda_1 of the normalised Laplacian of a resistance case's graph (of the component of the first pair, where the graph
    has several): the dense eigenvalue up to DENSE_MAX nodes, resistance_ref.lambda1_lower's bound above."""
    case = CASES[name]
    key = ('lambda1', case['graph'])
    if key not in _REFS:
        ei, n = graph(case['graph'])
        if n > DENSE_MAX:
            _REFS[key] = resistance_ref.lambda1_lower(ei, n, int(case['columns']()[0][0]))[0]
        elif case['graph'] == 'two_cycles22':
            _REFS[key] = resistance_ref.Dense(*resistance_ref.cycle(22)).lambda1
        else:
            _REFS[key] = resistance_ref.Dense(ei, n).lambda1
    return _REFS[key]


class Column:
    """One column of a case: its two runs and what is expected of the device at every cut."""


def result_at(op, run, column, k):
    """dict(x, residual, lower, steps) of a run cut at k, the closing in the operator's own precision."""
    x = run.x(k)
    resid, lower = op.closing(x, column)
    return dict(x=x, residual=resid, lower=lower, steps=run.steps_at(k))


def reference(name):
    """The replica's two runs of every column of a case, computed once and shared: dict(case, n, d_max, columns, cuts, pinned
    (the cuts the GPU test asserts: all of them but in case F), f_max, seconds) with columns a list of Column: .column, .decided (the host's `lower`, or None), .long / .f64 (the Runs), .stop,
    .f (the longdouble run's counted steps when it froze, None if it did not), .scales, and per cut k .want[k] (x, residual, lower,
    steps in np.longdouble), .dist[k] (x, residual, lower: |float64 - longdouble|), .allow[k] (the same three allowances)."""
    key = ('ref', name)
    if key in _REFS:
        return _REFS[key]
    t0 = time.perf_counter()
    case, ops = CASES[name], operators(name)
    long_, f64 = ops['long'], ops['f64']
    run_to = case.get('run_to') or DEFAULT_MAX_STEPS
    cols = []
    for column in case['columns']():
        c = Column()
        c.column, c.decided = column, long_.host_decided(column)
        if c.decided is None:
            c.long, c.f64 = long_.solve(column, case['tol'], run_to), f64.solve(column, case['tol'], run_to)
            c.stop = f64.stop(column, case['tol'])
            c.f = c.long.steps if c.long.launch is not None else None
            cnorm = float(np.sqrt(long_.rhs(column)[1])) if case['kind'] == 'resistance' else None
            c.scales = scales(case['kind'], cnorm, lambda1(name) if case['kind'] == 'resistance' else None, max(float(t) for t in c.long.rnorm))
        cols.append(c)
    solved = [c for c in cols if c.decided is None]
    f_max = max((c.f for c in solved if c.f is not None), default=0)
    cuts = list(case['cuts'](f_max))
    if case.get('freeze_cuts'):     # the frozen-stays-frozen comparison needs the call with max_steps = f
        cuts = sorted(set(cuts) | {c.f for c in solved if c.f is not None})
    if case['full']:
        cuts.append(DEFAULT_MAX_STEPS)
    for c in solved:
        c.want, c.dist, c.allow = {}, {}, {}
        for k in cuts:
            w, g = result_at(long_, c.long, c.column, k), result_at(f64, c.f64, c.column, k)
            c.want[k] = w
            c.dist[k] = dict(x=float(np.abs(w['x'] - g['x'].astype(L)).max()), residual=abs(float(w['residual'] - L(g['residual']))),
                             lower=None if w['lower'] is None else abs(float(w['lower'] - L(g['lower']))))
            steps = max(w['steps'], 1)
            c.allow[k] = {q: None if c.scales[q] is None else
                          allow(counted(long_.n, long_.d_max, steps + (q != 'x'), c.scales[q]), c.dist[k][q])
                          for q in ('x', 'residual', 'lower')}
    _REFS[key] = dict(case=case, name=name, n=long_.n, d_max=long_.d_max, columns=cols, cuts=cuts, f_max=f_max,
                      pinned=[k for k in cuts if k in case.get('pinned', cuts)],
                      seconds=time.perf_counter() - t0)
    return _REFS[key]


def columns_array(name):
    """What the device call takes: the sources as int32 [P], or the pairs as int64 [P, 2]."""
    cols = CASES[name]['columns']()
    return np.asarray(cols, dtype=np.int32) if CASES[name]['kind'] == 'ppr' else np.asarray(cols, dtype=np.int64).reshape(-1, 2)


def expect_converged(c, k):
    """A column is converged after k steps exactly when the recurrence froze it as converged by then: the threshold condition of
    tests/test_column_cg_cpu.py keeps |r| clear of stop on both sides, and the true residual is the recurrence's to rounding.  A
    breakdown freeze is judged by the residual, as the API documents: at tol = 0 never, short of an exact zero."""
    return c.long.reason == 'converged' and c.long.launch <= k


def replica_result(name, k, dtype=np.float64, mutate=None):
    """What a device that ran this replica in `dtype` would return for the case cut at k, in the layout of `compare`'s `got`:
    dict(x [P, n] (PageRank) or lower [P] (resistance), residual [P], steps [P], converged [P])."""
    case = CASES[name]
    op = operators(name)['long' if dtype is L else 'f64']
    key = ('mutant', name, dtype, mutate)
    if key not in _REFS:
        run_to = case.get('run_to') or DEFAULT_MAX_STEPS
        if mutate is not None:      # a broken recurrence need not converge: no further than the cuts look
            run_to = min(run_to, max(reference(name)['cuts']))
        _REFS[key] = [None if op.host_decided(col) is not None else op.solve(col, case['tol'], run_to, mutate)
                      for col in case['columns']()]
    cols = case['columns']()
    P = len(cols)
    out = dict(residual=np.zeros(P), steps=np.zeros(P, dtype=np.int32), converged=np.ones(P, dtype=bool))
    if case['kind'] == 'ppr':
        out['x'] = np.zeros((P, op.n))
    else:
        out['lower'] = np.zeros(P)
    for i, (col, run) in enumerate(zip(cols, _REFS[key])):
        if run is None:
            out['lower'][i] = op.host_decided(col)
            continue
        r = result_at(op, run, col, k)
        out['residual'][i], out['steps'][i] = float(r['residual']), r['steps']
        out['converged'][i] = float(r['residual']) <= float(op.stop(col, case['tol']))
        if case['kind'] == 'ppr':
            out['x'][i] = r['x'].astype(np.float64)
        else:
            out['lower'][i] = float(r['lower'])
    return out


def compare(name, k, got, want, show=None):
    """The failed assertions, as strings, of a result `got` (the layout of `replica_result`: the device's, or a mutated replica's)
    for case `name` cut at max_steps = k against `want` = reference(name); [] when it passes.  Per column: steps == min(k, f);
    the iterate (PageRank), lower (resistance) and the residual within the allowance of the longdouble replica's; converged
    exactly as the replica says; a host-decided pair has steps 0, residual 0.0 and its lower.  `show`: a list that receives one
    line per column (distance next to allowance)."""
    fails = []
    kind = want['case']['kind']
    for i, c in enumerate(want['columns']):
        tag = f'{name} k={k} column {i} ({c.column})'
        if c.decided is not None:
            if not (got['steps'][i] == 0 and got['residual'][i] == 0.0 and got['lower'][i] == c.decided and got['converged'][i]):
                fails.append(f'{tag}: host-decided pair returned steps {got["steps"][i]}, residual {got["residual"][i]!r}, '
                             f'lower {got["lower"][i]!r}, converged {got["converged"][i]}')
            continue
        w, a = c.want[k], c.allow[k]
        if int(got['steps'][i]) != w['steps']:
            fails.append(f'{tag}: steps {int(got["steps"][i])}, the replica {w["steps"]}')
        d = {}
        if kind == 'ppr':
            d['x'] = float(np.abs(np.asarray(got['x'][i], dtype=L) - w['x']).max())
        else:
            d['lower'] = abs(float(L(got['lower'][i]) - w['lower']))
        d['residual'] = abs(float(L(got['residual'][i]) - w['residual']))
        for q, dist in d.items():
            if not dist <= a[q]:
                fails.append(f'{tag}: {q} off by {dist:.3e}, allowed {a[q]:.3e}')
        if bool(got['converged'][i]) != expect_converged(c, k):
            fails.append(f'{tag}: converged {bool(got["converged"][i])}, the replica {expect_converged(c, k)} '
                         f'(residual {got["residual"][i]:.3e}, stop {float(c.stop):.3e})')
        if show is not None:
            show.append(f'{tag}: steps {int(got["steps"][i])} ({w["steps"]}) ' +
                        ' '.join(f'|d {q}| {dist:.3e} (allowed {a[q]:.3e})' for q, dist in d.items()))
    return fails
