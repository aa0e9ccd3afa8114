"""Host replica of the heat kernel's Taylor recurrence (k_heat_start, k_heat_term, k_heat_mass and the loop of diffusion_batches in
csrc/dcr_diffusion.hip), term by term: the partial sum X^(k) = sum_{m <= k} theta_m H^m e_j at every requested cut k, in np.longdouble
(the recurrence of heat_ref.taylor_long, run once) and in float64 in the device's operation order, with hooks that break it on
purpose; the ball of radius k, outside of which X^(k) is exactly zero; the acceptance rule both compare a column with, entry by
entry and relative; and the cases of tests/test_heat_steps_cpu.py and tests/test_heat_steps_gpu.py.  Also `accept`, the rule of
tests/test_heat_gpu.py, so that it and the tests that show what it lets through share one copy.  Nothing here imports the package
under test."""
import numpy as np

import diffusion_ref
import heat_ref as ref
import hops_ref
import scale_ref
import spectral_ref
from spectral_ref import LONG_DEG, SHORT_DEG, csr_matvec_long

L = np.longdouble
TOL = ref.TOL
UNDERFLOW = L(2) ** -960    # every positive entry of a replica's partial sum lies above this: no rounding below is a subnormal's
MUTATIONS = ('m1', 'm2', 'm3', 'm4', 'm5', 'm6')
M4_FROM = 1536              # m4: the slots of a long row from here on are left out of the gather
M5_VALUE = 1e-300           # m5: what an entry outside the ball is set to
M6_BELOW, M6_REL = 1e-12, 1e-3   # m6: entries below M6_BELOW are multiplied by 1 + M6_REL


# ---- the rule of tests/test_heat_gpu.py -------------------------------------------------------------------------------------------------
def accept(x, info, want, oracle, ei, n, src, t, label):
    """The acceptance rule of the head of tests/test_heat_gpu.py for the columns `src`, and the two statements about the deficit."""
    _, _, r, deg = ref.operator_long(ei, n)
    K, d_max = info['terms'], int(deg.max()) if n else 0
    a = ref.allow(K, d_max)
    src = np.asarray(src, dtype=np.int64)
    diff = np.asarray(want, dtype=L) - x
    hi = info['deficit'].astype(L)[:, None] / r[None, :]   # deficit_j / r_i
    print(f'  {label}: {len(x)} columns, K {K}, want - x in [{float(diff.min()):.3e}, {float(diff.max()):.3e}], allow {a:.3e}, '
          f'oracle {float(oracle):.3e}, deficit {info["deficit"].min():.3e} .. {info["deficit"].max():.3e}')
    assert np.all(x >= 0.0)
    assert np.all(diff >= -a), (label, 'above the oracle', float(diff.min()))
    assert np.all(diff <= hi + a + oracle), (label, 'below the bound', float((diff - hi).max()))
    own = r[src] - x.astype(L) @ r                       # the deficit of the device's own column
    slack = (n + 2) * ref.EPS * r[src]
    got = info['deficit'].astype(L)
    assert np.all(np.abs(got - own) <= slack), (label, 'deficit of the own column', float(np.abs(got - own).max()))
    assert np.all(np.abs(got - r[src] * ref.tail(t, K)) <= slack + a * r[src]), (label, 'deficit against r rho_K')


# ---- the longdouble replica -------------------------------------------------------------------------------------------------------------
def partial_sums(edge_index, n, t, sources, cuts):
    """{k: X^(k) as [len(sources), n] np.longdouble} for every k of `cuts` (k = 0 is e^-t e_j), from ONE run of the recurrence of
    heat_ref.taylor_long per source, operation for operation: the entry at k is bit for bit taylor_long(..., K=k)."""
    at, s, _, _ = ref.operator_long(edge_index, n)
    cuts = sorted(set(int(k) for k in cuts))
    out = {k: np.zeros((len(sources), n), dtype=L) for k in cuts}
    for i, j in enumerate(sources):
        v = np.zeros(n, dtype=L)
        v[j] = np.exp(-L(t))
        x = v.copy()
        if 0 in out:
            out[0][i] = x
        for k in range(cuts[-1] if cuts else 0):
            v = (L(t) / L(k + 1)) * (s * csr_matvec_long(at, s * v))
            x += v
            if k + 1 in out:
                out[k + 1][i] = x
    return out


# ---- the float64 replica, in the device's operation order ----------------------------------------------------------------------------------
class Gather:
    """(A z)_row as csrc/dcr_analysis.h::gather adds it, for all columns at once (z is [n, P]).  The lanes of a row's scope take
    the slots lane, lane + stride, ... one after the other from 0.0; a butterfly adds the lanes of a wave (x + shuffled x: the same
    bits in every lane); a long row's four wave sums are then added in wave order.  Slot lanes (256 / COL_CP a workgroup): 32 in
    four waves for a long row, 8 for a medium row's wave, 4 for a short row's 32 lanes.  A lane with nothing left adds 0.0 here,
    which changes no bit.  The neighbours of a row in id order, as a fresh handle has them.  drop_long_from: the slots of a long
    row from that one on are left out (mutation m4)."""

    def __init__(self, edge_index, n, drop_long_from=None):
        a = spectral_ref.adjacency(edge_index, n)
        a.sort_indices()
        indptr, indices = a.indptr.astype(np.int64), a.indices.astype(np.int64)
        self.n, self.deg = n, np.diff(indptr)
        long_, short = self.deg > LONG_DEG, self.deg <= SHORT_DEG
        self.plans = []
        for rows, stride, waves in ((np.flatnonzero(long_), 32, 4), (np.flatnonzero(~long_ & ~short), 8, 1), (np.flatnonzero(short), 4, 1)):
            if rows.size == 0 or self.deg[rows].max() == 0:
                continue
            d = self.deg[rows]
            steps = -(-int(d.max()) // stride)
            slot = np.arange(steps * stride, dtype=np.int64)
            live = slot[None, :] < d[:, None]
            if drop_long_from is not None and waves == 4:
                live &= slot[None, :] < drop_long_from
            at = np.minimum(indptr[rows][:, None] + slot[None, :], indices.size - 1)
            idx = np.where(live, indices[at], n).reshape(rows.size, steps, stride)   # n: a row of zeros
            self.plans.append((rows, idx, stride, waves))

    def __call__(self, z):
        zext = np.vstack([z, np.zeros((1, z.shape[1]))])
        out = np.zeros_like(z)
        for rows, idx, stride, waves in self.plans:
            acc = np.zeros((rows.size, stride, z.shape[1]))
            for step in range(idx.shape[1]):
                acc += zext[idx[:, step, :]]
            per = stride // waves
            acc = acc.reshape(rows.size, waves, per, -1)
            off = per // 2
            while off:
                acc = acc + acc[:, :, np.arange(per) ^ off]
                off //= 2
            total = acc[:, 0, 0]
            for w in range(1, waves):
                total = total + acc[:, w, 0]
            out[rows] = total
        return out


def partial_sums_f64(edge_index, n, t, sources, cuts, mutate=None):
    """({k: x^(k) [len(sources), n] float64}, {k: deficit [len(sources)] float64}) of the device's recurrence in its float64 and its
    order: s~ = 1 / sqrt(deg + 1), x = e^-t e_j, z = s~ x; per term acc from Gather, v = c * (s~_u * (acc + z_in[u])) with
    c = t / (k + 1), x += v, z_out = s~_u * v, the two z buffers by turns; deficit_j = sqrt(deg_j + 1) - sum_i sqrt(deg_i + 1) x_i.
    mutate: None, or one of
      'm1'  the z buffers are not swapped: every term reads the first buffer and writes the second;
      'm2'  c = t / k instead of t / (k + 1) (from the second term on; the first would divide by zero);
      'm3'  the self term + z_in[u] dropped for rows of degree above 2,048;
      'm4'  the slots from 1,536 on of a row longer than 2,048 left out of the gather.
    ('m5' and 'm6' change a finished column: `spoil`.)"""
    assert mutate in (None, 'm1', 'm2', 'm3', 'm4')
    gather = Gather(edge_index, n, drop_long_from=M4_FROM if mutate == 'm4' else None)
    src = np.asarray(sources, dtype=np.int64)
    P = src.size
    root = np.sqrt(gather.deg.astype(np.float64) + 1.0)
    s = (1.0 / root)[:, None]
    keep_self = np.where(gather.deg > LONG_DEG, 0.0, 1.0)[:, None] if mutate == 'm3' else None
    cuts = sorted(set(int(k) for k in cuts))
    x = np.zeros((n, P))
    x[src, np.arange(P)] = np.exp(-np.float64(t))
    z = [s * x, np.zeros((n, P))]
    xs = {}
    if 0 in cuts:
        xs[0] = x.T.copy()
    for k in range(cuts[-1] if cuts else 0):
        z_in, z_out = (0, 1) if mutate == 'm1' else (k % 2, (k + 1) % 2)
        c = np.float64(t) / np.float64(k if mutate == 'm2' and k > 0 else k + 1)
        zu = z[z_in] if keep_self is None else z[z_in] * keep_self
        v = c * (s * (gather(z[z_in]) + zu))
        x = x + v
        z[z_out] = s * v
        if k + 1 in cuts:
            xs[k + 1] = x.T.copy()
    return xs, {k: deficit_f64(xk, gather.deg, src) for k, xk in xs.items()}


def deficit_f64(x, deg, sources):
    """sqrt(deg_j + 1) - sum_i sqrt(deg_i + 1) x_i in float64, the sum added one entry after the other."""
    root = np.sqrt(np.asarray(deg, dtype=np.float64) + 1.0)
    return root[np.asarray(sources, dtype=np.int64)] - np.cumsum(x * root[None, :], axis=1)[:, -1]


def spoil(x, mutate, ball):
    """A copy of the columns x [P, n] with 'm5': the first entry outside the ball (`ball` [P, n] bool) of every column that has
    one set to 1e-300; 'm6': a relative error of 1e-3 on every entry below 1e-12.  Also the number of entries changed."""
    x = x.copy()
    if mutate == 'm5':
        rows = np.flatnonzero((~ball).any(axis=1))
        x[rows, np.argmin(ball[rows], axis=1)] = M5_VALUE
        return x, rows.size
    assert mutate == 'm6'
    small = (x > 0.0) & (x < M6_BELOW)
    x[small] *= 1.0 + M6_REL
    return x, int(small.sum())


# ---- the support ----------------------------------------------------------------------------------------------------------------------
def distances(edge_index, n, sources):
    """Hop distances [len(sources), n] int32 from hops_ref, -1 where there is no path."""
    return hops_ref.hops_sparse(edge_index, n, sources)[0]


def support(edge_index, n, source, k, dist=None):
    """bool [n]: the ball of radius k about `source`.  Every term of the sum is non-negative and (H^m)_ij > 0 exactly where a walk
    of m steps leads from j to i (a walk may wait: H has a positive diagonal), so X^(k)_i > 0 exactly on this ball."""
    d = distances(edge_index, n, [source])[0] if dist is None else dist
    return (d >= 0) & (d <= k)


# ---- the acceptance rule ------------------------------------------------------------------------------------------------------------------
def compare(x, deficit, X, k, t, edge_index, n, sources, dist=None):
    """Columns x [P, n] and deficits [P] of a call cut at k terms against X = partial_sums(...)[k].  All of it is derived:
      relative   |x_i - X_i| <= a X_i with a = heat_ref.allow(k, d_max), used as its derivation states it: componentwise and
                 relative (the replica's own longdouble rounding is 2^-11 of it, inside the factor of two allow keeps in hand);
      support    x_i == 0.0 exactly outside the ball of radius k, x_i > 0 inside;
      deficit    |deficit_j - r_j rho_k| <= ((n + 2) 2^-52 + a) r_j, rho_k = heat_ref.tail(t, k).
    The relative bound assumes that nothing underflows: asserted of X, whose smallest positive entry must lie above 2^-960, as
    is that X itself is positive exactly on the ball (both are facts about the case, not about x).  dist: distances(...) of the
    sources, where the caller has them.  Returns a dict: 'fails' (a list of lines, empty where x passes) and the figures the
    tests print: 'ratio' max |x - X| / (a X), 'rel' max |x - X| / X, 'allow' a, 'deficit' max |deficit - r rho| / r and
    'deficit_allow'."""
    _, _, r, deg = ref.operator_long(edge_index, n)
    a = ref.allow(k, int(deg.max()) if n else 0)
    src = np.asarray(sources, dtype=np.int64)
    x, X = np.asarray(x, dtype=np.float64), np.asarray(X, dtype=L)
    dist = distances(edge_index, n, src) if dist is None else dist
    ball = (dist >= 0) & (dist <= k)
    assert x.shape == X.shape == ball.shape == (src.size, n) and np.asarray(deficit).shape == (src.size,)
    assert np.array_equal(X > 0, ball), 'the replica is positive exactly on the ball'
    assert X[ball].min() > UNDERFLOW, ('the case underflows: lower its cuts', k, float(X[ball].min()))
    fails = []

    def note(what, where):
        rows, cols = np.nonzero(where)
        if rows.size:
            i, v = int(rows[0]), int(cols[0])
            fails.append(f'k {k}: {what}: {rows.size} entries, the first at source {int(src[i])} node {v} (hops {int(dist[i, v])}): '
                         f'x {x[i, v]!r} X {float(X[i, v])!r}')

    note('not exactly 0.0 outside the ball', ~ball & (x != 0.0))
    note('not positive inside the ball', ball & ~(x > 0.0))
    err = np.abs(x.astype(L) - X)
    note(f'beyond the relative allowance {a:.3e}', ball & ~(err <= a * X))
    rel = np.where(ball, err / np.where(ball, X, L(1)), L(0))
    dd = np.abs(np.asarray(deficit, dtype=np.float64).astype(L) - r[src] * ref.tail(t, k)) / r[src]
    da = (n + 2) * ref.EPS + a
    for i in np.flatnonzero(~(dd <= da)):
        fails.append(f'k {k}: deficit of source {int(src[i])}: {deficit[i]!r} against r rho_k {float(r[src[i]] * ref.tail(t, k))!r}, '
                     f'|difference| / r {float(dd[i]):.3e} allowed {da:.3e}')
    return dict(fails=fails, ratio=float(rel.max() / a), rel=float(rel.max()), allow=a, deficit=float(dd.max()), deficit_allow=da)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _every(K):
    return range(1, K + 1)


def _ends(K):
    return (1, 2, K)


# label -> (case, graph, sources, t, cuts from K); graph and sources are built when a unit is first asked for
_SPECS = {'A barbell20_4': ('A', lambda: ref.graphs()['barbell20_4'], lambda g: range(44), 5.0, _every)}
_SPECS.update({f'B {name}': ('B', lambda name=name: {g[0]: g[1:] for g in diffusion_ref.plan_family()}[name], lambda g: _theirs().plan_sources(*g)[0],
                             5.0, lambda K: (1, 2, 3, K - 1, K)) for name in diffusion_ref.PLAN_NAMES})
_SPECS.update({f'C hub2100 t {t}': ('C', lambda: ref.graphs()['hub2100'], lambda g: _theirs().HUB_SOURCES, t, _ends) for t in (0.5, 20.0)})
_SPECS.update({
    'D path300': ('D', lambda: spectral_ref.path(300), lambda g: (0, 150, 299), 20.0, lambda K: [1, 2] + list(range(5, K, 5)) + [K]),
    'E triangle_star_isolated': ('E', diffusion_ref.triangle_star_isolated, lambda g: range(9), 0.5, _every),
    'F lattice33133': ('F', lambda: scale_ref.diffusion_large()[:2], lambda g: _theirs().large_sources(), 5.0, lambda K: (1, 2, 3, K)),
    'G path8 t 256': ('G', lambda: diffusion_ref.path(8), lambda g: (2, 7), 256.0, _ends),
})
LABELS = tuple(_SPECS)
_UNITS, _REFERENCE = {}, {}


def _theirs():
    """tests/test_heat_gpu.py, whose sources the cases B, C and F take (imported late: that file imports `accept` from here)."""
    import test_heat_gpu
    return test_heat_gpu


def labels(*cases):
    """The labels of the units of the given cases.  A unit is one graph at one t; a case of the table in the docstring of
    tests/test_heat_steps_gpu.py is one or more of them."""
    return [label for label in LABELS if _SPECS[label][0] in cases]


def unit(label):
    """dict(case, graph, n, sources, t, K, cuts); K = heat_ref.terms(t, TOL), the device's own count at the default tol."""
    if label not in _UNITS:
        case, graph, sources, t, cuts = _SPECS[label]
        g = graph()
        K = ref.terms(t, TOL)
        cuts = sorted(set(int(k) for k in cuts(K)))
        assert cuts[0] >= 1 and cuts[-1] == K
        _UNITS[label] = dict(case=case, graph=g[0], n=g[1], sources=[int(v) for v in sources(g)], t=t, K=K, cuts=cuts)
    return _UNITS[label]


def reference(label):
    """The unit with 'X': partial_sums at its cuts, one run, and 'dist': the hop distances of its sources.  Computed once."""
    if label not in _REFERENCE:
        u = dict(unit(label))
        u['X'] = partial_sums(u['graph'], u['n'], u['t'], u['sources'], u['cuts'])
        u['dist'] = distances(u['graph'], u['n'], u['sources'])
        _REFERENCE[label] = u
    return _REFERENCE[label]


def compare_unit(label, k, x, deficit):
    u = reference(label)
    return compare(x, deficit, u['X'][k], k, u['t'], u['graph'], u['n'], u['sources'], dist=u['dist'])
