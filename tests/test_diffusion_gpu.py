"""PageRank diffusion on the GPU (csrc/dcr_diffusion.hip) against closed forms, the dense restatement tests/diffusion_ref.py
(pinned on the CPU by tests/test_diffusion_cpu.py) and the reference's two sparsifiers as recorded in
tests/golden/diffusion_reference.json.

The one acceptance rule for values, derived and not measured:   |x_i - S_ij| <= rho_j / alpha + allow,   allow = 64 n 2^-52,
with x the device column, S the dense matrix and rho_j the TRUE residual the call reports: x - S_j = M^-1 (M x - alpha e_j) and
lambda_min(M) >= alpha; allow is the rounding of the dense reference (solve and inv agree within it on every graph used here,
tests/test_diffusion_cpu.py).  The selection is compared bit for bit with a lexsort of the device's own column.

The bits of a column depend on the source and on the graph as it lies in device memory, the order of the neighbours within a row
included (the mat-vec adds a row's neighbours in slot order).  add_edge appends to both rows and remove_edge closes the gap; a
graph built from a sorted edge index has ascending rows.  So the bit-for-bit comparison of a live graph with a fresh one uses an
edge whose ends each become the largest neighbour of the other, where the rows coincide; an edit anywhere else is checked by the
acceptance rule.  No test loops around a failing step."""
import ctypes
import warnings

import numpy as np
import pytest

import diffusion_ref as ref
import scale_ref
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-10
_DENSE = {}


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


def dense(name, alpha):
    """S of a graph of ref.graphs(), computed once."""
    if (name, alpha) not in _DENSE:
        ei, n = ref.graphs()[name]
        _DENSE[name, alpha] = ref.ppr_matrix(ei, n, alpha)
    return _DENSE[name, alpha]


def solve(G, sources, alpha, **kw):
    """ppr that must converge: (columns [P, n], info)."""
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        x, info = G.ppr(sources, alpha=alpha, return_info=True, **kw)
    assert x.dtype == np.float64 and x.shape == (len(sources), G.num_nodes)
    assert info['residual'].dtype == np.float64 and info['steps'].dtype == np.int32 and info['converged'].all()
    return x, info


def sparse(G, alpha, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        ei, w, info = G.diffusion(alpha=alpha, return_info=True, **kw)
    assert ei.dtype == np.int64 and ei.shape == (2, w.size) and w.dtype == np.float64 and info['value'].shape == w.shape
    assert info['ptr'][0] == 0 and info['ptr'][-1] == w.size and info['converged'].all()
    return ei, w, info


def bound(info, alpha, n):
    return info['residual'] / alpha + ref.allow(n)


def accept(x, info, want, alpha, n, label):
    b = bound(info, alpha, n)
    err = np.abs(x - want).max(axis=1)
    print(f'  {label}: {len(x)} columns, max error {err.max():.3e}, bound >= {b.min():.3e}, max residual {info["residual"].max():.3e}, '
          f'steps {info["steps"].min()} .. {info["steps"].max()}')
    assert np.all(err <= b), (label, np.flatnonzero(err > b)[:5], err.max())


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', ref.ALPHAS)
@pytest.mark.parametrize('n', [5, 40])   # complete40: every row in the wave class
def test_ppr_complete_graph_closed_form(dcr, n, alpha):
    ei, _ = ref.complete(n)
    x, info = solve(dcr(ei, n), np.arange(n), alpha)
    accept(x, info, alpha * np.eye(n) + (1 - alpha) / n, alpha, n, f'complete{n}')
    if n == 5:
        assert info['steps'].max() <= 2   # M has two distinct eigenvalues


@pytest.mark.parametrize('alpha', ref.ALPHAS)
def test_ppr_isolated_nodes(dcr, alpha):
    ei, n = ref.triangle_star_isolated()
    x, info = solve(dcr(ei, n), np.arange(n), alpha)
    accept(x, info, ref.ppr_matrix(ei, n, alpha), alpha, n, 'triangle, star, isolated node')
    assert abs(x[8, 8] - 1.0) <= bound(info, alpha, n)[8] and np.all(x[8, :8] == 0.0) and np.all(x[:8, 8] == 0.0)
    E = dcr(np.zeros((2, 0), dtype=np.int64), 5)   # no edges at all: S = I
    x, info = solve(E, [3, 0, 4], alpha)
    assert np.abs(x - np.eye(5)[[3, 0, 4]]).max() <= bound(info, alpha, 5).max()


# ---- 2. against the dense S --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', ref.ALPHAS)
@pytest.mark.parametrize('name', list(ref.graphs()))
def test_ppr_against_dense(dcr, name, alpha):
    ei, n = ref.graphs()[name]
    G = dcr(ei, n)
    if name == 'hub2100':
        assert G.degree(0) == 2100 > 2048   # one workgroup-class row
        src = np.array([0, 1, 2, 17, 2100, 2101, 2102, n - 1, 5, 900, 1500, 2099, 3, 4, 6, 7, 8])
    else:
        src = np.arange(n)
    x, info = solve(G, src, alpha)
    accept(x, info, dense(name, alpha)[src], alpha, n, f'{name} alpha {alpha}')


# ---- 3. the row plan at its boundaries; batch independence ---------------------------------------------------------------------------
def plan_sources(ei, n):
    """A hub, a medium row, a short row and the last short row (the isolated one where there is one), then other nodes."""
    (nl, nm, ns), rows = ref.row_plan(ei, n)
    picked = []
    for lo, hi in ((0, nl), (nl, nl + nm), (nl + nm, n)):
        if hi > lo:
            picked += [int(rows[lo]), int(rows[hi - 1])]
    picked = list(dict.fromkeys(picked))
    others = [v for v in np.random.default_rng(3).permutation(n).tolist() if v not in picked]
    return picked, others


@pytest.mark.parametrize('name', ref.PLAN_NAMES)
def test_ppr_on_the_plan_family_and_batch_independence(dcr, name):
    alpha = 0.15
    ei, n = {g[0]: g[1:] for g in ref.plan_family()}[name]
    G = dcr(ei, n)
    picked, others = plan_sources(ei, n)
    x, info = solve(G, picked, alpha)
    accept(x, info, ref.ppr_columns(ei, n, alpha, picked), alpha, n, f'{name}, sources {picked}')
    want = {s: (x[i].tobytes(), info['residual'][i].hex(), int(info['steps'][i])) for i, s in enumerate(picked)}
    # the first source alone; then 15, 16 and 17 sources with the picked ones at other positions, in other company
    for P in (1, 15, 16, 17):
        fill = others[:P - len(picked)]
        order = {1: picked[:1], 15: fill + picked[::-1], 16: picked[1:] + fill + picked[:1], 17: fill + picked}[P]
        assert len(order) == P
        y, iy = solve(G, order, alpha)
        for i, s in enumerate(order):
            if s in want:
                assert (y[i].tobytes(), iy['residual'][i].hex(), int(iy['steps'][i])) == want[s], (name, P, i, s)


# ---- 3b. past one grid-stride trip of the element-wise kernels; the groups of a launch ------------------------------------------------
LARGE_ALPHA = 0.15
_LARGE = {}


def large_sources():
    """The 17 sources at 33,133 nodes: the hub, a medium row, a lattice corner, an isolated node, the last node, then others."""
    ei, n, names = scale_ref.diffusion_large()
    named = [names['hub0'], names['hub3'], names['corner'], names['isolated'], names['last']]
    others = [v for v in np.random.default_rng(5).permutation(n).tolist() if v not in named]
    return named + others[:scale_ref.DIFFUSION_P - len(named)]


def large_solve(dcr):
    """(graph handle, sources, the device's columns, info), solved once for the value and the selection test."""
    if 'solve' not in _LARGE:
        ei, n, _ = scale_ref.diffusion_large()
        G = dcr(ei, n)
        src = large_sources()
        _LARGE['solve'] = (G, src) + solve(G, src, LARGE_ALPHA)
    return _LARGE['solve']


def test_ppr_past_one_trip_against_the_host_certificate(dcr):
    """n = 33,133: k_col_start / update / direction / scale take a second grid-stride trip, two launches run at one group.  No
    dense matrix exists here, so the reference is a certificate, derived and not measured.  With rho the residual of the device's
    column computed on the host in np.longdouble:
      |rho - reported residual| <= (d_max + 4) 2^-52 | |M| |x| |_2     the forward error of the float64 mat-vec the device performs
      |x - x_ref|_inf <= (rho + rho_ref) / alpha                      x_ref from a sparse LU, rho_ref its own host residual:
    x - S_j = M^-1 (M x - alpha e_j) for both, and lambda_min(M) >= alpha (the argument at the head of this file).  The second
    line is a theorem about the exact residuals, and at an isolated source it holds with near equality (M is the 1 x 1 matrix
    1 - (1 - alpha), the device and the LU land on the two floats either side of alpha / M_jj): there the 2^-64 roundings of
    the host's own np.longdouble residual decide (measured: 4.441e-16 against 4.438e-16).  So rho and rho_ref enter with what
    their own arithmetic can be off by added (ref.residual_long_rounding), which is nothing beside a residual of 1e-11."""
    ei, n, _ = scale_ref.diffusion_large()
    G, src, x, info = large_solve(dcr)
    M, at, _ = ref.sparse_operator(ei, n, LARGE_ALPHA)
    d_max = int(at.getnnz(axis=1).max()) - 1
    assert d_max == G.degree(src[0]) == 2100
    want = ref.lu_columns(M, src, LARGE_ALPHA)
    for i, j in enumerate(src):
        rho, rho_ref = ref.residual_long(at, x[i], j, LARGE_ALPHA), ref.residual_long(at, want[i], j, LARGE_ALPHA)
        slack = ref.matvec_error(M, x[i], d_max)
        err = float(np.abs(x[i] - want[i]).max())
        print(f'  source {j}: reported {info["residual"][i]:.3e}, host {rho:.3e} (may differ by {slack:.3e}), LU {rho_ref:.3e}, '
              f'error {err:.3e} <= {(rho + rho_ref) / LARGE_ALPHA:.3e}, steps {info["steps"][i]}')
        assert abs(rho - info['residual'][i]) <= slack, (j, rho, info['residual'][i], slack)
        own = ref.residual_long_rounding(M, at, x[i]) + ref.residual_long_rounding(M, at, want[i])
        assert err <= (rho + rho_ref + own) / LARGE_ALPHA, (j, err, rho, rho_ref, own)
        assert rho <= TOL * LARGE_ALPHA + slack                      # converged by the host's residual too
    for i in (3, 4):   # the isolated sources: S_jj = 1, nothing else
        assert abs(x[i, src[i]] - 1.0) <= 4 * ref.EPS and np.count_nonzero(x[i]) == 1


def test_selection_past_one_trip_is_the_lexsort_of_the_device_columns(dcr):
    ei, n, _ = scale_ref.diffusion_large()
    G, src, x, _ = large_solve(dcr)
    P = len(src)
    order = np.lexsort((np.broadcast_to(np.arange(n), (P, n)), -x), axis=-1)
    for k in (1, 64, n):
        got_ei, w, info = sparse(G, LARGE_ALPHA, k=k, sources=src)
        assert np.array_equal(np.diff(info['ptr']), np.full(P, k)), k
        rows = got_ei[0].reshape(P, k)
        assert np.array_equal(got_ei[1].reshape(P, k), np.broadcast_to(np.asarray(src)[:, None], (P, k)))
        assert np.array_equal(rows, np.sort(order[:, :k], axis=1)), (k, 'kept sets')
        value = np.take_along_axis(x, rows, axis=1)
        assert info['value'].tobytes() == value.tobytes(), (k, 'values')
        total = np.cumsum(value, axis=1)[:, -1:]           # added in id order, one after the other
        assert np.all(total > 0) and w.tobytes() == (value / total).tobytes(), (k, 'weights')
    eps = load_golden('diffusion_reference.json')['cases'][0]['eps']
    got_ei, w, info = sparse(G, LARGE_ALPHA, eps=eps, sources=src)
    keep = x >= eps
    assert keep.sum() > P and np.array_equal(np.diff(info['ptr']), keep.sum(axis=1))
    jj, ii = np.nonzero(keep)                              # by column, then by node id
    assert np.array_equal(got_ei[0], ii) and np.array_equal(got_ei[1], np.asarray(src)[jj])
    assert info['value'].tobytes() == x[jj, ii].tobytes()
    assert w.tobytes() == np.concatenate([ref.normalise(x[j, keep[j]]) for j in range(P)]).tobytes()


def same_as_solo(G, order, named, y, iy, alpha, label):
    """The named positions of a call: the column, the residual and the step count are those of the source solved alone."""
    for pos in named:
        s = order[pos]
        x1, i1 = solve(G, [s], alpha)
        got = (y[pos].tobytes(), iy['residual'][pos].hex(), int(iy['steps'][pos]))
        assert got == (x1[0].tobytes(), i1['residual'][0].hex(), int(i1['steps'][0])), (label, pos, s)


def test_groups_limited_by_n_leave_the_columns_alone(dcr):
    """About 10,000 nodes: 65,536 // n = 6 groups, not 8 and not the 7 batches of P = 101.  One launch of six groups, then five
    columns alone."""
    ei, n, names = scale_ref.diffusion_groups()
    G = dcr(ei, n)
    P, B = scale_ref.GROUPS_P, 16
    special = [names['hub0'], names['hub1'], names['hub2'], names['corner'], names['isolated'], names['last'], n // 2, 4321]
    named = [0, B + 3, 2 * B + 7, 3 * B + 15, 4 * B, 5 * B + 9, 6 * B, P - 1]   # first, one per group 1 .. 5, the second launch's first, last
    fill = [v for v in np.random.default_rng(7).permutation(n).tolist() if v not in special]
    order = fill[:P]
    for pos, s in zip(named, special):
        order[pos] = s
    assert len(set(order)) == P
    y, iy = solve(G, order, LARGE_ALPHA)
    same_as_solo(G, order, named, y, iy, LARGE_ALPHA, 'six groups')


def test_groups_2_to_7_leave_the_columns_alone(dcr):
    """long3_mid9_short63 with 8 x 16 sources: all eight groups of a launch; the plan's picks sit in groups 2, 5 and 7."""
    ei, n = {g[0]: g[1:] for g in ref.plan_family()}['long3_mid9_short63']
    G = dcr(ei, n)
    picked, others = plan_sources(ei, n)
    assert len(picked) == 6
    P, B = scale_ref.SMALL_GROUPS_P, 16
    named = [2 * B, 2 * B + 15, 5 * B + 1, 5 * B + 8, 7 * B + 6, 7 * B + 15]
    order = others[:P]
    for pos, s in zip(named, picked):
        order[pos] = s
    assert len(set(order)) == P
    y, iy = solve(G, order, LARGE_ALPHA)
    same_as_solo(G, order, named, y, iy, LARGE_ALPHA, 'eight groups')


# ---- 4. the selection, exactly -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', ref.ALPHAS)
@pytest.mark.parametrize('name', list(ref.graphs()))
def test_selection_is_the_lexsort_of_the_device_columns(dcr, name, alpha):
    ei, n = ref.graphs()[name]
    assert n % 16 != 0
    G = dcr(ei, n)
    x, _ = solve(G, np.arange(n), alpha)       # row j = column j
    order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), -x), axis=-1)
    assert np.array_equal(order[0], np.lexsort((np.arange(n), -x[0])))
    for k in (1, 8, n - 1, n, n + 5):
        kk = min(k, n)
        got_ei, w, info = sparse(G, alpha, k=k)
        assert np.array_equal(np.diff(info['ptr']), np.full(n, kk)), (name, k)
        rows = got_ei[0].reshape(n, kk)
        assert np.array_equal(got_ei[1].reshape(n, kk), np.broadcast_to(np.arange(n)[:, None], (n, kk)))
        assert np.array_equal(rows, np.sort(order[:, :kk], axis=1)), (name, k, 'kept sets')
        value = np.take_along_axis(x, rows, axis=1)
        assert info['value'].tobytes() == value.tobytes(), (name, k, 'values')
        total = np.cumsum(value, axis=1)[:, -1:]           # added in id order, one after the other
        assert np.all(total > 0) and w.tobytes() == (value / total).tobytes(), (name, k, 'weights')
    fixture_eps = load_golden('diffusion_reference.json')['cases'][0]['eps']
    for eps in (fixture_eps, 2.0, -1.0):
        got_ei, w, info = sparse(G, alpha, eps=eps)
        keep = x >= eps
        assert np.array_equal(np.diff(info['ptr']), keep.sum(axis=1)), (name, eps)
        jj, ii = np.nonzero(keep)                          # by column, then by node id
        assert np.array_equal(got_ei[0], ii) and np.array_equal(got_ei[1], jj), (name, eps)
        assert info['value'].tobytes() == x[jj, ii].tobytes()
        want_w = np.concatenate([ref.normalise(x[j, keep[j]]) for j in range(n)]) if ii.size else np.empty(0)
        assert w.tobytes() == want_w.tobytes(), (name, eps, 'weights')
        if eps == 2.0:
            assert w.size == 0 and got_ei.shape == (2, 0)
        if eps == -1.0:
            assert w.size == n * n


def test_selection_of_a_subset_of_sources_in_any_order(dcr):
    ei, n = ref.graphs()['barbell20_4']
    G = dcr(ei, n)
    src = np.array([43, 0, 21, 22, 7, 7, 19, 20, 23, 24, 1, 2, 3, 4, 5, 6, 8, 9, 42])   # 19 columns, one twice
    x, _ = solve(G, src, 0.15)
    got_ei, w, info = sparse(G, 0.15, k=8, sources=src)
    assert np.array_equal(got_ei[1], np.repeat(src, 8))
    for i in range(len(src)):
        assert np.array_equal(got_ei[0][8 * i:8 * i + 8], ref.top_k(x[i], 8))
        assert w[8 * i:8 * i + 8].tobytes() == ref.normalise(x[i, ref.top_k(x[i], 8)]).tobytes()


# ---- 5. the selection against the reference's helpers ----------------------------------------------------------------------------------
def test_selection_reproduces_the_reference_helpers(dcr):
    fx = load_golden('diffusion_reference.json')
    (fn, args), = fx['graph'].items()
    ei, n = getattr(ref, fn)(*args)
    G = dcr(ei, n)
    for case in fx['cases']:
        alpha = case['alpha']
        for name, kw in (('top_k', {'k': fx['k']}), ('clipped', {'eps': case['eps']})):
            want_ptr, want_rows, want_w = ref.recorded(GOLDEN, fx, case[name])
            got_ei, w, info = sparse(G, alpha, **kw)
            assert np.array_equal(info['ptr'], want_ptr), (alpha, name)                       # every column, none left out
            assert np.array_equal(got_ei[0], want_rows), (alpha, name)
            assert np.array_equal(got_ei[1], np.repeat(np.arange(n), np.diff(want_ptr)))
            kept_sum = np.add.reduceat(info['value'], want_ptr[:-1])
            b = np.repeat(bound(info, alpha, n) / kept_sum, np.diff(want_ptr))
            err = np.abs(w - want_w)
            print(f'  alpha {alpha} {name}: {w.size} entries, max weight error {err.max():.3e}, bound >= {b.min():.3e}')
            assert np.all(err <= b), (alpha, name, err.max())


@pytest.mark.parametrize('alpha', ref.ALPHAS)
@pytest.mark.parametrize('name', ['path8', 'cycle7', 'star6', 'barbell20_4', 'random300'])
def test_selection_against_dense_outside_the_tie_zone(dcr, name, alpha):
    ei, n = ref.graphs()[name]
    S = dense(name, alpha)
    k = 8
    kk = min(k, n)
    got_ei, w, info = sparse(dcr(ei, n), alpha, k=k)
    assert np.array_equal(np.diff(info['ptr']), np.full(n, kk))
    b = bound(info, alpha, n)
    tied = 0
    for j in range(n):
        kept = np.zeros(n, dtype=bool)
        kept[got_ei[0][kk * j:kk * j + kk]] = True
        kth = np.sort(S[:, j])[::-1][kk - 1]
        assert kept[S[:, j] > kth + b[j]].all() and not kept[S[:, j] < kth - b[j]].any(), (name, j)
        tied += int((np.abs(S[:, j] - kth) <= b[j]).sum() > 1)
    print(f'  {name} alpha {alpha}: {tied} of {n} columns with more than the k-th value in the tie zone')


# ---- 6. interface ------------------------------------------------------------------------------------------------------------------
def test_errors_empty_and_capacity(dcr):
    from dcr import _lib
    ei, n = ref.path(8)
    G = dcr(ei, n)
    for kw in ({}, {'k': 3, 'eps': 0.1}):
        with pytest.raises(ValueError):
            G.diffusion(**kw)
    for bad in (0.0, 1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            G.ppr([0], alpha=bad)
        with pytest.raises(ValueError):
            G.diffusion(alpha=bad, k=2)
    for src in ([n], [-1], [0, 8]):
        with pytest.raises(ValueError):
            G.ppr(src)
        with pytest.raises(ValueError):
            G.diffusion(k=2, sources=src)
    with pytest.raises(ValueError):
        G.diffusion(k=0)
    with pytest.raises(ValueError):
        G.ppr([0], max_steps=0)
    with pytest.raises(ValueError):
        G.ppr([0], tol=-1.0)
    x, info = G.ppr([], return_info=True)
    assert x.shape == (0, n) and info['steps'].shape == (0,)
    e, w, info = G.diffusion(k=3, sources=[], return_info=True)
    assert e.shape == (2, 0) and w.shape == (0,) and info['ptr'].tolist() == [0]
    # the C ABI
    L = _lib.lib()
    i32, f64, i64 = ctypes.c_int32, ctypes.c_double, ctypes.c_int64
    src = (i32 * 2)(1, 6)
    out, res, ptr, nnz = (f64 * (2 * n))(), (f64 * 2)(-7.0, -7.0), (i64 * 3)(-7, -7, -7), i64(-7)
    row, wgt, val = (i32 * 6)(), (f64 * 6)(), (f64 * 6)()
    assert L.dcr_ppr_columns(None, src, 2, None, out, res, None) == -1
    assert L.dcr_ppr_columns(G._h, None, 2, None, out, res, None) == -1
    assert L.dcr_ppr_columns(G._h, src, 2, None, None, res, None) == -1
    assert L.dcr_ppr_columns(G._h, src, 2, None, out, None, None) == -1
    assert L.dcr_ppr_columns(G._h, src, -1, None, out, res, None) == -1
    assert L.dcr_ppr_columns(G._h, src, 0, None, out, res, None) == 0 and res[0] == -7.0 and out[0] == 0.0
    assert L.dcr_ppr_columns(G._h, src, 2, None, out, res, None) == 0       # NULL options are the defaults, steps may be NULL
    assert 0.0 <= res[0] <= TOL * 0.15 and abs(sum(out[:n]) - sum(ref.ppr_matrix(ei, n, 0.15)[:, 1])) <= 1e-9

    def sparsify(g=G._h, sources=src, P=2, mode=0, k=3, eps=0.0, ptr=ptr, cap=6, row=row, wgt=wgt, val=val, res=res, nnz=nnz):
        return L.dcr_diffusion_sparsify(g, sources, P, None, mode, k, eps, ptr, cap, row, wgt, val, res, None, ctypes.byref(nnz) if nnz is not None else None)
    assert sparsify(g=None) == -1 and sparsify(ptr=None) == -1 and sparsify(res=None) == -1 and sparsify(nnz=None) == -1
    assert sparsify(row=None) == -1 and sparsify(wgt=None) == -1 and sparsify(val=None) == -1
    assert sparsify(mode=2) == -1 and sparsify(k=0) == -1 and sparsify(mode=1, eps=float('nan')) == -1 and sparsify(cap=-1) == -1
    assert sparsify(sources=None) == -1                                       # NULL sources stand for all nodes: P must be n
    assert sparsify(P=0) == 0 and ptr[0] == -7 and nnz.value == -7
    assert sparsify(cap=5) == -4 and nnz.value == 6                           # top-k: known before any solve
    assert sparsify(cap=0, row=None, wgt=None, val=None) == -4 and nnz.value == 6
    assert sparsify() == 0 and nnz.value == 6 and list(ptr) == [0, 3, 6]
    assert list(row) == [0, 1, 2, 5, 6, 7] and abs(sum(wgt[:3]) - 1.0) <= 1e-15 and abs(sum(wgt[3:]) - 1.0) <= 1e-15
    # threshold: the count comes out of the solve; too small a cap returns it with the pointers, a counting call needs no arrays
    S = ref.ppr_matrix(ei, n, 0.15)
    need = int((S[:, [1, 6]] >= 0.05).sum())
    assert need > 2
    assert sparsify(mode=1, eps=0.05, cap=2) == -4 and nnz.value == need and ptr[2] == need
    nnz.value = -7
    assert sparsify(mode=1, eps=0.05, cap=0, row=None, wgt=None, val=None) == -4 and nnz.value == need
    big = need + 1
    row2, wgt2, val2 = (i32 * big)(), (f64 * big)(), (f64 * big)()
    assert sparsify(mode=1, eps=0.05, cap=big, row=row2, wgt=wgt2, val=val2) == 0 and nnz.value == need
    assert list(row2[:ptr[1]]) == np.flatnonzero(S[:, 1] >= 0.05).tolist()
    allp, allnnz = (i64 * (n + 1))(), i64()
    rown, wn, vn, resn = (i32 * (2 * n))(), (f64 * (2 * n))(), (f64 * (2 * n))(), (f64 * n)()
    assert L.dcr_diffusion_sparsify(G._h, None, n, None, 0, 2, 0.0, allp, 2 * n, rown, wn, vn, resn, None, ctypes.byref(allnnz)) == 0
    assert allnnz.value == 2 * n and list(allp) == list(range(0, 2 * n + 1, 2))


def test_cut_short_warns(dcr):
    ei, n = ref.graphs()['barbell20_4']
    G = dcr(ei, n)
    with pytest.warns(RuntimeWarning):
        x, info = G.ppr([0, 21, 43], alpha=0.05, max_steps=1, return_info=True)
    assert not info['converged'].any() and np.all(info['steps'] == 1)
    assert np.all(np.abs(x - dense('barbell20_4', 0.05)[[0, 21, 43]]).max(axis=1) <= bound(info, 0.05, n))   # the rule holds for any iterate
    with pytest.warns(RuntimeWarning):
        G.diffusion(alpha=0.05, k=4, max_steps=1)


def test_live_graph_edits(dcr):
    ei, n = ref.random_graph(300, 5)
    A = ref.adjacency(ei, n)
    v = n - 1
    u = max(w for w in range(v) if A[v, w] == 0)
    assert u > np.flatnonzero(A[v]).max() and v > np.flatnonzero(A[u]).max()    # each end becomes the other's largest neighbour
    G = dcr(ei, n)
    before = sparse(G, 0.15, k=8)
    G.add_edge(u, v)
    a, b = 7, int(np.flatnonzero(A[7])[0])
    G.remove_edge(a, b)
    live = sparse(G, 0.15, k=8)
    fresh = sparse(dcr(G.to_edge_index(), n), 0.15, k=8)
    assert not np.array_equal(before[0], live[0])
    assert np.array_equal(live[0], fresh[0]) and live[1].tobytes() == fresh[1].tobytes()
    for key in ('value', 'residual', 'steps', 'ptr'):
        assert live[2][key].tobytes() == fresh[2][key].tobytes(), key
    # an edge appended in the middle of two rows' order: other bits, the same matrix
    G.add_edge(3, 150) if A[3, 150] == 0 else G.add_edge(3, 151)
    now = G.to_edge_index()
    src = [3, 150, 151, 7, 299]
    x, info = solve(G, src, 0.15)
    accept(x, info, ref.ppr_columns(now, n, 0.15, src), 0.15, n, 'after three edits')


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------
def test_digl_feeds_the_gcn():
    import torch
    from dcr import synthetic
    from dcr.data import Data, Dataset
    from gcn_fp64 import gcn_logits
    from models.gcn import GCN
    from rewiring.diffusion import digl
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    g = torch.Generator(device='cuda').manual_seed(5)
    x = torch.rand(n, 96, device='cuda', generator=g)
    y = torch.randint(0, 7, (n,), device='cuda', generator=g)
    data = Data(x=x, edge_index=torch.from_numpy(ei).cuda(), y=y, num_nodes=n)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        out = digl(data, alpha=0.15, k=16)
    assert out.x is x and out.y is y and out.num_nodes == n and data.edge_attr is None
    assert out.edge_index.shape == (2, 16 * n) and out.edge_index.dtype == torch.int64 and out.edge_index.is_cuda
    assert out.edge_attr.shape == (16 * n,) and out.edge_attr.dtype == torch.float32
    sums = torch.zeros(n, device='cuda', dtype=torch.float64).index_add_(0, out.edge_index[1], out.edge_attr.double())
    assert (sums - 1).abs().max().item() <= 16 * 2.0 ** -24                  # every column's weights sum to one
    torch.manual_seed(3)
    model = GCN(Dataset(out, 7), hidden=[64], dropout=0.5).cuda()
    model.eval()
    with torch.no_grad():
        logits = model(out)
        weights = [(l.lin.weight.detach().double(), l.bias.detach().double()) for l in model.layers]
        want = gcn_logits(weights, x, out.edge_index, n, edge_weight=out.edge_attr)
    assert (logits.double() - want).abs().max().item() < 1e-5
    from dcr.graph import DcrGraph
    live = digl(DcrGraph(ei, n), alpha=0.15, k=16)                           # a live graph: the same edges and weights
    assert torch.equal(live.edge_index, out.edge_index.cpu()) and torch.equal(live.edge_attr, out.edge_attr.cpu())
