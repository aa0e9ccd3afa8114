"""Heat-kernel diffusion on the GPU (DcrGraph.heat, DcrGraph.diffusion(kernel='heat'), csrc/dcr_diffusion.hip) against the closed
form of the complete graph and the two host oracles of tests/heat_ref.py (held against each other by tests/test_heat_cpu.py): the
recurrence in np.longdouble with 40 terms more, and the spectral form.  Test for test the counterpart of
tests/test_diffusion_gpu.py, at its shapes.

The one acceptance rule for values, derived and not measured, with x the device column, K its number of terms, r = sqrt(deg + 1):
    -allow(K, d_max)  <=  want_i - x_i  <=  deficit_j / r_i + allow(K, d_max) + oracle allowance.
In exact arithmetic the partial sum is an entrywise lower bound of S_j and lacks the mass r_j rho_K, which is what the call reports
as the deficit (H r = r), so 0 <= S_ij - x_i <= deficit_j / r_i; allow is the rounding of the device's float64 recurrence
(heat_ref.allow has the count).  The oracle allowance is rho_{K + 40} for the longdouble recurrence and 64 n 2^-52 for the dense
one.  The deficit itself: within (n + 2) 2^-52 r_j of the deficit of the device's own column added up in np.longdouble (n products
and n - 1 additions of non-negative numbers whose sum is at most r_j, r_j itself, the subtraction), and within that plus
allow r_j of r_j rho_K (the errors of x are relative, and sum_i r_i x_i <= r_j).

The selection is compared bit for bit with a lexsort of the device's own columns.  The bits of a column depend on the order of
the neighbours within a row, so the live-graph test edits where the rows of a fresh handle coincide, as the PageRank test does.  No
test loops around a failing step."""
import ctypes
import warnings

import numpy as np
import pytest

import diffusion_ref
import heat_ref as ref
import scale_ref
from conftest import load_golden
from heat_steps_ref import accept   # the acceptance rule of the head of this file; tests/test_heat_steps_cpu.py shows what it lets through

pytestmark = pytest.mark.gpu

L = np.longdouble
TOL = ref.TOL
HEAT_TS = ref.HEAT_TS
HUB_SOURCES = [0, 1, 2, 17, 2100, 2101, 2102, 2103, 5, 900, 1500, 2099, 3, 4, 6, 7, 8]


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


def solve(G, sources, t, **kw):
    """heat that must not be cut short: (columns [P, n], info)."""
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        x, info = G.heat(sources, t=t, return_info=True, **kw)
    assert x.dtype == np.float64 and x.shape == (len(sources), G.num_nodes)
    assert info['deficit'].dtype == np.float64 and info['deficit'].shape == (len(sources),) and info['converged'].all()
    assert info['terms'] == ref.terms(t, kw.get('tol', TOL))
    return x, info


def sparse(G, t, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        ei, w, info = G.diffusion(kernel='heat', t=t, return_info=True, **kw)
    assert ei.dtype == np.int64 and ei.shape == (2, w.size) and w.dtype == np.float64 and info['value'].shape == w.shape
    assert info['ptr'][0] == 0 and info['ptr'][-1] == w.size and info['converged'].all() and info['terms'] == ref.terms(t, TOL)
    assert 'residual' not in info and 'steps' not in info
    return ei, w, info


def against_taylor(G, ei, n, src, t, label, **kw):
    x, info = solve(G, src, t, **kw)
    K = info['terms']
    accept(x, info, ref.taylor_long(ei, n, t, src, K + ref.ORACLE_EXTRA), ref.tail(t, K + ref.ORACLE_EXTRA), ei, n, src, t, label)
    return x, info


# ---- 1. closed form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', HEAT_TS)
@pytest.mark.parametrize('n', [5, 40])   # complete40: every row in the wave class
def test_heat_complete_graph_closed_form(dcr, n, t):
    """H = J / n, so S = e^-t I + (1 - e^-t) J / n; in np.longdouble, within four of its roundings."""
    ei, _ = diffusion_ref.complete(n)
    x, info = solve(dcr(ei, n), np.arange(n), t)
    e = np.exp(-L(t))
    want = e * np.eye(n, dtype=L) + (L(1) - e) / L(n)
    accept(x, info, want, 4 * float(np.finfo(L).eps), ei, n, np.arange(n), t, f'complete{n} t {t}')


# ---- 2. isolated nodes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', HEAT_TS)
def test_heat_isolated_nodes(dcr, t):
    ei, n = diffusion_ref.triangle_star_isolated()
    x, info = solve(dcr(ei, n), np.arange(n), t)
    accept(x, info, ref.dense(ei, n, t), ref.dense_allow(n), ei, n, np.arange(n), t, 'triangle, star, isolated node')
    K = info['terms']
    assert 0.0 <= 1.0 - x[8, 8] <= info['deficit'][8] + ref.allow(K, 4) and np.all(x[8, :8] == 0.0) and np.all(x[:8, 8] == 0.0)
    assert np.all(x[:3, 3:] == 0.0) and np.all(x[3:8, :3] == 0.0)       # nothing crosses components
    none = np.zeros((2, 0), dtype=np.int64)
    x, info = solve(dcr(none, 5), [3, 0, 4], t)                              # no edges at all: S = I
    accept(x, info, np.eye(5)[[3, 0, 4]], 0.0, none, 5, [3, 0, 4], t, 'no edges')
    assert np.count_nonzero(x) == 3 and np.all(x[[0, 1, 2], [3, 0, 4]] > 0.999)


# ---- 3. against the dense S --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', HEAT_TS)
@pytest.mark.parametrize('name', list(ref.graphs()))
def test_heat_against_dense(dcr, name, t):
    ei, n = ref.graphs()[name]
    G = dcr(ei, n)
    if name == 'hub2100':
        assert G.degree(0) == 2100 > 2048   # one workgroup-class row
        src = np.array(HUB_SOURCES)
    else:
        src = np.arange(n)
    x, info = solve(G, src, t)
    accept(x, info, ref.dense(ei, n, t, key=name)[src], ref.dense_allow(n), ei, n, src, t, f'{name} t {t}')


# ---- 4. the row plan at its boundaries; batch independence ---------------------------------------------------------------------------
def plan_sources(ei, n):
    """A hub, a medium row, a short row and the last short row (the isolated one where there is one), then other nodes: the
    sources of the PageRank test."""
    (nl, nm, ns), rows = diffusion_ref.row_plan(ei, n)
    picked = []
    for lo, hi in ((0, nl), (nl, nl + nm), (nl + nm, n)):
        if hi > lo:
            picked += [int(rows[lo]), int(rows[hi - 1])]
    picked = list(dict.fromkeys(picked))
    others = [v for v in np.random.default_rng(3).permutation(n).tolist() if v not in picked]
    return picked, others


@pytest.mark.parametrize('name', diffusion_ref.PLAN_NAMES)
def test_heat_on_the_plan_family_and_batch_independence(dcr, name):
    t = 5.0
    ei, n = {g[0]: g[1:] for g in diffusion_ref.plan_family()}[name]
    G = dcr(ei, n)
    picked, others = plan_sources(ei, n)
    x, info = against_taylor(G, ei, n, picked, t, f'{name}, sources {picked}')
    want = {s: (x[i].tobytes(), info['deficit'][i].hex()) for i, s in enumerate(picked)}
    # the first source alone; then 15, 16 and 17 sources with the picked ones at other positions, in other company
    for P in (1, 15, 16, 17):
        fill = others[:P - len(picked)]
        order = {1: picked[:1], 15: fill + picked[::-1], 16: picked[1:] + fill + picked[:1], 17: fill + picked}[P]
        assert len(order) == P
        y, iy = solve(G, order, t)
        for i, s in enumerate(order):
            if s in want:
                assert (y[i].tobytes(), iy['deficit'][i].hex()) == want[s], (name, P, i, s)


# ---- 5. past one grid-stride trip of the element-wise kernels ------------------------------------------------------------------------
LARGE_T = 5.0
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
        _LARGE['solve'] = (G, src) + solve(G, src, LARGE_T)
    return _LARGE['solve']


def test_heat_past_one_trip_against_the_longdouble_recurrence(dcr):
    """n = 33,133: k_heat_start and k_heat_mass take a second grid-stride trip, two launches run at one group.  No dense matrix
    exists here; the recurrence in np.longdouble needs none."""
    ei, n, _ = scale_ref.diffusion_large()
    G, src, x, info = large_solve(dcr)
    assert n * 8 > 1024 * 256 and G.degree(src[0]) == 2100
    K = info['terms']
    accept(x, info, ref.taylor_long(ei, n, LARGE_T, src, K + ref.ORACLE_EXTRA), ref.tail(LARGE_T, K + ref.ORACLE_EXTRA), ei, n, src,
           LARGE_T, 'lattice of 33,133')
    for i in (3, 4):   # the isolated sources: S_jj = 1, nothing else
        assert 0.0 <= 1.0 - x[i, src[i]] <= info['deficit'][i] + ref.allow(K, 0) and np.count_nonzero(x[i]) == 1


def test_heat_selection_past_one_trip_is_the_lexsort_of_the_device_columns(dcr):
    ei, n, _ = scale_ref.diffusion_large()
    G, src, x, sinfo = large_solve(dcr)
    P = len(src)
    order = np.lexsort((np.broadcast_to(np.arange(n), (P, n)), -x), axis=-1)
    for k in (1, 64, n):
        got_ei, w, info = sparse(G, LARGE_T, k=k, sources=src)
        assert info['deficit'].tobytes() == sinfo['deficit'].tobytes()
        assert np.array_equal(np.diff(info['ptr']), np.full(P, k)), k
        rows = got_ei[0].reshape(P, k)
        assert np.array_equal(got_ei[1].reshape(P, k), np.broadcast_to(np.asarray(src)[:, None], (P, k)))
        assert np.array_equal(rows, np.sort(order[:, :k], axis=1)), (k, 'kept sets')
        value = np.take_along_axis(x, rows, axis=1)
        assert info['value'].tobytes() == value.tobytes(), (k, 'values')
        total = np.cumsum(value, axis=1)[:, -1:]           # added in id order, one after the other
        assert np.all(total > 0) and w.tobytes() == (value / total).tobytes(), (k, 'weights')
    eps = load_golden('diffusion_reference.json')['cases'][0]['eps']
    got_ei, w, info = sparse(G, LARGE_T, eps=eps, sources=src)
    keep = x >= eps
    assert keep.sum() > P and np.array_equal(np.diff(info['ptr']), keep.sum(axis=1))
    jj, ii = np.nonzero(keep)                              # by column, then by node id
    assert np.array_equal(got_ei[0], ii) and np.array_equal(got_ei[1], np.asarray(src)[jj])
    assert info['value'].tobytes() == x[jj, ii].tobytes()
    assert w.tobytes() == np.concatenate([diffusion_ref.normalise(x[j, keep[j]]) for j in range(P)]).tobytes()


# ---- 6. the groups of a launch -------------------------------------------------------------------------------------------------------
def same_as_solo(G, order, named, y, iy, t, label):
    """The named positions of a call: the column and the deficit are those of the source solved alone."""
    for pos in named:
        s = order[pos]
        x1, i1 = solve(G, [s], t)
        assert (y[pos].tobytes(), iy['deficit'][pos].hex()) == (x1[0].tobytes(), i1['deficit'][0].hex()), (label, pos, s)
    assert iy['terms'] == i1['terms']


def test_heat_groups_limited_by_n_leave_the_columns_alone(dcr):
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
    y, iy = solve(G, order, LARGE_T)
    same_as_solo(G, order, named, y, iy, LARGE_T, 'six groups')


def test_heat_groups_2_to_7_leave_the_columns_alone(dcr):
    """long3_mid9_short63 with 8 x 16 sources: all eight groups of a launch; the plan's picks sit in groups 2, 5 and 7."""
    ei, n = {g[0]: g[1:] for g in diffusion_ref.plan_family()}['long3_mid9_short63']
    G = dcr(ei, n)
    picked, others = plan_sources(ei, n)
    assert len(picked) == 6
    P, B = scale_ref.SMALL_GROUPS_P, 16
    named = [2 * B, 2 * B + 15, 5 * B + 1, 5 * B + 8, 7 * B + 6, 7 * B + 15]
    order = others[:P]
    for pos, s in zip(named, picked):
        order[pos] = s
    assert len(set(order)) == P
    y, iy = solve(G, order, LARGE_T)
    same_as_solo(G, order, named, y, iy, LARGE_T, 'eight groups')


# ---- 7. the selection, exactly -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', HEAT_TS)
@pytest.mark.parametrize('name', list(ref.graphs()))
def test_heat_selection_is_the_lexsort_of_the_device_columns(dcr, name, t):
    ei, n = ref.graphs()[name]
    assert n % 16 != 0
    G = dcr(ei, n)
    x, sinfo = solve(G, np.arange(n), t)       # row j = column j
    order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), -x), axis=-1)
    for k in (1, 8, n - 1, n, n + 5):
        kk = min(k, n)
        got_ei, w, info = sparse(G, t, k=k)
        assert info['deficit'].tobytes() == sinfo['deficit'].tobytes()
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
        got_ei, w, info = sparse(G, t, eps=eps)
        keep = x >= eps
        assert np.array_equal(np.diff(info['ptr']), keep.sum(axis=1)), (name, eps)
        jj, ii = np.nonzero(keep)                          # by column, then by node id
        assert np.array_equal(got_ei[0], ii) and np.array_equal(got_ei[1], jj), (name, eps)
        assert info['value'].tobytes() == x[jj, ii].tobytes()
        want_w = np.concatenate([diffusion_ref.normalise(x[j, keep[j]]) for j in range(n)]) if ii.size else np.empty(0)
        assert w.tobytes() == want_w.tobytes(), (name, eps, 'weights')
        if eps == 2.0:
            assert w.size == 0 and got_ei.shape == (2, 0)
        if eps == -1.0:
            assert w.size == n * n


def test_heat_selection_of_a_subset_of_sources_in_any_order(dcr):
    ei, n = ref.graphs()['barbell20_4']
    G = dcr(ei, n)
    src = np.array([43, 0, 21, 22, 7, 7, 19, 20, 23, 24, 1, 2, 3, 4, 5, 6, 8, 9, 42])   # 19 columns, one twice
    x, _ = solve(G, src, 5.0)
    got_ei, w, info = sparse(G, 5.0, k=8, sources=src)
    assert np.array_equal(got_ei[1], np.repeat(src, 8))
    for i in range(len(src)):
        top = diffusion_ref.top_k(x[i], 8)
        assert np.array_equal(got_ei[0][8 * i:8 * i + 8], top)
        assert w[8 * i:8 * i + 8].tobytes() == diffusion_ref.normalise(x[i, top]).tobytes()


# ---- 8. cut short ------------------------------------------------------------------------------------------------------------------
def test_heat_cut_short_warns_and_stays_a_lower_bound(dcr):
    ei, n = ref.graphs()['barbell20_4']
    G = dcr(ei, n)
    src = [0, 21, 43]
    with pytest.warns(RuntimeWarning):
        x, info = G.heat(src, t=5.0, max_terms=3, return_info=True)
    assert not info['converged'].any() and info['terms'] == 3 < ref.terms(5.0, TOL)
    assert np.all(info['deficit'] > 0.5)                                       # rho_3 = 0.735 at t = 5
    accept(x, info, ref.dense(ei, n, 5.0, key='barbell20_4')[src], ref.dense_allow(n), ei, n, src, 5.0, 'three terms')
    with pytest.warns(RuntimeWarning):
        _, _, info = G.diffusion(kernel='heat', t=5.0, k=4, max_terms=3, return_info=True)
    assert info['terms'] == 3 and not info['converged'].any()


# ---- 9. interface ------------------------------------------------------------------------------------------------------------------
def test_heat_errors_empty_and_capacity(dcr):
    from dcr import _lib
    ei, n = diffusion_ref.path(8)
    G = dcr(ei, n)
    for kw in ({}, {'k': 3, 'eps': 0.1}):
        with pytest.raises(ValueError):
            G.diffusion(kernel='heat', **kw)
    for bad in (0.0, -1.0, float('nan'), 257.0):
        with pytest.raises(ValueError):
            G.heat([0], t=bad)
        with pytest.raises(ValueError):
            G.diffusion(kernel='heat', t=bad, k=2)
    for bad in ('gauss', None):
        with pytest.raises(ValueError):
            G.diffusion(k=2, kernel=bad)
    for src in ([n], [-1], [0, 8]):
        with pytest.raises(ValueError):
            G.heat(src)
        with pytest.raises(ValueError):
            G.diffusion(kernel='heat', k=2, sources=src)
    with pytest.raises(ValueError):
        G.diffusion(kernel='heat', k=0)
    for kw in ({'max_terms': 0}, {'tol': -1.0}, {'tol': float('nan')}):
        with pytest.raises(ValueError):
            G.heat([0], **kw)
        with pytest.raises(ValueError):
            G.diffusion(kernel='heat', k=2, **kw)
    x, info = G.heat([], return_info=True)
    assert x.shape == (0, n) and info['deficit'].shape == (0,) and info['converged'].shape == (0,)
    e, w, info = G.diffusion(kernel='heat', k=3, sources=[], return_info=True)
    assert e.shape == (2, 0) and w.shape == (0,) and info['ptr'].tolist() == [0]
    x, info = solve(G, [2, 7], 256.0)                                            # the largest t
    accept(x, info, ref.dense(ei, n, 256.0)[[2, 7]], ref.dense_allow(n), ei, n, [2, 7], 256.0, 'path8 at t = 256')
    # the C ABI
    lib = _lib.lib()
    i32, f64, i64 = ctypes.c_int32, ctypes.c_double, ctypes.c_int64
    src = (i32 * 2)(1, 6)
    out, res, ptr, nnz, K = (f64 * (2 * n))(), (f64 * 2)(-7.0, -7.0), (i64 * 3)(-7, -7, -7), i64(-7), i64(-7)
    row, wgt, val = (i32 * 6)(), (f64 * 6)(), (f64 * 6)()
    assert lib.dcr_heat_columns(None, src, 2, None, out, res, K) == -1
    assert lib.dcr_heat_columns(G._h, None, 2, None, out, res, K) == -1
    assert lib.dcr_heat_columns(G._h, src, 2, None, None, res, K) == -1
    assert lib.dcr_heat_columns(G._h, src, 2, None, out, None, K) == -1
    assert lib.dcr_heat_columns(G._h, src, -1, None, out, res, K) == -1
    for bad in ((0.0, TOL, 10), (257.0, TOL, 10), (float('nan'), TOL, 10), (5.0, -1.0, 10), (5.0, float('nan'), 10), (5.0, TOL, 0)):
        assert lib.dcr_heat_columns(G._h, src, 2, ctypes.byref(_lib.HeatOpts(*bad)), out, res, K) == -1, bad
    assert lib.dcr_heat_columns(G._h, src, 0, None, out, res, K) == 0 and res[0] == -7.0 and out[0] == 0.0 and K.value == -7
    assert lib.dcr_heat_columns(G._h, src, 2, None, out, res, None) == 0       # NULL options are the defaults, the terms may be NULL
    assert lib.dcr_heat_columns(G._h, src, 2, None, out, res, K) == 0 and K.value == ref.terms(5.0, TOL)
    S = ref.dense(ei, n, 5.0)
    assert 0.0 < res[0] <= TOL * np.sqrt(3.0) and abs(sum(out[:n]) - S[:, 1].sum()) <= 1e-9

    def sparsify(g=G._h, sources=src, P=2, opts=None, mode=0, k=3, eps=0.0, ptr=ptr, cap=6, row=row, wgt=wgt, val=val, res=res, nnz=nnz):
        return lib.dcr_heat_sparsify(g, sources, P, opts, mode, k, eps, ptr, cap, row, wgt, val, res, K,
                                     ctypes.byref(nnz) if nnz is not None else None)
    assert sparsify(g=None) == -1 and sparsify(ptr=None) == -1 and sparsify(res=None) == -1 and sparsify(nnz=None) == -1
    assert sparsify(row=None) == -1 and sparsify(wgt=None) == -1 and sparsify(val=None) == -1
    assert sparsify(mode=2) == -1 and sparsify(k=0) == -1 and sparsify(mode=1, eps=float('nan')) == -1 and sparsify(cap=-1) == -1
    assert sparsify(opts=ctypes.byref(_lib.HeatOpts(0.0, TOL, 10))) == -1 and sparsify(opts=ctypes.byref(_lib.HeatOpts(5.0, TOL, 0))) == -1
    assert sparsify(sources=None) == -1                                       # NULL sources stand for all nodes: P must be n
    K.value = -7
    assert sparsify(P=0) == 0 and ptr[0] == -7 and nnz.value == -7 and K.value == -7
    assert sparsify(cap=5) == -4 and nnz.value == 6                           # top-k: known before any solve
    assert sparsify(cap=0, row=None, wgt=None, val=None) == -4 and nnz.value == 6
    assert sparsify() == 0 and nnz.value == 6 and list(ptr) == [0, 3, 6] and K.value == ref.terms(5.0, TOL)
    assert list(row) == diffusion_ref.top_k(S[:, 1], 3).tolist() + diffusion_ref.top_k(S[:, 6], 3).tolist()
    assert abs(sum(wgt[:3]) - 1.0) <= 1e-15 and abs(sum(wgt[3:]) - 1.0) <= 1e-15
    # threshold: the count comes out of the solve; too small a cap returns it with the pointers, a counting call needs no arrays
    need = int((S[:, [1, 6]] >= 0.05).sum())
    assert need > 2 and np.abs(S[:, [1, 6]] - 0.05).min() > 1e-6
    assert sparsify(mode=1, eps=0.05, cap=2) == -4 and nnz.value == need and ptr[2] == need
    nnz.value = -7
    assert sparsify(mode=1, eps=0.05, cap=0, row=None, wgt=None, val=None) == -4 and nnz.value == need
    big = need + 1
    row2, wgt2, val2 = (i32 * big)(), (f64 * big)(), (f64 * big)()
    assert sparsify(mode=1, eps=0.05, cap=big, row=row2, wgt=wgt2, val=val2) == 0 and nnz.value == need
    assert list(row2[:ptr[1]]) == np.flatnonzero(S[:, 1] >= 0.05).tolist()
    allp, allnnz = (i64 * (n + 1))(), i64()
    rown, wn, vn, resn = (i32 * (2 * n))(), (f64 * (2 * n))(), (f64 * (2 * n))(), (f64 * n)()
    assert lib.dcr_heat_sparsify(G._h, None, n, None, 0, 2, 0.0, allp, 2 * n, rown, wn, vn, resn, None, ctypes.byref(allnnz)) == 0
    assert allnnz.value == 2 * n and list(allp) == list(range(0, 2 * n + 1, 2))


# ---- 10. the live graph ------------------------------------------------------------------------------------------------------------
def test_heat_live_graph_edits(dcr):
    ei, n = diffusion_ref.random_graph(300, 5)
    A = diffusion_ref.adjacency(ei, n)
    v = n - 1
    u = max(w for w in range(v) if A[v, w] == 0)
    assert u > np.flatnonzero(A[v]).max() and v > np.flatnonzero(A[u]).max()    # each end becomes the other's largest neighbour
    G = dcr(ei, n)
    before = sparse(G, 5.0, k=8)
    G.add_edge(u, v)
    a, b = 7, int(np.flatnonzero(A[7])[0])
    G.remove_edge(a, b)
    live = sparse(G, 5.0, k=8)
    fresh = sparse(dcr(G.to_edge_index(), n), 5.0, k=8)
    assert not np.array_equal(before[0], live[0])
    assert np.array_equal(live[0], fresh[0]) and live[1].tobytes() == fresh[1].tobytes()
    for key in ('value', 'deficit', 'ptr'):
        assert live[2][key].tobytes() == fresh[2][key].tobytes(), key
    src = [3, 150, 151, 7, 299, u, v]
    xl, il = solve(G, src, 5.0)
    xf, jf = solve(dcr(G.to_edge_index(), n), src, 5.0)
    assert xl.tobytes() == xf.tobytes() and il['deficit'].tobytes() == jf['deficit'].tobytes()
    # an edge appended in the middle of two rows' order: other bits, the same matrix
    G.add_edge(3, 150) if A[3, 150] == 0 else G.add_edge(3, 151)
    against_taylor(G, G.to_edge_index(), n, src, 5.0, 'after three edits')


# ---- 11. end to end ----------------------------------------------------------------------------------------------------------------
def test_heat_digl_trains_the_gcn():
    """digl(kernel='heat') feeds models/gcn.py as digl(kernel='ppr') does, and the GCN trains on it: full batch, no dropout, Adam.
    Adam's first steps have the length of the learning rate whatever the gradient, so the loss may rise from one step to the next;
    what training has to show is a finite loss at every epoch that ends below where it began."""
    import torch
    from dcr import synthetic
    from dcr.data import Data, Dataset
    from models.gcn import GCN
    from rewiring.diffusion import digl
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    g = torch.Generator(device='cuda').manual_seed(5)
    x = torch.rand(n, 96, device='cuda', generator=g)
    e = torch.from_numpy(ei).cuda()
    y = x[:, :7].clone().index_add_(0, e[0], x[e[1], :7]).argmax(dim=1)      # labels a node's neighbourhood explains
    data = Data(x=x, edge_index=torch.from_numpy(ei).cuda(), y=y, num_nodes=n)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        out = digl(data, kernel='heat', t=5.0, k=64)
        other = digl(data, kernel='heat', t=5.0, k=64, alpha=0.9)             # alpha is not used
    assert out.x is x and out.y is y and out.num_nodes == n and data.edge_attr is None
    assert out.edge_index.shape == (2, 64 * n) and out.edge_index.dtype == torch.int64 and out.edge_index.is_cuda
    assert out.edge_attr.shape == (64 * n,) and out.edge_attr.dtype == torch.float32
    assert torch.equal(out.edge_index, other.edge_index) and torch.equal(out.edge_attr, other.edge_attr)
    sums = torch.zeros(n, device='cuda', dtype=torch.float64).index_add_(0, out.edge_index[1], out.edge_attr.double())
    assert (sums - 1).abs().max().item() <= 64 * 2.0 ** -24                  # every column's weights sum to one
    ppr = digl(data, alpha=0.15, k=64)
    assert not torch.equal(out.edge_attr, ppr.edge_attr)                      # another matrix than PageRank's
    torch.manual_seed(3)
    model = GCN(Dataset(out, 7), hidden=[64], dropout=0.0).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    model.train()
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = torch.nn.functional.nll_loss(model(out), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print('  losses', ' '.join(f'{v:.4f}' for v in losses))
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0] and min(losses[10:]) < min(losses[:10]), losses


# ---- 12. PageRank untouched --------------------------------------------------------------------------------------------------------
def test_ppr_is_the_default_kernel_and_unchanged(dcr):
    ei, n = ref.graphs()['random300']
    G = dcr(ei, n)
    a = G.diffusion(alpha=0.15, k=8, return_info=True)
    b = G.diffusion(alpha=0.15, k=8, kernel='ppr', return_info=True)
    G.heat([0, 5], t=5.0)                                                     # a heat solve in between leaves nothing behind
    c = G.diffusion(alpha=0.15, k=8, kernel='ppr', t=20.0, return_info=True)  # t is not used
    for other in (b, c):
        assert a[0].tobytes() == other[0].tobytes() and a[1].tobytes() == other[1].tobytes()
        assert set(a[2]) == set(other[2]) == {'value', 'ptr', 'residual', 'steps', 'converged'}
        for key in a[2]:
            assert a[2][key].tobytes() == other[2][key].tobytes(), key
