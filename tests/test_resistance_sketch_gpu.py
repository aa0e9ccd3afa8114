"""The resistance sketch on the GPU (csrc/dcr_resistance_sketch.hip) against the numpy restatement tests/resistance_sketch_ref.py
(pinned on the CPU by tests/test_resistance_sketch_cpu.py): the right-hand sides by ==, the values under the one acceptance rule

    |R~ - R~_ref| <= 1/k sum_j (2 |a_j| eps_j sqrt(R~_ref) + eps_j^2 R~_ref) + ROUNDING_ALLOW max(1, R~_ref)

with R~_ref and a_j = z_j[u] - z_j[v] from pinv with the same signs, eps_j = rho_j / sqrt(lambda_1), rho_j the true residuals the
call returns and lambda_1 from the dense restatement; ROUNDING_ALLOW is 16 x what the CPU test measures (3.84e-12).  On a bridge
a_j = +-1 and R~_ref = 1, so the rule reads |R~ - 1| <= 1/k sum_j (2 eps_j + eps_j^2) + ROUNDING_ALLOW."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

import resistance_ref as ref
import resistance_sketch_ref as skref
import spectral_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

BIG_SEED = 0x9E3779B97F4A7C15


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


@functools.lru_cache(maxsize=None)
def general(name):
    ei, n = skref.GENERAL[name]()
    return ei, n, ref.Dense(ei, n)


def sketch(G, k, **kw):
    """resistance_sketch that must converge: ((eu, ev, R), pair values or None, info)."""
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        out = G.resistance_sketch(columns=k, return_info=True, **kw)
    (eu, ev, R), info = out[0], out[-1]
    assert R.dtype == np.float64 and R.shape == eu.shape == ev.shape and info['residual'].shape == (k,)
    assert info['columns'] == k and info['batches'] == -(-k // 16) and info['converged'].all()
    assert info['residual_max'] == info['residual'].max() and np.isfinite(info['residual']).all()
    return (eu, ev, R), (out[1] if len(out) == 3 else None), info


def accept(got, a, residual, lam, label):
    """The rule of the module docstring for values ``got`` [P] against the reference differences ``a`` [k, P]."""
    want = (a ** 2).mean(axis=0)
    bound = skref.residual_bound(a, residual, lam) + skref.allow(want)
    gap = np.abs(got - want)
    print(f'  {label}: {len(got)} values, max |R~ - R~_ref| = {gap.max():.3e}, bound there {bound[gap.argmax()]:.3e}, smallest bound '
          f'{bound.min():.3e}, max gap / bound {(gap / bound).max():.3e}, residual <= {np.max(residual):.3e}')
    assert np.all(gap <= bound), (label, np.flatnonzero(gap > bound)[:5], gap.max())


def check_against_replica(G, ei, n, d, k, seed=0, pairs=None, label='', **kw):
    """Edges (in G.edges() order) and pairs of one call against pinv with the same signs; returns the call's outputs."""
    (eu, ev, R), Rp, info = sketch(G, k, seed=seed, pairs=pairs, **kw)
    geu, gev = G.edges()
    assert np.array_equal(eu, geu) and np.array_equal(ev, gev)
    want = skref.Sketch(ei, n, k, seed=seed, dense=d)
    e = np.stack([np.minimum(eu, ev), np.maximum(eu, ev)], axis=1).astype(np.int64)
    assert np.array_equal(e[np.lexsort((e[:, 1], e[:, 0]))], want.edges)
    if len(e):
        accept(R, want.diffs(e), info['residual'], d.lambda1, f'{label} k = {k}, edges')
    if pairs is not None:
        pr = np.asarray(pairs)
        same, across = pr[:, 0] == pr[:, 1], d.labels[pr[:, 0]] != d.labels[pr[:, 1]]
        assert np.all(Rp[same] == 0.0) and not np.signbit(Rp[same]).any()
        assert np.all(np.isposinf(Rp[across & ~same]))
        solved = ~same & ~across
        assert np.isfinite(Rp[solved]).all()
        if solved.any():
            accept(Rp[solved], want.diffs(pr[solved]), info['residual'], d.lambda1, f'{label} k = {k}, pairs')
    return R, Rp, info


# ---- 1. the right-hand side ----------------------------------------------------------------------------------------------------
def rhs_graph(name):
    if name in spectral_ref.PLAN_NAMES:
        return next((ei, n) for nm, ei, n in spectral_ref.plan_family() if nm == name)
    return {'hub_with_tail': lambda: ref.hub_with_tail(2100), 'triangle_star_isolated': ref.triangle_star_isolated,
            'random300': lambda: ref.random_graph(300)}[name]()


@pytest.mark.parametrize('name', ['hub_with_tail', 'triangle_star_isolated', 'random300'] + list(spectral_ref.PLAN_NAMES))
def test_rhs_equals_the_replica(dcr, name):
    ei, n = rhs_graph(name)
    G = dcr(ei, n)
    for seed, batch in ((0, 0), (0, 1), (0, 7), (BIG_SEED, 1), (0, 2 ** 32 + 3)):
        got = G.resistance_sketch_rhs(seed, batch)
        want = skref.batch_rhs(ei, n, seed, batch)
        assert got.shape == want.shape == (n, 16)
        assert np.array_equal(got, want), (name, seed, batch, np.argwhere(got != want)[:5])
    with pytest.raises(ValueError):
        G.resistance_sketch_rhs(0, -1)


# ---- 2. bridges: a closed form that needs no statistics -------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['path70', 'hub_with_tail'])
def test_bridges_are_one(dcr, name):
    ei, n = ref.path(70) if name == 'path70' else ref.hub_with_tail(2100)
    lam = ref.Dense(ei, n).lambda1
    G = dcr(ei, n)
    for k in (20, 80):
        (eu, ev, R), _, info = sketch(G, k)
        assert len(R) == n - 1
        eps = info['residual'] / np.sqrt(lam)
        bound = (2.0 * eps + eps ** 2).mean() + skref.allow(1.0)
        print(f'  {name}, k = {k}: max |R~ - 1| = {np.abs(R - 1.0).max():.3e}, bound {bound:.3e}, residual <= {info["residual"].max():.3e}, '
              f'{info["steps_total"]} steps')
        assert np.abs(R - 1.0).max() <= bound


# ---- 3. general graphs: one batch, padding columns, two batches, more than one launch of groups ----------------------------------
@pytest.mark.parametrize('k', skref.COLUMNS)
@pytest.mark.parametrize('name', list(skref.GENERAL))
def test_edges_and_pairs_against_pinv_with_the_same_signs(dcr, name, k):
    ei, n, d = general(name)
    check_against_replica(dcr(ei, n), ei, n, d, k, pairs=skref.pairs_of(n), label=name)


def test_a_tight_solve_and_another_seed(dcr):
    ei, n, d = general('random300')
    _, _, loose = check_against_replica(dcr(ei, n), ei, n, d, 20, seed=BIG_SEED, pairs=skref.pairs_of(n), label='random300, 64-bit seed,')
    _, _, tight = check_against_replica(dcr(ei, n), ei, n, d, 20, seed=BIG_SEED, pairs=skref.pairs_of(n), tol=1e-12, label='random300, tol 1e-12,')
    assert tight['residual'].max() < 1e-3 * loose['residual'].max() and tight['steps_total'] > loose['steps_total']


def test_pairs_alone_and_edges_alone(dcr):
    ei, n, d = general('barbell_20_4')
    G = dcr(ei, n)
    pairs = skref.pairs_of(n)
    (eu, ev, R), Rp, info = sketch(G, 20, pairs=pairs)
    only_pairs, info_p = G.resistance_sketch(columns=20, pairs=pairs, edges=False, return_info=True)
    eu2, ev2, only_edges = G.resistance_sketch(columns=20)
    assert only_pairs.tobytes() == Rp.tobytes() and only_edges.tobytes() == R.tobytes() and np.array_equal(eu2, eu)
    assert info_p['residual'].tobytes() == info['residual'].tobytes()
    with pytest.raises(ValueError):
        G.resistance_sketch(columns=20, edges=False)


# ---- 4. determinism, columns on their own, edits -----------------------------------------------------------------------------------
def test_same_bits_twice_and_a_column_does_not_depend_on_the_column_count(dcr):
    ei, n, d = general('random300')
    G = dcr(ei, n)
    pairs = skref.pairs_of(n)
    (_, _, R1), P1, i1 = sketch(G, 80, pairs=pairs)
    (_, _, R2), P2, i2 = sketch(G, 80, pairs=pairs)
    assert R1.tobytes() == R2.tobytes() and P1.tobytes() == P2.tobytes() and i1['residual'].tobytes() == i2['residual'].tobytes()
    assert i1['steps_total'] == i2['steps_total']
    (_, _, R16), _, i16 = sketch(G, 16)
    assert i16['residual'].tobytes() == i1['residual'][:16].tobytes()
    (_, _, R20), _, i20 = sketch(G, 20)                                 # padding beside them
    assert i20['residual'].tobytes() == i1['residual'][:20].tobytes()
    assert not np.array_equal(R16, R1[:len(R16)])
    H = dcr(ei, n)                                                       # another handle: fresh buffers
    (_, _, R3), _, i3 = sketch(H, 80)
    assert R3.tobytes() == R1.tobytes() and i3['residual'].tobytes() == i1['residual'].tobytes()


def test_live_graph_edits(dcr):
    ei, n, _ = general('random300')
    G = dcr(ei, n)
    sketch(G, 16)                                                        # the buffers exist before the edits
    e = ref.edges(ei)
    assert not G.has_edge(0, 299)
    G.add_edge(0, 299)
    if not G.has_edge(17, 250):
        G.add_edge(17, 250)
    u, v = (int(x) for x in e[len(e) // 2])
    G.remove_edge(u, v)
    now = G.to_edge_index()
    assert not np.array_equal(now, ei)
    d = ref.Dense(now, n)
    check_against_replica(G, now, n, d, 20, pairs=skref.pairs_of(n), label='after add_edge / remove_edge,')
    H = dcr(*ref._und([(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (4, 5), (3, 5)], 6))
    H.remove_edge(2, 3)                                                  # the bridge: two components
    now = H.to_edge_index()
    check_against_replica(H, now, 6, ref.Dense(now, 6), 20, pairs=np.array([(0, 5), (2, 3), (0, 1), (4, 5), (1, 1)]), label='bridge removed,')


# ---- 5. the Python surface -------------------------------------------------------------------------------------------------------
def test_resistance_curvature_with_the_sketch(dcr):
    from experiment.effective_resistance import edge_resistances, resistance_curvature, sketch_relative_std
    ei, n, d = general('barbell_20_4')
    G = dcr(ei, n)
    k = 256
    p, eu, ev, kappa = resistance_curvature(G, method='sketch', columns=k, seed=0)
    p0, eu0, ev0, kappa0 = resistance_curvature(G)
    assert np.array_equal(eu, eu0) and np.array_equal(ev, ev0) and p.shape == p0.shape == (n,) and kappa.shape == kappa0.shape
    assert p.dtype == kappa.dtype == np.float64
    foster = np.sqrt(2.0 * (n - 1) / k)
    print(f'  barbell(20, 4), k = {k}: sum p - 1 = {p.sum() - 1.0:.4f}, Foster deviation {foster:.4f}; max |R~ / R - 1| = '
          f'{np.abs(edge_resistances(G, method="sketch", columns=k)[2] / edge_resistances(G)[2] - 1).max():.4f}, '
          f'sqrt(2 / k) = {sketch_relative_std(k):.4f}')
    assert abs(p.sum() - 1.0) <= 5.0 * foster                          # sum p = n - sum R~: mean c = 1, deviation <= sqrt(2 (n - c) / k)
    eu1, ev1, R = edge_resistances(G, method='sketch', columns=k, seed=0)
    assert np.array_equal(eu1, eu) and np.array_equal(2.0 * (p[eu] + p[ev]) / R, kappa)
    with pytest.raises(ValueError):
        edge_resistances(G, method='exact')
    with pytest.raises(TypeError):
        edge_resistances(G, method='sketch', colums=3)


# ---- 6. errors and graphs without edges ----------------------------------------------------------------------------------------------
def test_errors_and_empty(dcr):
    from dcr import _lib
    ei, n = ref.path(4)
    G = dcr(ei, n)
    for bad in (dict(columns=0), dict(columns=-3), dict(tol=-1.0), dict(tol=float('nan')), dict(max_steps=0), dict(pairs=[(0, n)]),
                dict(pairs=[(-1, 2)])):
        with pytest.raises(ValueError):
            G.resistance_sketch(**bad)
    (eu, ev, R), Rp, info = sketch(G, 1, pairs=np.zeros((0, 2), dtype=np.int64))
    assert Rp.shape == (0,) and np.abs(R - 1.0).max() <= 1e-6 and info['batches'] == 1
    L = _lib.lib()
    out = (ctypes.c_double * 3)(-7.0, -7.0, -7.0)
    assert L.dcr_resistance_sketch(None, None, out, None, None, 0, None, None, None) == -1
    assert L.dcr_resistance_sketch(G._h, None, out, None, None, -1, None, None, None) == -1
    u = (ctypes.c_int32 * 1)(0)
    assert L.dcr_resistance_sketch(G._h, None, out, u, None, 1, None, None, None) == -1 and out[0] == -7.0
    assert L.dcr_resistance_sketch_rhs(G._h, 0, 0, None) == -1
    assert L.dcr_resistance_sketch(G._h, None, out, None, None, 0, None, None, None) == 0    # NULL options: 256 columns, tol 1e-6
    assert np.abs(np.array(out[:]) - 1.0).max() <= 1e-6
    E = dcr(np.zeros((2, 0), dtype=np.int64), 5)                         # no edge: every b_j is zero and no column takes a step
    (eu, ev, R), Rp, info = sketch(E, 20, pairs=[(0, 1), (3, 2), (4, 4)])
    assert R.shape == (0,) and np.isposinf(Rp[:2]).all() and Rp[2] == 0.0
    assert info['steps_total'] == 0 and not info['residual'].any()
    assert not E.resistance_sketch_rhs(0, 0).any()
    T = dcr(*ref.triangle_star_isolated())                               # an isolated node beside components with edges
    assert not T.resistance_sketch_rhs(0, 0)[8].any()


# ---- 7. the bench graph ----------------------------------------------------------------------------------------------------------------
def test_foster_on_the_bench_graph(dcr):
    import time
    from dcr import synthetic
    from experiment.effective_resistance import edge_resistances
    scale = load_golden('cheeger_bounds_reference.json')['scale']
    ei, n = synthetic.powerlaw_graph(*scale['generator']['powerlaw_graph'][:2], seed=scale['generator']['powerlaw_graph'][2])
    G = dcr(ei, n)
    c = G.connected_components()[0]
    k = 64
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        eu, ev, R = edge_resistances(G, method='sketch', columns=k, seed=0)
    dt = time.perf_counter() - t0
    deg = np.bincount(ei[0], minlength=n).astype(float)
    five = 5.0 * np.sqrt(2.0 * (n - c) / k)
    ratio = R / (0.5 * (1 / deg[eu] + 1 / deg[ev]))
    print(f'  S100k, {len(R)} edges, k = {k}: {dt * 1e3:.1f} ms (first call), sum R~ - (n - c) = {R.sum() - (n - c):.2f}, 5 sigma = {five:.2f}; '
          f'R~ / (1/2 (1/d_u + 1/d_v)) in {ratio.min():.3f} .. {ratio.max():.3f}')
    assert len(R) == G.number_of_edges() and np.isfinite(R).all() and (R > 0).all()
    assert abs(R.sum() - (n - c)) <= five
