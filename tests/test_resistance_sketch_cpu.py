"""The resistance sketch without a GPU: the numpy restatement tests/resistance_sketch_ref.py against the estimator's own
properties (b_j sums to zero on every component, a bridge is exactly 1, Foster and the relative deviation within five standard
deviations), the rounding term of the GPU tests' acceptance rule measured on the float64 CG replica, and the call surface."""
import os
import re

import numpy as np
import pytest

import resistance_ref as ref
import resistance_sketch_ref as skref
import spectral_ref
from conftest import PKG, REPO

CSRC = os.path.join(PKG, 'csrc')


def rhs_graphs():
    out = {'hub_with_tail': ref.hub_with_tail(2100), 'triangle_star_isolated': ref.triangle_star_isolated(), 'random300': ref.random_graph(300)}
    out.update({name: (ei, n) for name, ei, n in spectral_ref.plan_family()})
    return out


@pytest.mark.parametrize('name', ['hub_with_tail', 'triangle_star_isolated', 'random300'] + list(spectral_ref.PLAN_NAMES))
def test_rhs_sums_to_zero_per_component_and_stays_within_the_degree(name):
    ei, n = rhs_graphs()[name]
    _, labels = spectral_ref.components(ei, n)
    deg = np.bincount(np.asarray(ei)[0], minlength=n)
    for seed, batch in ((0, 0), (0, 7), (0x9E3779B97F4A7C15, 1)):
        b = skref.batch_rhs(ei, n, seed, batch)
        assert b.shape == (n, 16) and np.array_equal(b, np.rint(b))
        assert (np.abs(b) <= deg[:, None]).all() and ((b - deg[:, None]) % 2 == 0).all()   # deg terms of +1 or -1 each
        sums = np.zeros((n, 16))
        np.add.at(sums, labels, b)
        assert not sums.any()
    assert not np.array_equal(skref.batch_rhs(ei, n, 0, 0), skref.batch_rhs(ei, n, 0, 1)) or not deg.any()


def test_signs_are_keyed_by_the_endpoints_and_look_fair():
    e = ref.edges(ref.random_graph(300)[0])
    q = skref.signs(e, 0, 0, 256)
    assert set(np.unique(q)) == {-1.0, 1.0}
    assert abs(q.mean()) <= 5.0 / np.sqrt(q.size)                                        # 151,000 fair signs
    assert np.array_equal(skref.signs(e[::-1], 0, 0, 256), q[:, ::-1])                   # the order of the edges does not matter
    assert np.array_equal(skref.signs(e, 0, 16, 16), q[16:32]) and np.array_equal(skref.signs(e, 0, 5, 20), q[5:25])
    assert not np.array_equal(skref.signs(e, 1, 0, 16), q[:16])


@pytest.mark.parametrize('name', ['path70', 'star40'])
def test_bridges_are_exactly_one(name):
    ei, n = ref.path(70) if name == 'path70' else ref.star(40)
    for k in (1, 16, 20):
        sk = skref.Sketch(ei, n, k, seed=0)
        r = sk.edge_values()
        print(f'  {name}, k = {k}: max |R~ - 1| = {np.abs(r - 1.0).max():.3e}')
        assert np.abs(r - 1.0).max() <= 64 * n * ref.EPS                                  # B L^+ B^T is the identity on a tree


def test_foster_and_relative_deviation_on_random300():
    ei, n = ref.random_graph(300, 5)
    k = 256
    d = ref.Dense(ei, n)
    sk = skref.Sketch(ei, n, k, seed=0, dense=d)
    r_sketch, r_exact = sk.edge_values(), d.resistance(sk.edges)
    foster, rel = abs(r_sketch.sum() - (n - 1)), np.abs(r_sketch / r_exact - 1.0).max()
    print(f'  random_graph(300, 5), k = 256, seed 0: |sum R~ - (n - 1)| = {foster:.4f} (5 sigma = {5 * np.sqrt(2 * (n - 1) / k):.4f}), '
          f'max |R~ / R - 1| = {rel:.4f} (5 sigma = {5 * np.sqrt(2 / k):.4f})')
    assert foster <= 5.0 * np.sqrt(2.0 * (n - 1) / k)
    assert rel <= 5.0 * np.sqrt(2.0 / k)


def test_cg_replica_is_within_the_residual_bound_of_pinv_and_the_rounding_term_covers_the_rest():
    """The measurement behind ROUNDING_MEASURED: over the graphs and column counts of the GPU tests, at the default tolerance and
    at 1e-12 and 1e-15 (where the residual bound is small and what is left shows: rounding in the iteration and the error of pinv
    itself), the largest excess of |R~_cg - R~_pinv| over the residual bound, relative to max(1, R~_pinv)."""
    worst = 0.0
    for name, make in skref.GENERAL.items():
        ei, n = make()
        d = ref.Dense(ei, n)
        pairs = np.concatenate([ref.edges(ei), skref.pairs_of(n)])
        pairs = pairs[(pairs[:, 0] != pairs[:, 1]) & (d.labels[pairs[:, 0]] == d.labels[pairs[:, 1]])]
        for k in skref.COLUMNS:
            want = skref.Sketch(ei, n, k, seed=0, dense=d)
            a = want.diffs(pairs)
            r_ref = (a ** 2).mean(axis=0)
            for tol in (1e-6, 1e-12, 1e-15):
                got = skref.Sketch(ei, n, k, seed=0, dense=d, solver='cg', tol=tol)
                gap = np.abs(got.values(pairs) - r_ref)
                excess = ((gap - skref.residual_bound(a, got.residual, d.lambda1)) / np.maximum(1.0, r_ref)).max()
                print(f'  {name}, k = {k}, tol {tol:g}: steps {got.steps.min()} .. {got.steps.max()}, residual <= {got.residual.max():.3e}, '
                      f'max gap {gap.max():.3e}, excess over the residual bound {excess:.3e}')
                worst = max(worst, excess)
    print(f'  largest excess {worst:.3e}; recorded {skref.ROUNDING_MEASURED:.3e}')
    assert 0.0 < skref.ROUNDING_MEASURED and worst <= skref.ROUNDING_MEASURED * 1.0000001
    assert skref.ROUNDING_ALLOW == 16.0 * skref.ROUNDING_MEASURED


def pinv_error(d, sk):
    """float64 [k]: a bound on |z_j - z_j*| of Sketch(solver='pinv'), entry by entry: the residual |L z_j - b_j| over the smallest
    non-zero eigenvalue of L = D - A.  A difference of two entries is within twice that."""
    lap = np.diag(d.deg) - d.a
    lam = np.linalg.eigvalsh(lap)[d.count]
    return np.linalg.norm(sk.z @ lap - sk.b, axis=1) / lam


def test_windmill_closed_form_against_pinv():
    """Every kind of blade on both centres, 143 nodes: all edges, pairs inside a blade, across blades of one centre and across the
    bridge.  The bound is the pseudo-inverse's own (pinv_error) plus 64 roundings of the largest difference for the closed form."""
    ei, n, parts = skref.windmill(skref.WINDMILL_SMALL, seed=3)
    assert n == 143 and len(parts) == 1 + 2 * len(skref.BLADES)
    d = ref.Dense(ei, n)
    assert d.count == 1
    c0, c1 = skref.windmill_centres(parts)
    assert d.deg[c0] == 1 + 2 * sum(sum(1 for e in loc if 0 in e) for loc in skref.BLADES.values()) and d.a[c0, c1] == 1.0
    pairs = np.concatenate([ref.edges(ei), np.random.default_rng(4).integers(0, n, size=(400, 2)), [(c0, c1)]])
    for k, seed in ((20, 0), (48, 0x9E3779B97F4A7C15)):
        sk = skref.Sketch(ei, n, k, seed=seed, dense=d)
        got, want = skref.windmill_diffs(n, parts, seed, k, pairs), sk.diffs(pairs)
        tol = 2.0 * pinv_error(d, sk)[:, None] + 64 * ref.EPS * np.abs(want).max()
        print(f'  windmill of 143 nodes, k = {k}: max |a_closed - a_pinv| = {np.abs(got - want).max():.3e}, bound >= {tol.min():.3e}, '
              f'max |a| = {np.abs(want).max():.3f}')
        assert np.all(np.abs(got - want) <= tol)


def test_sparse_diffs_against_pinv_and_its_two_grounds():
    for name in ('random300', 'triangle_star_isolated', 'barbell_20_4'):
        ei, n = skref.GENERAL[name]()
        d = ref.Dense(ei, n)
        sk = skref.Sketch(ei, n, 20, seed=0, dense=d)
        pairs = np.concatenate([ref.edges(ei), skref.pairs_of(n)])
        inside = d.labels[pairs[:, 0]] == d.labels[pairs[:, 1]]
        a0, a1 = (skref.sparse_diffs(ei, n, sk.b, pairs, g) for g in ('smallest', 'largest'))
        assert np.isnan(a0[:, ~inside]).all() and np.isnan(a1[:, ~inside]).all() and np.isfinite(a0[:, inside]).all()
        want = sk.diffs(pairs)
        tol = 2.0 * pinv_error(d, sk)[:, None] + 64 * ref.EPS * np.abs(want).max()
        e_a = skref.ground_error(a0[:, inside], a1[:, inside])
        print(f'  {name}: max |a_splu - a_pinv| = {np.abs(a0 - want)[:, inside].max():.3e}, bound >= {tol.min():.3e}, e_a = {e_a:.3e}')
        assert np.all(np.abs(a0 - want)[:, inside] <= tol) and e_a <= 64 * ref.EPS * np.abs(want).max()
        assert not a0[:, pairs[:, 0] == pairs[:, 1]].any()


def test_sparse_cg_is_the_dense_iteration():
    ei, n = ref.random_graph(300)
    d, op = ref.Dense(ei, n), skref.SparseOperator(ei, n)
    assert np.abs(op.lap.toarray() - d.lap).max() <= 4 * ref.EPS and np.array_equal(op.s, d.s)
    sk = skref.Sketch(ei, n, 4, seed=0, dense=d, solver='cg', tol=1e-12)
    z, resid, steps = skref.cg_sparse(op, sk.b, tol=1e-12)
    assert np.array_equal(steps, sk.steps) and np.abs(z - sk.z).max() <= 1e-12 and np.abs(resid - sk.residual).max() <= 1e-14


def test_replica_converges_on_the_windmill_and_rounding_at_scale_is_covered():
    """The measurement behind SCALE_ROUNDING_MEASURED and E_A_MEASURED.  The windmill's normalised Laplacian has few distinct
    eigenvalues, so the replica takes 47 to 49 steps there at tol 1e-12 on 4,081 nodes."""
    import scale_ref
    worst = -np.inf
    for name in skref.LARGE_CASES:
        case = skref.large_case(name)
        got, resid, steps = case.replica()
        ceiling = 2.0 * 1e-12 * np.sqrt(2.0 * len(case.e))                  # what DcrGraph.resistance_sketch calls converged
        assert (resid <= ceiling).all() and steps.max() < 1000, (name, resid.max(), steps.max())
        r_ref = (case.a ** 2).mean(axis=0)
        gap = np.abs(got - r_ref)
        bound = case.bound(resid)
        excess = ((gap - bound) / np.maximum(1.0, r_ref)).max()
        print(f'  {name}, n = {case.n}, k = {case.k}, seed {case.seed}: steps {steps.min()} .. {steps.max()}, residual <= {resid.max():.3e}, '
              f'lam_lo = {case.lam_lo:.4e}, e_a = {case.e_a:.3e}, max gap {gap.max():.3e}, max gap / bound {(gap / bound).max():.3e}, '
              f'excess {excess:.3e}')
        worst = max(worst, excess)
        if name == 'windmill':
            assert steps.max() <= 64 and case.e_a == 0.0
        else:
            assert case.e_a <= 16.0 * skref.E_A_MEASURED[name]                  # the rule uses the e_a of this run
            assert scale_ref.SKETCH_LARGE[name][1] == case.k
    print(f'  largest excess {worst:.3e}; recorded {skref.SCALE_ROUNDING_MEASURED:.3e}')
    assert worst <= skref.SCALE_ROUNDING_MEASURED and skref.SCALE_ROUNDING_ALLOW == 16.0 * max(0.0, skref.SCALE_ROUNDING_MEASURED)


def test_rounding_term_covers_the_small_graphs_at_the_limit_tests_column_counts():
    """tests/test_resistance_sketch_limits_gpu.py runs random300 and barbell_20_4 at k = 48 and 112, tol 1e-12, under ROUNDING_ALLOW."""
    import scale_ref
    for name in ('random300', 'barbell_20_4'):
        ei, n = skref.GENERAL[name]()
        d = ref.Dense(ei, n)
        lam_lo = ref.lambda1_lower(ei, n, 0)[0]
        assert 0.0 < lam_lo <= d.lambda1 and d.lambda1 - lam_lo <= 1e-9
        pairs = np.concatenate([ref.edges(ei), skref.pairs_of(n)])
        pairs = pairs[pairs[:, 0] != pairs[:, 1]]
        for k in scale_ref.SKETCH_SMALL_COLUMNS:
            want = skref.Sketch(ei, n, k, seed=0, dense=d)
            a = want.diffs(pairs)
            r_ref = (a ** 2).mean(axis=0)
            got = skref.Sketch(ei, n, k, seed=0, dense=d, solver='cg', tol=1e-12)
            excess = ((np.abs(got.values(pairs) - r_ref) - skref.residual_bound(a, got.residual, lam_lo)) / np.maximum(1.0, r_ref)).max()
            print(f'  {name}, k = {k}, tol 1e-12: excess over the residual bound {excess:.3e}')
            assert excess <= skref.ROUNDING_MEASURED


def test_call_surface():
    from dcr import _lib
    from dcr.graph import DcrGraph
    from experiment import effective_resistance as er
    header = open(os.path.join(REPO, 'include', 'dcr.h')).read()
    bare = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    m = re.search(r'\bint\s+dcr_resistance_sketch\s*\(([^;]*)\)\s*;', bare)
    assert m, 'dcr_resistance_sketch is not declared in include/dcr.h'
    assert len(m.group(1).split(',')) == len(_lib.SIGNATURES['dcr_resistance_sketch'][1]) == 9
    m = re.search(r'\bint\s+dcr_resistance_sketch_rhs\s*\(([^;]*)\)\s*;', bare)
    assert m, 'dcr_resistance_sketch_rhs is not declared in include/dcr.h'
    assert len(m.group(1).split(',')) == len(_lib.SIGNATURES['dcr_resistance_sketch_rhs'][1]) == 4
    assert re.search(r'typedef\s+struct\s*\{\s*int32_t\s+columns\s*;\s*uint64_t\s+seed\s*;\s*double\s+tol\s*;\s*int64_t\s+max_steps\s*;\s*\}\s*'
                     r'dcr_sketch_opts', header)
    assert re.search(r'typedef\s+struct\s*\{\s*int32_t\s+columns\s*,\s*batches\s*;\s*int64_t\s+steps_total\s*;\s*double\s+residual_max\s*;\s*\}\s*'
                     r'dcr_sketch_info', header)
    assert _lib.SketchOpts._fields_ == [('columns', _lib._i32), ('seed', _lib.ctypes.c_uint64), ('tol', _lib._f64), ('max_steps', _lib._i64)]
    assert _lib.SketchInfo._fields_ == [('columns', _lib._i32), ('batches', _lib._i32), ('steps_total', _lib._i64),
                                        ('residual_max', _lib._f64)]
    assert _lib.ctypes.sizeof(_lib.SketchOpts) == 32 and _lib.ctypes.sizeof(_lib.SketchInfo) == 24
    assert callable(DcrGraph.resistance_sketch) and callable(DcrGraph.resistance_sketch_rhs)
    assert er.sketch_relative_std(256) == np.sqrt(2 / 256) and er.sketch_relative_std(1) == np.sqrt(2.0)
    with pytest.raises(ValueError):
        er.sketch_relative_std(0)
    import inspect
    for fn in (er.edge_resistances, er.resistance_curvature):
        par = inspect.signature(fn).parameters
        assert par['method'].default == 'cg' and par['columns'].default == 256 and par['seed'].default == 0
    par = inspect.signature(DcrGraph.resistance_sketch).parameters
    assert [(k, p.default) for k, p in par.items()][1:] == [('columns', 256), ('seed', 0), ('pairs', None), ('edges', True), ('tol', 1e-6),
                                                            ('max_steps', 20000), ('return_info', False)]
    assert 'out of scope here' not in er.__doc__ and "method='sketch'" in er.__doc__
    assert 'dcr_resistance_sketch' in open(os.path.join(CSRC, 'build.sh')).read().split()
    assert 'dcr_resistance_sketch' in open(os.path.join(REPO, 'tools', 'build_variant.sh')).read().split()
    source = open(os.path.join(CSRC, 'dcr_resistance_sketch.hip')).read()
    assert 'asm' not in re.sub(r'//.*', '', source)                    # plain HIP: no inline assembly
    assert 'atomicAdd' not in source                                   # no floating-point atomics: the sums have a fixed order
    for kernel in ('k_sketch_rhs', 'k_sketch_accumulate', 'k_sketch_pairs', 'struct SketchProblem', 'col_cg_solve'):
        assert kernel in source
    # every buffer of the sketch is an owning member of the analysis state, freed with it
    state = open(os.path.join(CSRC, 'dcr_analysis.h')).read()
    state = state[state.index('struct AnalysisState {'):]
    state = state[:state.index('\n};')]
    for b in ('vec', 'part', 'ctl', 'slot', 'pair', 'pair_idx'):
        assert re.search(rf'^\s*DevBuf<[^>]+>\s+skt_{b}\s*;', state, flags=re.M), b
    assert '*' not in re.sub(r'//.*', '', state)     # no raw pointer left to free by hand
