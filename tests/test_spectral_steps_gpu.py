"""The Lanczos solver of csrc/dcr_spectral.hip, step by step, against the host replica tests/spectral_lanczos_ref.py.

At ``tol = 0`` nothing converges and the driver's control flow is fixed by the graph and the seed (the replica's docstring says
how): with ``max_steps = s + 1`` it runs s Lanczos steps from the Philox start vector, is forced to restart from the top Ritz vector
of T_s (k_spec_combine, then the deflation and normalisation of a first column), runs one more step and returns that vector, its
Rayleigh quotient and its true residual.  In exact arithmetic the three are functions of the graph and the seed, whatever the order
of the orthogonalisation, and the replica states them in np.longdouble.  A Gram-Schmidt coefficient that loses the tail of a slab,
a partial closed wrongly, a deflation dot over the wrong chunks or a combination over the wrong columns moves them by far more than
rounding, where a full solve (tests/test_cheeger_bounds_gpu.py) would only take more steps to the same eigenvalue.

The allowance rule.  ref.counted is a counted first-order rounding bound for lambda1 and the residual (the inner products of length
n, the Gram-Schmidt updates against at most s columns twice a step, the longest row's accumulation, |B| <= 2); for the vector it is
divided by the gap of the two largest Ritz values of the last T_k, which tests/test_spectral_steps_cpu.py holds above 2^-8 on the
replica for every case here (the smallest is 1.478e-02).  The device gets 16 times the larger of that bound and the distance
between the replica's float64 and longdouble runs, measured on the CPU on every case (ref.allow): the device is a float64
evaluation in another summation order, under the same error law.  Nothing in it is tuned against the device.  The largest CPU
distances over the cases (test_spectral_steps_cpu.py prints them all): lambda1 7.203e-16, residual 6.373e-16, vector 2.281e-15;
on every case the counted bound is the larger of the two.

Run the file under a time limit (``timeout 300 pytest -m gpu ...``): no test loops around a failing step."""
import numpy as np
import pytest

import spectral_lanczos_ref as ref
import spectral_ref
from test_cheeger_bounds_gpu import check_against, solve

pytestmark = pytest.mark.gpu

L = np.longdouble
_GRAPHS = {}


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


def device_graph(dcr, key):
    if key not in _GRAPHS:
        ei, n = ref.graph(key)
        _GRAPHS[key] = dcr(ei, n)
    return _GRAPHS[key]


def run(dcr, case):
    key, ms, mb = case
    with pytest.warns(RuntimeWarning):
        return device_graph(dcr, key).spectral_gap(tol=0.0, max_steps=ms, max_basis=mb, seed=ref.SEED, return_vector=True)


# ---- 1. every case, step by step -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ref.CASES, ids=ref.case_id)
def test_steps_against_the_replica(dcr, case):
    """One component at the slab, block and chunk tails of k_spec_gs_coef and the deflation (n = 511 .. 2049); components of 1024,
    1025 and 2049 nodes through order[] with ch.z != 0 and ch.w in (2, 3); 65 waves' partials, past one trip of the closing lanes;
    every class of row in the mat-vec (alpha_0 and beta_0 at max_steps = 1 are its values); chained restarts over a full basis of 4
    and of 16 columns; the basis capped by the dimension."""
    key, ms, mb = case
    ei, n = ref.graph(key)
    want = ref.reference(case)
    lam, res, y, steps, restarts = want['long']
    r = run(dcr, case)
    allow_value = ref.allow(want['counted'], max(want['dist'][:2]))
    allow_vector = ref.allow(want['counted_vector'], want['dist'][2])
    d_lam, d_res = abs(float(L(r.lambda1) - lam)), abs(float(L(r.residual) - res))
    d_vec = ref.vector_distance(r.vector, y, signed=ms > 1)
    K = spectral_ref.null_vectors(ei, n)
    defl, unit = float(np.abs(K @ r.vector).max()), abs(float(np.linalg.norm(r.vector)) - 1)
    print(f'{ref.case_id(case)}: steps {r.steps} ({steps}) restarts {r.restarts} ({restarts}) lambda1 {r.lambda1!r} residual {r.residual!r}')
    print(f'    |d lambda1| {d_lam:.3e} |d residual| {d_res:.3e} (allowed {allow_value:.3e}); |d vector| {d_vec:.3e} '
          f'(allowed {allow_vector:.3e}); |K y| {defl:.3e} ||y| - 1| {unit:.3e}')
    assert (r.steps, r.restarts, r.converged) == (steps, restarts, False)
    assert r.components == spectral_ref.components(ei, n)[0]
    assert d_lam <= allow_value
    assert d_res <= allow_value
    assert d_vec <= allow_vector
    assert defl <= 1e-12 and unit <= 1e-12
    deg = np.bincount(ei[0], minlength=n)
    assert (r.vector[deg == 0] == 0.0).all()


def test_by_component_path_same_bits(dcr):
    """The ticket and the partials are reused between the mat-vec, the deflation and the Gram-Schmidt launches; the graph of several
    multi-chunk components is the one that takes them through order[]."""
    for ms in (9, 25):
        a, b = run(dcr, ('multi', ms, None)), run(dcr, ('multi', ms, None))
        assert a.lambda1.hex() == b.lambda1.hex() and a.residual.hex() == b.residual.hex()
        assert (a.steps, a.restarts) == (b.steps, b.restarts)
        assert a.vector.tobytes() == b.vector.tobytes()


# ---- 2. full solves ----------------------------------------------------------------------------------------------------------------------
def test_full_solve_of_the_multi_chunk_components(dcr):
    """The default tolerance on the graph of 1024-, 1025- and 2049-node components: lambda1 is the smallest of the components' own
    (dense, per component), and the residual the solver reports is the vector's true one."""
    ei, n = ref.graph('multi')
    R = ref.operators('multi')['long']
    r = solve(device_graph(dcr, 'multi'), n, seed=ref.SEED, return_vector=True)
    assert r.components == R.components == 7
    per_component = []
    for root in R.roots:
        ids = np.flatnonzero(R.labels == root)
        local = np.full(n, -1, dtype=np.int64)
        local[ids] = np.arange(ids.size)
        inside = R.labels[ei[0]] == root
        per_component.append(spectral_ref.lambda1(local[ei[:, inside]], ids.size))
    print('  per component:', per_component)
    assert per_component[3] == 2.0      # the two-node component
    check_against(r, min(per_component), n, 'multi-chunk components')
    y = r.vector.astype(L)
    host = (L(2) - L(r.lambda1)) * y - R.apply_B(y)       # L y - lambda1 y: L = 2 - B where y is not zero
    host = float(np.sqrt(host @ host))
    defl = float(np.abs(spectral_ref.null_vectors(ei, n) @ r.vector).max())
    # the reported residual is |P(B y) - alpha y| of one closing step against one column; the host's has no P: they differ by at
    # most |K (B y)| = 2 |K y| <= 2e-12 (asserted), and by the roundings of that one step
    allowance = ref.allow(ref.counted(n, int(R.deg.max()), 1, 1), 0.0) + 2e-12
    print(f'  host residual {host:.6e}, reported {r.residual:.6e}, allowed difference {allowance:.3e}; |K y| {defl:.3e}')
    assert defl <= 1e-12 and abs(float(np.linalg.norm(r.vector)) - 1) <= 1e-12
    assert abs(host - r.residual) <= allowance
    assert (r.vector[R.deg == 0] == 0.0).all()


def test_breakdown_with_several_components(dcr):
    """complete(5) u complete(7) u an isolated node, ids interleaved: P B P has the two eigenvalues 3/4 and 5/6 on the deflated space,
    so beta_1 is zero and the driver solves T_2 and finishes: two steps and the closing one.  (When the host first looked at the
    coefficients again after step 8 of a cycle this took 9 steps, six of them on zero columns; it now also looks after steps 2
    and 4.)"""
    ei, n = ref.graph('k5_k7_iso')
    assert n == 13 and spectral_ref.components(ei, n)[0] == 3
    r = solve(dcr(ei, n), n, seed=ref.SEED)
    assert r.components == 3
    check_against(r, 7 / 6, n, 'K5 u K7 u K1')
    assert r.steps <= 4
