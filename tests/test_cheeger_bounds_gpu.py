"""Spectral gap and Cheeger bounds on the GPU (csrc/dcr_spectral.hip) against closed forms, the reference's recorded output
(tests/golden/cheeger_bounds_reference.json) and the dense restatement tests/spectral_ref.py.

The one bound used throughout: |lambda_1 - eigenvalue| <= residual + 8 n 2^-52.  A Ritz value lies within its residual norm of an
eigenvalue (the residual is the TRUE one, recomputed by the solver with a mat-vec of its own, and at most tol when ``converged``);
the second term is the backward error of the dense eigh the value is compared with.  Every graph here has its lambda_1 separated
from the next distinct eigenvalue by far more than that.  Run the file under a time limit (``timeout 300 pytest -m gpu ...``): no
test loops around a failing step."""
import ctypes
import warnings

import numpy as np
import pytest

import spectral_ref
from conftest import load_golden
from test_cheeger_bounds_cpu import case_graph, fh

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


def solve(G, n, **kw):
    """spectral_gap that must converge; returns the SpectralGap."""
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        r = G.spectral_gap(**kw)
    tol = kw.get('tol', TOL)
    print(f'  lambda1={r.lambda1!r} residual={r.residual:.3e} steps={r.steps} restarts={r.restarts} components={r.components}')
    assert r.converged and 0 <= r.residual <= tol, r
    return r


def check_against(r, want, n, label):
    err = abs(r.lambda1 - want)
    print(f'  {label}: |lambda1 - want| = {err:.3e}, bound {spectral_ref.bound(r.residual, n):.3e}')
    assert err <= spectral_ref.bound(r.residual, n), (label, r.lambda1, want)


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c[0] for c in spectral_ref.closed_forms()] + ['grid60x60'])
def test_closed_forms(dcr, name):
    """Degenerate gaps (cycle, K_n, hypercube, grid) and the graphs on which Lanczos breaks down after one or two steps (K_n, star,
    two nodes).  The 60 x 60 grid: the normalised Laplacian of a grid has no closed form (the degrees differ), so it is compared
    with the dense value."""
    from dcr import synthetic
    if name == 'grid60x60':
        ei, n = synthetic.grid_graph(60, 60)
        want = spectral_ref.lambda1(ei, n)
    else:
        (ei, n), want = {c[0]: c[1:] for c in spectral_ref.closed_forms()}[name]
    r = solve(dcr(ei, n), n)
    assert r.components == 1
    check_against(r, want, n, name)


# ---- 2. the fixture ----------------------------------------------------------------------------------------------------------
def test_fixture_graphs(dcr):
    import torch
    from dcr.data import Data
    from experiment.cheeger_bounds import cheeger_bounds, cheeger_bounds_values
    seen = {True: 0, False: 0}
    for case in load_golden('cheeger_bounds_reference.json')['graphs']:
        ei, n = case_graph(case)
        c = case['components']
        want = fh(case['eigenvalues'][c])
        print(case['name'])
        G = dcr(ei, n)
        r = solve(G, n)
        assert r.components == c, case['name']
        check_against(r, want, n, case['name'])
        data = Data(edge_index=torch.from_numpy(ei), num_nodes=n)
        left, right, lam = cheeger_bounds_values(G)
        assert lam == r.lambda1 and left == lam / 2 and right == np.sqrt(2 * lam)
        strings = cheeger_bounds(data)
        assert strings == spectral_ref.bounds_strings(want), case['name']
        if case['reference_sound']:
            assert list(strings) == case['reference'], case['name']
        else:   # the documented deviation: the reference took rounding noise, here it is the (c+1)-th eigenvalue
            assert fh(case['reference_lambda1']) < 1e-12 and list(strings) != case['reference'], case['name']
        seen[case['reference_sound']] += 1
    assert seen[True] >= 3 and seen[False] >= 2


# ---- 3. components and deflation -----------------------------------------------------------------------------------------------
def union_graph():
    """powerlaw_graph(300, 2) ∪ a 5 x 5 grid ∪ three isolated nodes, node ids shuffled by a fixed permutation."""
    from dcr import synthetic
    a, na = synthetic.powerlaw_graph(300, 2)
    b, nb = synthetic.grid_graph(5, 5)
    n = na + nb + 3
    perm = np.random.Generator(np.random.PCG64(2024)).permutation(n)
    src = np.concatenate([a[0], b[0] + na])
    dst = np.concatenate([a[1], b[1] + na])
    return synthetic.coalesced_edge_index(perm[src], perm[dst], n), n


def test_components_and_deflation(dcr):
    ei, n = union_graph()
    G = dcr(ei, n)
    count, labels = G.connected_components()
    want_count, want_labels = spectral_ref.components(ei, n)
    assert labels.dtype == np.int32 and count == want_count == 5
    assert np.array_equal(labels, want_labels)
    for root in np.unique(labels):
        assert root == np.flatnonzero(labels == root).min()
    r = solve(G, n, return_vector=True)
    assert r.components == 5
    check_against(r, spectral_ref.lambda1(ei, n), n, 'union')
    K = spectral_ref.null_vectors(ei, n)
    print('  max |k_C . y| =', np.abs(K @ r.vector).max(), ' | |y| - 1 | =', abs(np.linalg.norm(r.vector) - 1))
    assert np.abs(K @ r.vector).max() <= 1e-12
    assert abs(np.linalg.norm(r.vector) - 1) <= 1e-12


# ---- 4. live graph -------------------------------------------------------------------------------------------------------------
def check_live(G, label):
    ei, n = G.to_edge_index(), G.number_of_nodes()
    count, labels = G.connected_components()
    want_count, want_labels = spectral_ref.components(ei, n)
    assert count == want_count and np.array_equal(labels, want_labels), label
    r = solve(G, n)
    assert r.components == want_count, label
    check_against(r, spectral_ref.lambda1(ei, n), n, label)
    return r


def test_live_graph_bridge_and_join(dcr):
    """Two power-law graphs and one bridge between them.  Removing the bridge raises c by one; an edge between the halves joins
    them again; forty appends at one node outgrow its row's slack (the rows are laid out again)."""
    from dcr import synthetic
    a, na = synthetic.powerlaw_graph(300, 2, seed=1)
    b, nb = synthetic.powerlaw_graph(200, 3, seed=2)
    n = na + nb
    ei = synthetic.coalesced_edge_index(np.concatenate([a[0], b[0] + na, [5]]), np.concatenate([a[1], b[1] + na, [na + 7]]), n)
    G = dcr(ei, n)
    r0 = check_live(G, 'bridged')
    assert r0.components == 1
    G.remove_edge(5, na + 7)
    r1 = check_live(G, 'bridge removed')
    assert r1.components == 2 and r1.lambda1 > r0.lambda1   # the bottleneck is gone: each half is an expander
    G.add_edge(na + 100, 17)
    r2 = check_live(G, 'joined again')
    assert r2.components == 1
    rng = np.random.Generator(np.random.PCG64(6))
    for _ in range(40):
        v = int(rng.integers(1, n))
        if not G.has_edge(0, v):
            G.add_edge(0, v)
    eu, ev = G.edges()
    for k in range(0, 60, 3):
        G.remove_edge(int(eu[k]), int(ev[k]))
    check_live(G, 'after appends and removals')


def test_live_graph_after_sdrf_at_coras_shape():
    import torch
    from dcr import synthetic
    from dcr.data import Data
    from rewiring.sdrf_no_cuda import SdrfRun
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    np.random.seed(0)
    run = SdrfRun(Data(edge_index=torch.from_numpy(ei), num_nodes=n), 'bfc', True, 0.5, 50)
    before = solve(run.G, n)
    for i in range(40):
        assert run.step(more=i + 1 < 40)
    assert not np.array_equal(run.G.to_edge_index(), ei)
    after = check_live(run.G, 'after 40 SDRF iterations')
    print('  gap before', before.lambda1, 'after', after.lambda1)


# ---- 5. / 6. scale and determinism ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def s100k_runs(dcr):
    from dcr import synthetic
    scale = load_golden('cheeger_bounds_reference.json')['scale']
    ei, n = synthetic.powerlaw_graph(*scale['generator']['powerlaw_graph'][:2], seed=scale['generator']['powerlaw_graph'][2])
    G = dcr(ei, n)
    return scale, ei, n, [solve(G, n, seed=0, return_vector=True), solve(G, n, seed=0, return_vector=True),
                          solve(G, n, seed=7, return_vector=True)]


def test_scale_s100k(s100k_runs):
    scale, ei, n, runs = s100k_runs
    r = runs[0]
    assert r.components == scale['components'] == 1
    check_against(r, fh(scale['lambda1']), n, 'S100k against eigsh')
    L = spectral_ref.laplacian(ei, n)
    res = np.linalg.norm(L @ r.vector - r.lambda1 * r.vector)
    print('  host residual |L y - lambda y| =', res, ' |y| - 1 =', np.linalg.norm(r.vector) - 1)
    assert res <= 2 * TOL
    assert abs(np.linalg.norm(r.vector) - 1) <= 1e-12


def test_same_seed_same_bits(s100k_runs):
    scale, ei, n, (a, b, c) = s100k_runs
    assert a.lambda1.hex() == b.lambda1.hex() and a.residual.hex() == b.residual.hex()
    assert (a.steps, a.restarts) == (b.steps, b.restarts)
    assert a.vector.tobytes() == b.vector.tobytes()
    check_against(c, fh(scale['lambda1']), n, 'S100k, another seed')
    assert c.vector.tobytes() != a.vector.tobytes()


# ---- 7. exhaustion and errors --------------------------------------------------------------------------------------------------
def test_exhaustion_warns_and_stays_above(dcr):
    from dcr import synthetic
    ei, n = synthetic.grid_graph(60, 60)
    G = dcr(ei, n)
    with pytest.warns(RuntimeWarning):
        r = G.spectral_gap(max_steps=5)
    true = spectral_ref.lambda1(ei, n)
    print(f'  after {r.steps} steps: lambda1={r.lambda1} residual={r.residual} true={true}')
    assert not r.converged and r.steps <= 5 and np.isfinite(r.lambda1) and np.isfinite(r.residual)
    assert r.lambda1 >= true   # a Rayleigh quotient of B on the deflated space never exceeds theta_max


def test_small_basis_restarts(dcr):
    """A 16-column basis on the 20 x 20 grid: several explicit restarts, the same eigenvalue."""
    from dcr import synthetic
    ei, n = synthetic.grid_graph(20, 20)
    r = solve(dcr(ei, n), n, max_basis=16)
    assert r.restarts >= 2
    check_against(r, spectral_ref.lambda1(ei, n), n, 'grid20x20, 16 columns')


def test_errors(dcr):
    from dcr import _lib
    G = dcr(np.zeros((2, 0), dtype=np.int64), 5)
    assert G.connected_components()[0] == 5
    with pytest.raises(ValueError, match='no positive eigenvalue'):
        G.spectral_gap()
    from experiment.cheeger_bounds import cheeger_bounds
    with pytest.raises(ValueError):
        cheeger_bounds(G)
    H = dcr(np.array([[0, 1], [1, 0]]), 2)
    L = _lib.lib()
    res = _lib.SpectralResult()
    assert L.dcr_spectral_gap(H._h, None, None, None) == -1
    assert L.dcr_spectral_gap(None, None, ctypes.byref(res), None) == -1
    assert L.dcr_connected_components(H._h, None, None) == -1
    with pytest.raises(ValueError):
        H.spectral_gap(tol=-1.0)
    with pytest.raises(ValueError):
        H.spectral_gap(max_steps=0)
    r = H.spectral_gap()   # NULL options are the defaults
    assert L.dcr_spectral_gap(H._h, None, ctypes.byref(res), None) == 0
    assert res.lambda1 == r.lambda1 and res.converged == 1
