"""The host restatement tests/resistance_ref.py against closed forms and the identities effective resistances obey.  No GPU: this
pins the yardstick of tests/test_resistance_gpu.py, not the kernels.  The numpy CG is held to the same acceptance rule as the device."""
import numpy as np
import pytest

import resistance_ref as ref

GRAPHS = {
    'path8': lambda: ref.path(8),
    'cycle7': lambda: ref.cycle(7),
    'complete5': lambda: ref.complete(5),
    'star6': lambda: ref.star(6),
    'barbell20_4': lambda: ref.barbell(20, 4),
    'random300': lambda: ref.random_graph(),
    'triangle_star_isolated': ref.triangle_star_isolated,
    'hub_with_tail40': lambda: ref.hub_with_tail(40),
}


@pytest.fixture(scope='module')
def dense():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ref.Dense(*GRAPHS[name]())
        return cache[name]
    return get


def all_pairs(n):
    return np.array([(i, j) for i in range(n) for j in range(n)])


def close(got, want, n):
    return np.all(np.abs(got - want) <= ref.allow(n, want))


def test_path(dense):
    d = dense('path8')
    pr = all_pairs(8)
    assert close(d.resistance(pr), np.abs(pr[:, 0] - pr[:, 1]).astype(float), 8)


def test_cycle(dense):
    d = dense('cycle7')
    pr = all_pairs(7)
    k = np.abs(pr[:, 0] - pr[:, 1])
    assert close(d.resistance(pr), k * (7 - k) / 7, 7)


def test_complete(dense):
    d = dense('complete5')
    pr = all_pairs(5)
    assert close(d.resistance(pr), np.where(pr[:, 0] == pr[:, 1], 0.0, 2 / 5), 5)
    assert d.lambda1 == pytest.approx(5 / 4, abs=1e-14)


def test_star(dense):
    d = dense('star6')
    pr = all_pairs(6)
    want = np.where(pr[:, 0] == pr[:, 1], 0.0, np.where((pr[:, 0] == 0) | (pr[:, 1] == 0), 1.0, 2.0))
    assert close(d.resistance(pr), want, 6)


def test_components_and_host_cases(dense):
    d = dense('triangle_star_isolated')
    assert d.count == 3 and d.labels.tolist() == [0, 0, 0, 3, 3, 3, 3, 3, 8]
    r = d.resistance([(0, 0), (0, 3), (4, 8), (8, 8), (1, 2), (4, 5)])
    assert r[0] == 0.0 and r[3] == 0.0 and np.isinf(r[1]) and np.isinf(r[2])
    assert close(r[4:], np.array([2 / 3, 2.0]), 9)
    assert d.cg(4, 8) == (float('inf'), 0.0, 0) and d.cg(2, 2) == (0.0, 0.0, 0)


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_foster_curvature_lovasz(dense, name):
    d = dense(name)
    n = d.n
    e = ref.edges(np.stack(np.nonzero(d.a)))
    r = d.resistance(e)
    assert abs(r.sum() - (n - d.count)) <= len(e) * ref.allow(n, 1.0)            # Foster
    p, e2, kappa = d.curvature()
    assert np.array_equal(e, e2) and abs(p.sum() - d.count) <= len(e) * ref.allow(n, 1.0)
    assert np.all(p[d.deg == 0] == 1.0) and np.all(np.isfinite(kappa))
    pr = all_pairs(n) if n <= 50 else np.random.default_rng(1).integers(0, n, size=(2000, 2))
    pr = pr[(pr[:, 0] != pr[:, 1]) & (d.labels[pr[:, 0]] == d.labels[pr[:, 1]])]
    rp = d.resistance(pr)
    inv = 1 / d.deg[pr[:, 0]] + 1 / d.deg[pr[:, 1]]
    assert np.all(0.5 * inv <= rp + ref.allow(n, rp))                             # Lovász, both sides
    assert np.all(rp <= inv / d.lambda1 + ref.allow(n, rp))


@pytest.mark.parametrize('name,most', [('barbell20_4', 8), ('path8', 7), ('random300', 38)])
def test_numpy_cg_meets_the_acceptance_rule(dense, name, most):
    d = dense(name)
    n = d.n
    e = ref.edges(np.stack(np.nonzero(d.a)))
    pairs = np.concatenate([e, [(0, n - 1), (1, n - 2)]])
    want = d.resistance(pairs)
    worst = 0
    for (u, v), r_ref in zip(pairs, want):
        lower, res, steps = d.cg(int(u), int(v))
        a = ref.allow(n, r_ref)
        assert res <= 1e-10 * np.sqrt(1 / d.deg[u] + 1 / d.deg[v]) * (1 + 1e-3)
        assert lower - a <= r_ref <= lower + res ** 2 / d.lambda1 + a, (u, v, lower, r_ref)
        worst = max(worst, steps)
    assert worst <= most


def test_cut_short_is_still_a_lower_bound(dense):
    d = dense('barbell20_4')
    for u, v in [(0, 43), (3, 30), (19, 24)]:
        r_ref = float(d.resistance([(u, v)])[0])
        lower, res, steps = d.cg(u, v, max_steps=2)
        a = ref.allow(d.n, r_ref)
        assert steps == 2 and res > 1e-10
        assert lower <= r_ref + a and r_ref <= lower + res ** 2 / d.lambda1 + a


def test_hub_with_tail_closed_forms():
    ei, n = ref.hub_with_tail(40)
    d = ref.Dense(ei, n)
    assert close(d.resistance([(2, 3), (0, 7), (5, n - 1), (1, n - 1)]), np.array([2.0, 1.0, 5.0, 3.0]), n)


# ---- the sparse reference of the 33,133-node test ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(GRAPHS))
@pytest.mark.parametrize('ground', ['smallest', 'largest'])
def test_sparse_resistance_is_pinv(dense, name, ground):
    d = dense(name)
    n = d.n
    pr = all_pairs(n) if n <= 50 else np.random.default_rng(2).integers(0, n, size=(500, 2))
    ei = np.stack(np.nonzero(d.a))
    want = d.resistance(pr)
    got = ref.sparse_resistance(ei, n, pr, ground=ground)
    fin = np.isfinite(want)
    assert np.array_equal(np.isposinf(got), ~fin) and np.all(got[pr[:, 0] == pr[:, 1]] == 0.0)
    assert close(got[fin], want[fin], n)
    if name == 'triangle_star_isolated':
        assert np.isposinf(got[~fin]).all() and (~fin).sum() == 2 * (3 * 5 + 3 + 5)


def test_sparse_reference_at_33133_nodes():
    """What tests/test_resistance_gpu.py holds the device to at 33,133 nodes, measured against itself: e_ref, the largest
    disagreement of two groundings (at node 0 and at hub4, the last connected node) over the test's 17 solved pairs, and lam_lo.
    Measured here: e_ref = 2.2e-16 (allow = 4.7e-10), lambda_1 >= 9.4189e-3 with a Ritz residual of 5e-16."""
    import scale_ref as sc
    ei, n, names = sc.diffusion_large()
    pairs, solved, _ = sc.resistance_pairs()
    first = ref.sparse_resistance(ei, n, pairs)
    second = ref.sparse_resistance(ei, n, pairs, ground='largest')
    assert np.isposinf(first[5]) and np.isposinf(second[5]) and first[6] == 0.0 and second[6] == 0.0
    assert np.isfinite(first[solved]).all()
    e_ref = np.abs(first[solved] - second[solved]).max()
    lam_lo, theta, ritz = ref.lambda1_lower(ei, n, 0)
    print(f'  e_ref = {e_ref:.3e}, allow = {ref.allow(n, 1.0):.3e}; lambda_1 >= {lam_lo:.6e} (theta {theta:.6e}, Ritz residual {ritz:.3e})')
    print('  R_ref =', np.array2string(first, precision=6))
    # two exact solutions of the same system agree to the rounding of the arithmetic, which is what allow() stands for
    assert e_ref <= ref.allow(n, 1.0)
    deg = sc.degrees(ei, n).astype(float)
    inv = 1 / deg[pairs[solved, 0]] + 1 / deg[pairs[solved, 1]]
    assert np.all(0.5 * inv <= first[solved]) and np.all(first[solved] <= inv / lam_lo)          # Lovász, with the certified gap
    assert np.all(first[[3, 7, 8]] < 1.0)                                                        # an edge that lies on a cycle
    assert 0.0 < lam_lo <= theta and ritz <= 64 * n * ref.EPS
