"""All three row classes of the analysis kernels in one launch, and the class limits themselves: spectral_ref.row_classes_graph has
rows of degree 32 | 33 and 2,048 | 2,049 next to short ones, a second component and an isolated node.  Nothing new is accepted
here: the sweep is compared bit for bit (tests/sweep_ref.py), the gap and the resistances under the rules of
test_cheeger_bounds_gpu.py and test_resistance_gpu.py against the dense restatements.

That graph pins the DEGREES at the limits and the counts of rows per class at one point.  The second half of the file runs the same
three rules over spectral_ref.plan_family, whose COUNTS sit at and either side of every boundary of csrc/dcr_analysis.h::walk_rows
and row_grid (tests/test_row_classes_cpu.py asserts which), and over one handle whose rows cross both limits by edits.  Run the
file under a time limit (``timeout 300 pytest -m gpu ...``): no test loops around a failing step."""
import numpy as np
import pytest

import resistance_ref
import spectral_ref
import sweep_ref
from test_cheeger_bounds_gpu import TOL as GAP_TOL, check_against, solve as solve_gap
from test_resistance_gpu import accept, solve as solve_pairs
from test_sweep_gpu import DEFINITIONS, assert_same

pytestmark = pytest.mark.gpu

HUBS, LEAF0, TRIANGLE, ISOLATED = (0, 1, 2, 3), 4, (2053, 2054, 2055), 2056


@pytest.fixture(scope='module')
def graph():
    from dcr.graph import DcrGraph
    ei, n = spectral_ref.row_classes_graph()
    G = DcrGraph(ei, n)
    assert n == 2057 and G.number_of_edges() == 32 + 33 + 2048 + 2049 + 3
    assert [G.degree(h) for h in HUBS] == [32, 33, 2048, 2049] and G.degree(ISOLATED) == 0
    leaf_deg = [G.degree(v) for v in range(LEAF0, TRIANGLE[0])]
    assert min(leaf_deg) == 1 and max(leaf_deg) == 4
    return ei, n, G


@pytest.mark.parametrize('definition', DEFINITIONS)
def test_sweep_bit_exact(graph, definition):
    ei, n, G = graph
    rng = np.random.Generator(np.random.PCG64(2057))
    for name, score in (('normal', rng.standard_normal(n)), ('ties', rng.integers(0, 5, n).astype(np.float64))):
        got = G.sweep_cut(score, definition=definition, return_profile=True)
        assert_same(got, sweep_ref.sweep(ei, n, score, definition), name)


def test_spectral_gap(graph):
    ei, n, G = graph
    r = solve_gap(G, n)
    assert r.components == 3
    check_against(r, spectral_ref.lambda1(ei, n), n, 'row classes')


def test_effective_resistance_two_batches(graph):
    from dcr.graph import RESISTANCE_BATCH as B
    ei, n, G = graph
    d = resistance_ref.Dense(ei, n)
    last = TRIANGLE[0] - 1   # the leaf of degree 1
    pairs = np.array([(0, 1), (0, 3), (2, 3), (1, 2), (0, 2),                    # hub - hub
                      (0, 4), (3, last), (2, 40), (1, last), (3, 4), (2, last),   # hub - leaf
                      (4, 5), (4, last), (36, last - 1), (100, 200), (35, 36), (5, 2000), (37, 38),   # leaf - leaf
                      (TRIANGLE[0], TRIANGLE[2]),
                      (10, TRIANGLE[1])])                                         # no path: decided from the components
    assert B < len(pairs) - 1 < 2 * B   # two batches, the second padded
    lower, info = solve_pairs(G, pairs)
    assert np.isposinf(lower[-1]) and info['steps'][-1] == 0 and info['residual'][-1] == 0.0
    want = d.resistance(pairs[:-1])
    assert np.isfinite(want).all()
    accept(lower[:-1], info['residual'][:-1], want, d.lambda1, n, 'row classes')
    print('  steps', info['steps'])


# ---- the plan family: the counts of rows per class at every boundary of the walker -----------------------------------------------------
BIG = 'long3_mid9_short63'


@pytest.fixture(scope='module')
def family():
    """family(name) -> (edge_index, n, handle, Dense, lambda_1).  A graph's handle and dense references are made on first use and
    live as long as this module's tests; every test below only reads them (no test edits a family handle)."""
    from dcr.graph import DcrGraph
    graphs = {name: (ei, n) for name, ei, n in spectral_ref.plan_family()}
    made = {}

    def get(name):
        if name not in made:
            ei, n = graphs[name]
            made[name] = (ei, n, DcrGraph(ei, n), resistance_ref.Dense(ei, n), spectral_ref.lambda1(ei, n))
        return made[name]
    return get


def check_sweeps(G, ei, n, label):
    rng = np.random.Generator(np.random.PCG64(n))
    for name, score in (('normal', rng.standard_normal(n)), ('ties', rng.integers(0, 5, n).astype(np.float64))):
        for definition in DEFINITIONS:
            got = G.sweep_cut(score, definition=definition, return_profile=True)
            assert_same(got, sweep_ref.sweep(ei, n, score, definition), (label, name, definition))


def check_gap(G, ei, n, want, label):
    r = solve_gap(G, n, return_vector=True)
    assert r.components == spectral_ref.components(ei, n)[0], label
    check_against(r, want, n, label)
    res = np.linalg.norm(spectral_ref.laplacian(ei, n) @ r.vector - r.lambda1 * r.vector)
    print(f'  {label}: host residual |L y - lambda y| = {res:.3e}')
    assert res <= 2 * GAP_TOL, label
    return r


def pairs_by_kind(ei, n):
    """(pairs with a path, kinds, a pair without a path or None).  Up to three pairs of each kind of classes that the graph has
    (long - long, long - medium, ..., short - short), the edges between rows above the short limit first, from the first, last,
    middle and third-way row of each class; then pairs drawn by PCG64(n) up to RESISTANCE_BATCH + 5."""
    from dcr.graph import RESISTANCE_BATCH as B
    (nl, nm, ns), rows = spectral_ref.row_plan(ei, n)
    deg = np.bincount(np.asarray(ei)[0], minlength=n)
    klass = np.empty(n, dtype=np.int64)
    klass[rows] = np.repeat([0, 1, 2], [nl, nm, ns])
    linked = [rows[klass[rows] == k] for k in range(3)]
    linked = [c[deg[c] > 0] for c in linked]
    picks = [list(dict.fromkeys(int(c[i]) for i in (0, -1, len(c) // 2, len(c) // 3))) if len(c) else [] for c in linked]
    pairs, kinds = [], []

    def add(a, b):
        kind = 'LMS'[min(klass[a], klass[b])] + 'LMS'[max(klass[a], klass[b])]
        if a != b and (a, b) not in pairs and (b, a) not in pairs and kinds.count(kind) < 3:
            pairs.append((a, b))
            kinds.append(kind)
    for a, b in resistance_ref.edges(ei):
        if klass[a] < 2 and klass[b] < 2:
            add(int(a), int(b))
    for ka in range(3):
        for kb in range(ka, 3):
            for a in picks[ka]:
                for b in picks[kb][::-1]:
                    add(a, b)
    every = np.concatenate(linked)
    rng = np.random.Generator(np.random.PCG64(n))
    while len(pairs) < B + 5:
        a, b = (int(x) for x in rng.choice(every, 2, replace=False))
        if (a, b) not in pairs and (b, a) not in pairs:
            pairs.append((a, b))
            kinds.append('..')
    lone = np.flatnonzero(deg == 0)
    return np.array(pairs), kinds, ((picks[2][0], int(lone[-1])) if lone.size else None)


def check_resistances(G, d, pairs, no_path, n, label):
    """Two batches, the second padded; the pair without a path, where there is one, in the middle of the first."""
    from dcr.graph import RESISTANCE_BATCH as B
    assert B < len(pairs) < 2 * B
    asked = pairs if no_path is None else np.insert(pairs, 3, no_path, axis=0)
    lower, info = solve_pairs(G, asked)
    if no_path is not None:
        assert np.isposinf(lower[3]) and info['steps'][3] == 0 and info['residual'][3] == 0.0
        lower, info = np.delete(lower, 3), {k: np.delete(v, 3) for k, v in info.items()}
    want = d.resistance(pairs)
    assert np.isfinite(want).all()
    accept(lower, info['residual'], want, d.lambda1, n, label)
    print('  steps', info['steps'])
    return lower, info


@pytest.mark.parametrize('name', spectral_ref.PLAN_NAMES)
def test_family_sweep_bit_exact(family, name):
    ei, n, G, _, _ = family(name)
    check_sweeps(G, ei, n, name)


@pytest.mark.parametrize('name', spectral_ref.PLAN_NAMES)
def test_family_spectral_gap(family, name):
    ei, n, G, _, lam = family(name)
    check_gap(G, ei, n, lam, name)


@pytest.mark.parametrize('name', spectral_ref.PLAN_NAMES)
def test_family_effective_resistance(family, name):
    ei, n, G, d, _ = family(name)
    pairs, kinds, no_path = pairs_by_kind(ei, n)
    (nl, nm, ns), _ = spectral_ref.row_plan(ei, n)
    have = {'LL': nl > 1, 'LM': nl and nm, 'LS': nl and ns, 'MM': nm > 1, 'MS': nm and ns, 'SS': ns > 1}
    assert {k for k in kinds if k != '..'} == {k for k, there in have.items() if there}, kinds
    if name == BIG:
        assert {'LL', 'LM', 'LS', 'MS', 'SS'} <= set(kinds) and no_path is not None
    check_resistances(G, d, pairs, no_path, n, name)


def test_family_resistance_bits_do_not_depend_on_column_or_batch(family):
    """The three-long-row graph: the same pairs in reverse and rotated by seven, so that every pair changes its column and most
    change their batch and what shares it.  The same bits per pair (csrc/dcr_resistance.hip, the head comment)."""
    ei, n, G, d, _ = family(BIG)
    pairs, _, _ = pairs_by_kind(ei, n)
    P = len(pairs)
    base, info = solve_pairs(G, pairs)
    for label, perm in (('reversed', np.arange(P)[::-1]), ('rotated', np.roll(np.arange(P), 7))):
        lower, other = solve_pairs(G, pairs[perm])
        for k in range(P):
            got = (lower[k].hex(), other['residual'][k].hex(), int(other['steps'][k]))
            want = (base[perm[k]].hex(), info['residual'][perm[k]].hex(), int(info['steps'][perm[k]]))
            assert got == want, (label, k, pairs[perm[k]], got, want)


def test_family_foster_over_all_edges(family):
    """Foster on the three-long-row graph (n = 2,123, 9,124 edges): the resistances of all edges sum to n - c, under the
    bound of test_resistance_gpu.test_foster_and_curvature; every 37th of them against the dense value as well."""
    from experiment.effective_resistance import edge_resistances
    ei, n, G, d, _ = family(BIG)
    eu, ev, R = edge_resistances(G)
    E = len(R)
    assert E == G.number_of_edges() == resistance_ref.edges(ei).shape[0]
    bound = E * resistance_ref.allow(n, 1.0)
    print(f'  {E} edges: sum R - (n - c) = {R.sum() - (n - d.count):.3e}, bound {bound:.3e}')
    assert abs(R.sum() - (n - d.count)) <= bound
    some = np.stack([eu, ev], axis=1)[::37]
    lower, info = solve_pairs(G, some)
    assert lower.tobytes() == R[::37].tobytes()
    accept(lower, info['residual'], d.resistance(some), d.lambda1, n, 'every 37th edge')


# ---- limit crossings on a live handle ---------------------------------------------------------------------------------------------------
def test_rows_cross_both_limits_on_one_handle():
    """Hubs 0 and 1 of degree 32 and 2,048 over the leaves 2 .. 2049, and node 2050 with no edge, with both hub rows FULL: a row is
    laid out with max(8, deg / 4) free places (csrc/dcr_graph.hip, slack_for), so the handle is made with the hubs at degree 24
    and 1,639 and filled up by add_edge.  One more edge at the long hub then finds no place: all rows are laid out again, and
    both hubs are in the next class.  Removing another leaf from the middle of each row takes them back.  The plan, its device
    list and the buffers sized by the grid must follow on the same handle."""
    from dcr.graph import DcrGraph
    S, L = spectral_ref.SHORT_DEG, spectral_ref.LONG_DEG
    S0, L0 = 24, 1639
    assert S0 + max(8, S0 // 4) == S and L0 + max(8, L0 // 4) == L   # made at these degrees, a row has room up to the limit exactly
    n = 2 + L + 1
    made, _ = spectral_ref._und([(0, 2 + i) for i in range(S0)] + [(1, 2 + i) for i in range(L0)], n)
    G = DcrGraph(made, n)
    for i in range(S0, S):
        G.add_edge(0, 2 + i)
    for i in range(L0, L):
        G.add_edge(1, 2 + i)
    ei, _ = spectral_ref._und([(0, 2 + i) for i in range(S)] + [(1, 2 + i) for i in range(L)], n)
    assert np.array_equal(resistance_ref.edges(G.to_edge_index()), resistance_ref.edges(ei))
    spare = n - 1
    pairs = [(0, 1), (0, 2), (1, 2), (0, 2 + S), (1, 2 + L - 1), (2, 3), (2 + S - 1, 2 + L - 1), (5, 1500), (1, spare), (2 + S, spare)]

    def check(counts, degrees, label):
        live = G.to_edge_index()
        assert spectral_ref.row_plan(live, n)[0] == counts and (G.degree(0), G.degree(1)) == degrees, label
        check_sweeps(G, live, n, label)
        r = check_gap(G, live, n, spectral_ref.lambda1(live, n), label)
        d = resistance_ref.Dense(live, n)
        lower, info = solve_pairs(G, pairs)
        want = d.resistance(pairs)
        fin = np.isfinite(want)
        assert np.array_equal(np.isposinf(lower), ~fin) and fin.sum() >= 8, label
        accept(lower[fin], info['residual'][fin], want[fin], d.lambda1, n, label)
        return live, r

    check((0, 1, n - 1), (S, L), 'at the limits')
    G.add_edge(1, spare)     # the 2,049th entry of a row with 2,048 places
    G.add_edge(0, 2 + S)
    live, r = check((1, 1, n - 2), (S + 1, L + 1), 'one past the limits')
    gap, cut, score = G.fiedler_sweep()   # the sweep runs on the plan the solver hands back
    assert gap.lambda1.hex() == r.lambda1.hex() and gap.residual.hex() == r.residual.hex()
    assert_same(cut, sweep_ref.sweep(live, n, score, 'conductance'), 'fiedler sweep, one past the limits')
    assert gap.lambda1 / 2 <= cut.value <= np.sqrt(2 * gap.lambda1)
    G.remove_edge(0, 2 + 5)
    G.remove_edge(1, 2 + 1000)
    live, _ = check((0, 1, n - 1), (S, L), 'back at the limits, a hole in each row')
    assert not np.array_equal(resistance_ref.edges(live), resistance_ref.edges(ei))
