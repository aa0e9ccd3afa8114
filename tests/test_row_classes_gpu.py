"""All three row classes of the analysis kernels in one launch, and the class limits themselves: spectral_ref.row_classes_graph has
rows of degree 32 | 33 and 2,048 | 2,049 next to short ones, a second component and an isolated node.  Nothing new is accepted
here: the sweep is compared bit for bit (tests/sweep_ref.py), the gap and the resistances under the rules of
test_cheeger_bounds_gpu.py and test_resistance_gpu.py against the dense restatements."""
import numpy as np
import pytest

import resistance_ref
import spectral_ref
import sweep_ref
from test_cheeger_bounds_gpu import check_against, solve as solve_gap
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
