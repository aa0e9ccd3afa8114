"""FoSR without a GPU: the rule of include/dcr.h (tests/fosr_ref.py) against the dense brute-force minimum, the margins that let
tests/test_fosr_gpu.py demand equal edge sequences, the host-side plan patching alone under the sanitizers, and the call surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import fosr_ref
import spectral_ref
from conftest import PKG, REPO

CSRC = os.path.join(PKG, 'csrc')


def small_graphs():
    rng = np.random.Generator(np.random.PCG64(21))
    out = [spectral_ref.path(2), (np.zeros((2, 0), dtype=np.int64), 2), spectral_ref.path(5), spectral_ref.star(7), spectral_ref.cycle(9),
           spectral_ref.barbell(4, 3), (np.zeros((2, 0), dtype=np.int64), 5)]
    for _ in range(50):
        n = int(rng.integers(2, 15))
        out.append(fosr_ref.random_graph(n, float(rng.choice([0.15, 0.4, 0.7, 0.95])), rng))
    return out


def test_rule_attains_the_brute_force_minimum():
    """On a few hundred (graph, vector) pairs the rule's product is the smallest fl(y_u y_v) over the free pairs, and the pair it
    names is free and has that product."""
    rng = np.random.Generator(np.random.PCG64(7))
    cases = 0
    for ei, n in small_graphs():
        _, deg, rows = fosr_ref.degrees_and_rows(ei, n)
        for name, x in fosr_ref.vector_kinds(n, rng).items():
            y = fosr_ref.y_of(x, deg)
            got, want = fosr_ref.pick(y, rows), fosr_ref.brute_minimum(y, rows)
            assert (got is None) == (want is None), (n, name)
            if got is not None:
                u, v, p = got
                assert u != v and v not in rows[u] and p == want and p == y[u] * y[v], (n, name, got, want)
            cases += 1
    assert cases >= 300


def test_fast_row_products_are_the_rule():
    """fosr_ref.row_products_fast (array operations on the CSR adjacency, what the GPU tests of 70,001 and 262,182 nodes compare
    with) returns what fosr_ref.row_products returns, on every graph and vector kind of this file: products by bits, partners by
    value, the rows without a candidate included."""
    rng = np.random.Generator(np.random.PCG64(9))
    graphs = small_graphs() + [spectral_ref.complete(n) for n in (2, 3, 6, 11)] + [spectral_ref.path(4)]
    graphs += [fosr_ref.irregular_graph(300, seed=5, isolated=1), spectral_ref.row_classes_graph()]
    graphs += [fosr_ref.loop_fixture(name)[:2] for name, *_ in fosr_ref.LOOP_FIXTURES]
    cases = 0
    for ei, n in graphs:
        a, deg, rows = fosr_ref.degrees_and_rows(ei, n)
        vectors = dict(fosr_ref.vector_kinds(n, rng))
        vectors['with_infinities'] = np.where(rng.random(n) < 0.3, np.inf, vectors['both_zeros'])    # 0 x inf: not a candidate
        for name, x in vectors.items():
            if n > 1000 and name not in ('normal', 'small_integers', 'both_zeros', 'negative'):
                continue
            y = fosr_ref.y_of(x, deg)
            with np.errstate(invalid='ignore'):
                p, partner = fosr_ref.row_products(y, rows)
            fp, fpartner = fosr_ref.row_products_fast(y, a)
            assert p.tobytes() == fp.tobytes() and np.array_equal(partner, fpartner), (n, name)
            assert fosr_ref.pick_of(p, partner) == fosr_ref.pick_of(fp, fpartner)
            cases += 1
    assert cases >= 400


def test_fast_loop_is_the_loop():
    name = 'irregular200'
    ei, n, x0, iters, (edges, x, margins) = fosr_ref.loop_fixture(name)
    fast = fosr_ref.loop_fast(ei, n, iters, fosr_ref.LOOP_INITIAL, x0)
    assert np.array_equal(fast[0], edges) and fast[1].tobytes() == x.tobytes() and fast[2] == margins
    assert [list(p[:2]) for p in fast[3]] == edges.T.tolist()
    again = fosr_ref.loop_fast(ei, n, iters, fosr_ref.LOOP_INITIAL, x0, replay=edges)
    assert np.array_equal(again[0], edges) and again[1].tobytes() == x.tobytes()


def test_large_loop_has_a_margin_and_the_reference_knows_its_rounding():
    """The loop of tests/test_fosr_gpu.py at 70,001 nodes: in the restatement's own run every one of the ten runner-up margins is
    above the bound the GPU test uses (16 times the float64 step's difference from the np.longdouble step), far above; the GPU
    test allows one iteration under it.  And that bound stays under the ceiling of 1e-12 at 262,182 nodes too."""
    import scale_ref
    ei, n = scale_ref.whole_small()
    a = spectral_ref.adjacency(ei, n)
    deg = np.diff(a.indptr).astype(np.int64)
    x0 = np.random.Generator(np.random.PCG64(fosr_ref.LOOP_LARGE_SEED)).standard_normal(n)
    own = fosr_ref.own_rounding(a, deg, x0, 1)
    edges, x, margins, picks = fosr_ref.loop_fast(ei, n, fosr_ref.LOOP_LARGE_ITERS, fosr_ref.LOOP_INITIAL, x0)
    print(f'n = {n}: the reference against itself {own:.3e}; margins {min(margins):.3e} .. {max(margins):.3e}')
    assert 0 < 16 * own < 1e-12 and len(margins) == fosr_ref.LOOP_LARGE_ITERS
    assert sum(m <= 16 * own for m in margins) == 0 and min(margins) >= 1e-6
    assert abs(np.linalg.norm(x) - 1.0) < 1e-12
    ei, n = scale_ref.fosr_large()
    a = spectral_ref.adjacency(ei, n)
    deg = np.diff(a.indptr).astype(np.int64)
    x0 = np.random.Generator(np.random.PCG64(26)).standard_normal(n)
    for steps in (1, 5):
        own = fosr_ref.own_rounding(a, deg, x0, steps)
        print(f'n = {n}, {steps} steps: the reference against itself {own:.3e}')
        assert 0 < 16 * own < 1e-12


def test_long_double_step_is_the_step():
    """power_step_long is power_step in another precision: on a small graph they agree to float64 rounding, and np.longdouble is
    wider than float64 here (otherwise own_rounding would measure nothing)."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    ei, n = fosr_ref.irregular_graph(300, seed=5, isolated=1)
    a, deg, _ = fosr_ref.degrees_and_rows(ei, n)
    x0 = np.random.Generator(np.random.PCG64(1)).standard_normal(n)
    xl = fosr_ref.power_step_long(a, deg, x0)
    assert xl.dtype == np.longdouble and np.abs(fosr_ref.power_step(a, deg, x0) - xl).max() < 1e-15
    assert 0 < fosr_ref.own_rounding(a, deg, x0, 1) < 1e-15
    dense = a.toarray().astype(np.longdouble) @ x0.astype(np.longdouble)
    assert np.abs(spectral_ref.csr_matvec_long(a, x0) - dense).max() < 1e-17


@pytest.mark.parametrize('n', [2, 3, 6, 11])
def test_complete_graphs_have_no_pick(n):
    ei, _ = spectral_ref.complete(n)
    _, deg, rows = fosr_ref.degrees_and_rows(ei, n)
    for x in fosr_ref.vector_kinds(n, np.random.Generator(np.random.PCG64(n))).values():
        assert fosr_ref.pick(fosr_ref.y_of(x, deg), rows) is None and fosr_ref.brute_minimum(fosr_ref.y_of(x, deg), rows) is None


def test_ties_go_to_the_smallest_node_and_zeros_are_one_value():
    ei, n = spectral_ref.path(4)       # free pairs: (0, 2), (0, 3), (1, 3)
    _, deg, rows = fosr_ref.degrees_and_rows(ei, n)
    assert fosr_ref.pick(np.zeros(n), rows) == (0, 2, 0.0)                      # every product 0: u = 0, its first eligible node
    assert fosr_ref.pick(np.array([-0.0, 0.0, -0.0, 0.0]), rows)[:2] == (0, 2)  # -0.0 == 0.0 in the order and in the arg-min
    assert fosr_ref.pick(np.array([1.0, 1.0, 1.0, 1.0]), rows) == (0, 2, 1.0)
    assert fosr_ref.pick(np.array([-1.0, 5.0, 2.0, 3.0]), rows) == (0, 3, -3.0)  # y_0 < 0: the LAST eligible node


@pytest.mark.parametrize('name', [f[0] for f in fosr_ref.LOOP_FIXTURES])
def test_loop_fixtures_have_a_margin(name):
    """What makes equality of the edge sequences a fair demand on the GPU: at every iteration of the restatement's own run the
    runner-up is at least 1e-6 max |y|^2 away.  (Both ends of the picked pair attain the minimum, so the runner-up is the best of
    the other rows: fosr_ref.runner_up_margin.)"""
    ei, n, x0, iters, (edges, x, margins) = fosr_ref.loop_fixture(name)
    assert edges.shape == (2, iters) and len(margins) == iters and 30 <= iters <= 60 and 200 <= n <= 2500
    print(name, 'smallest margin', min(margins), 'at iteration', int(np.argmin(margins)))
    assert min(margins) >= 1e-6
    assert abs(np.linalg.norm(x) - 1.0) < 1e-12
    # a replay of the same picks is the same run
    again = fosr_ref.loop(ei, n, iters, fosr_ref.LOOP_INITIAL, x0, replay=edges)
    assert np.array_equal(again[0], edges) and again[1].tobytes() == x.tobytes()


def test_loop_fixture_shapes():
    comps = {name: spectral_ref.components(*fosr_ref.loop_fixture(name)[:2])[0] for name, *_ in fosr_ref.LOOP_FIXTURES}
    assert comps['irregular200'] == 1 and comps['two_components600'] == 2
    ei, n, _, _, (edges, _, _) = fosr_ref.loop_fixture('two_components600')
    labels = spectral_ref.components(ei, n)[1]
    assert labels[edges[0, 0]] != labels[edges[1, 0]]      # the first added edge joins the components


def test_power_step_keeps_the_unit_sphere_and_the_complement():
    ei, n = fosr_ref.irregular_graph(300, seed=5, isolated=1)
    a, deg, _ = fosr_ref.degrees_and_rows(ei, n)
    x = fosr_ref.power_step(a, deg, np.random.Generator(np.random.PCG64(1)).standard_normal(n))
    assert abs(np.linalg.norm(x) - 1.0) < 1e-14 and abs(np.dot(x, np.sqrt(deg))) < 1e-12
    assert fosr_ref.power_step(a, deg, np.zeros(n)) is None      # |z| = 0: the loop stops


def test_plan_patching_alone_under_the_sanitizers(tmp_path):
    """csrc/dcr_row_patch.h is pure host code: tests/row_patch_check.cpp includes it and nothing of the library, and compares the
    patched plan with a full rebuild after every edit of random sequences that cross both class limits, under
    -fsanitize=address,undefined (a stand-alone program: nothing is loaded into this process)."""
    header = open(os.path.join(CSRC, 'dcr_row_patch.h')).read()
    assert sorted(re.findall(r'#include\s*[<"]([^>"]+)', header)) == ['algorithm', 'stdint.h', 'vector']   # no HIP include
    exe = str(tmp_path / 'row_patch_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC,
                           os.path.join(REPO, 'tests', 'row_patch_check.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == '', run.stderr
    edits, lower, upper = (int(t) for t in run.stdout.split())
    assert edits > 5000 and lower > 100 and upper > 100


def test_call_surface():
    from dcr import _lib, graph
    from dcr.graph import DcrGraph
    header = open(os.path.join(REPO, 'include', 'dcr.h')).read()
    for name in ('dcr_fosr_pick', 'dcr_fosr'):
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert m, name + ' is not declared in include/dcr.h'
        params = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
        assert len(params.split(',')) == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r'typedef\s+struct\s*\{\s*int64_t\s+num_iterations\s*,\s*initial_power_iters\s*;\s*uint64_t\s+seed\s*;\s*\}\s*dcr_fosr_opts',
                     header)
    assert [f[0] for f in _lib.FosrOpts._fields_] == ['num_iterations', 'initial_power_iters', 'seed']
    assert callable(DcrGraph.fosr_pick) and callable(DcrGraph.fosr)
    source = open(os.path.join(CSRC, 'dcr_fosr.hip')).read()
    assert int(re.search(r'constexpr\s+int\s+FSR_WINDOW\s*=\s*(\d+)\s*;', source).group(1)) == graph.FOSR_WINDOW
    assert 'dcr_fosr' in open(os.path.join(CSRC, 'build.sh')).read().split()
    from rewiring.fosr import fosr
    assert callable(fosr)
