"""The dense restatement tests/diffusion_ref.py, pinned on the CPU: against the reference's two sparsifiers as recorded in
tests/golden/diffusion_reference.json (tools/make_golden_diffusion.py ran them), against closed forms of the personalised-PageRank
matrix, and the constants of the column CG in csrc/dcr_analysis.h against those the row-plan family was built for."""
import os
import re

import numpy as np
import pytest

import diffusion_ref as ref
from conftest import GOLDEN, PKG, load_golden

CSRC = os.path.join(PKG, 'csrc')


@pytest.fixture(scope='module')
def fixture():
    return load_golden('diffusion_reference.json')


@pytest.fixture(scope='module')
def fixture_graph(fixture):
    (fn, args), = fixture['graph'].items()
    ei, n = getattr(ref, fn)(*args)
    assert n == fixture['num_nodes']
    return ei, n


# ---- 1. the reference's helpers ----------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_helpers(fixture, fixture_graph):
    ei, n = fixture_graph
    k = fixture['k']
    assert [c['alpha'] for c in fixture['cases']] == list(ref.ALPHAS)
    for case in fixture['cases']:
        assert case['top_k_gap'] > fixture['gap'] and case['eps_gap'] > fixture['gap']   # no tie the reference's argsort could break
        S = ref.ppr_matrix(ei, n, case['alpha'])
        for name, kw in (('top_k', {'k': k}), ('clipped', {'eps': case['eps']})):
            want_ptr, want_rows, want_w = ref.recorded(GOLDEN, fixture, case[name])
            ptr, rows, w, _ = ref.sparsify(S, **kw)
            assert np.array_equal(ptr, want_ptr) and np.array_equal(rows, want_rows), (case['alpha'], name)
            kept = np.repeat(np.diff(ptr), np.diff(ptr))
            err = np.abs(w - want_w)
            print(f'  alpha {case["alpha"]} {name}: {rows.size} entries, columns of {np.diff(ptr).min()} .. {np.diff(ptr).max()}, '
                  f'max weight error {err.max():.3e}')
            assert np.all(err <= 8 * kept * ref.EPS), (case['alpha'], name)
        assert np.all(np.diff(ref.recorded(GOLDEN, fixture, case['top_k'])[0]) == k)
        assert np.diff(ref.recorded(GOLDEN, fixture, case['clipped'])[0]).min() >= 1


def test_tie_break_is_larger_value_then_smaller_id():
    col = np.array([0.5, 0.25, 0.5, 0.125, 0.25, 0.5])
    assert ref.top_k(col, 1).tolist() == [0]
    assert ref.top_k(col, 2).tolist() == [0, 2]
    assert ref.top_k(col, 4).tolist() == [0, 1, 2, 5]
    assert ref.top_k(col, 9).tolist() == [0, 1, 2, 3, 4, 5]
    assert ref.threshold(col, 0.25).tolist() == [0, 1, 2, 4, 5] and ref.threshold(col, 0.75).size == 0
    ptr, rows, w, v = ref.sparsify(col[:, None], eps=0.75)
    assert ptr.tolist() == [0, 0] and rows.size == 0 and w.size == 0
    assert ref.ordered_sum([0.1, 0.2, 0.3]) == (0.1 + 0.2) + 0.3


# ---- 2. closed forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', ref.ALPHAS)
@pytest.mark.parametrize('n', [5, 40])
def test_complete_graph_closed_form(n, alpha):
    ei, _ = ref.complete(n)
    S = ref.ppr_matrix(ei, n, alpha)
    want = alpha * np.eye(n) + (1 - alpha) / n
    assert np.abs(S - want).max() <= ref.allow(n)


@pytest.mark.parametrize('alpha', ref.ALPHAS)
def test_isolated_node_and_symmetry(alpha):
    ei, n = ref.triangle_star_isolated()
    S = ref.ppr_matrix(ei, n, alpha)
    assert abs(S[8, 8] - 1.0) <= ref.allow(n) and np.all(S[8, :8] == 0) and np.all(S[:8, 8] == 0)
    assert np.all(S[:3, 3:] == 0)                       # nothing crosses components
    for name, (ei, n) in ref.graphs().items():
        if n > 400:
            continue
        S = ref.ppr_matrix(ei, n, alpha)
        assert np.abs(S - S.T).max() <= ref.allow(n), name
        assert np.all(S > 0), name                      # connected graphs


def test_solve_and_inverse_agree_within_the_allowance():
    """The acceptance rule of tests/test_diffusion_gpu.py adds allow = 64 n 2^-52 for the dense reference's own rounding: here
    numpy's solve and inv, two routes to the same S, are within it on every graph the GPU tests compare against S."""
    for name, (ei, n) in ref.graphs().items():
        for alpha in ref.ALPHAS:
            S = ref.ppr_matrix(ei, n, alpha)
            dev = np.abs(S - alpha * np.linalg.inv(ref.operator(ei, n, alpha))).max()
            print(f'  {name} alpha {alpha}: |solve - inv| = {dev:.3e}, allow {ref.allow(n):.3e}')
            assert dev <= ref.allow(n), (name, alpha)


# ---- 3. the constants in the source ------------------------------------------------------------------------------------------------
def constant(text, name):
    m = re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, text)
    assert m, name + ' not found'
    return int(m.group(1))


def test_geometry_is_that_of_the_resistance_mat_vec():
    dif = open(os.path.join(CSRC, 'dcr_diffusion.hip')).read()
    res = open(os.path.join(CSRC, 'dcr_resistance.hip')).read()
    header = open(os.path.join(CSRC, 'dcr_analysis.h')).read()
    # one geometry and one batch width, in the header; neither file keeps a copy of its own
    assert constant(header, 'COL_SHORT_LANES') == 32 and constant(header, 'COL_SHORT_ROWS') == 64
    m = re.search(r'#\s*define\s+DCR_COL_B\s+(\d+)', header)
    assert m and int(m.group(1)) == 16 and re.search(r'constexpr\s+int\s+COL_B\s*=\s*DCR_COL_B\s*;', header)
    assert re.search(r'constexpr\s+int\s+COL_CP\s*=\s*COL_B\s*/\s*2\s*;', header)
    assert re.search(r'using\s+ColRows\s*=\s*RowGeom<\s*COL_SHORT_LANES\s*,\s*COL_SHORT_ROWS\s*/\s*8\s*,\s*COL_CP\s*>', header)
    for text in (dif, res):
        assert not re.search(r'RowGeom\s*<|_SHORT_LANES\s*=|_SHORT_ROWS\s*=|#\s*define\s+DCR_\w*_B\b', text)
        assert 'row_grid<ColRows>' in text and 'col_cg_solve' in text
    assert 'walk_rows<ColRows>' in header and 'walk_rows<ColRows>' in dif   # the CG mat-vec; k_heat_term
    assert constant(header, 'SP_CHECK_EVERY') >= 1 and len(re.findall(r'% SP_CHECK_EVERY', header)) == 1
    from dcr import graph
    assert graph.DIFFUSION_BATCH == graph.RESISTANCE_BATCH == int(m.group(1))


def test_entry_points_are_declared_and_bound():
    from dcr import _lib
    assert {'dcr_ppr_columns', 'dcr_diffusion_sparsify'} <= set(_lib.SIGNATURES)
    assert [f[0] for f in _lib.DiffusionOpts._fields_] == ['alpha', 'tol', 'max_steps']
    import rewiring.diffusion
    assert 'utils/adjacency_matrix_ops.py:26-39' in rewiring.diffusion.__doc__
