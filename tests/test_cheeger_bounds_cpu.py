"""The spectral bracket of the Cheeger constant without a GPU: tests/spectral_ref.py (the dense restatement the GPU tests compare
with) against the reference's recorded output, tests/golden/cheeger_bounds_reference.json, and against closed forms; the
conditions the fixture has to meet; the call surface of experiment/cheeger_bounds.py."""
import numpy as np
import pytest

import spectral_ref
from conftest import load_golden


def fh(s):
    return float.fromhex(s)


def case_graph(case):
    from dcr import synthetic
    if case['generator'] is not None:   # a generator of dcr/synthetic.py, or of tests/spectral_ref.py
        (fn, args), = case['generator'].items()
        ei, n = (getattr(synthetic, fn) if hasattr(synthetic, fn) else getattr(spectral_ref, fn))(*args)
        assert n == case['num_nodes']
        return ei, n
    return np.asarray(case['edge_index'], dtype=np.int64).reshape(2, -1), case['num_nodes']


@pytest.fixture(scope='module')
def fixture():
    return load_golden('cheeger_bounds_reference.json')


def test_restatement_reproduces_the_recorded_eigenvalues(fixture):
    """To 8 n 2^-52: eigh's backward error at |L| <= 2, all that separates two runs of the same LAPACK on permuted input."""
    for case in fixture['graphs']:
        ei, n = case_graph(case)
        c, labels = spectral_ref.components(ei, n)
        assert c == case['components'], case['name']
        want = np.array([fh(h) for h in case['eigenvalues']])
        got = spectral_ref.eigenvalues(ei, n)[:c + 3]
        err = np.abs(got - want).max()
        print(case['name'], 'eigenvalue error', err, 'bound', 8 * n * spectral_ref.EPS)
        assert err <= 8 * n * spectral_ref.EPS, case['name']
        assert abs(spectral_ref.lambda1(ei, n) - want[c]) <= 8 * n * spectral_ref.EPS


def test_restatement_reproduces_the_reference_strings_where_it_is_sound(fixture):
    for case in fixture['graphs']:
        if not case['reference_sound']:
            continue
        ei, n = case_graph(case)
        assert list(spectral_ref.bounds_strings(spectral_ref.lambda1(ei, n))) == case['reference'], case['name']
        assert fh(case['reference_lambda1']) == fh(case['eigenvalues'][case['components']]), case['name']


def test_fixture_has_sound_and_unsound_graphs(fixture):
    sound = [c['name'] for c in fixture['graphs'] if c['reference_sound']]
    unsound = [c['name'] for c in fixture['graphs'] if not c['reference_sound']]
    assert len(sound) >= 3 and len(unsound) >= 2, (sound, unsound)
    for case in fixture['graphs']:
        lam = [fh(h) for h in case['eigenvalues']]
        c = case['components']
        assert len(lam) == c + 3
        assert case['reference_sound'] == all(v <= 0 for v in lam[:c]), case['name']
        if not case['reference_sound']:   # what the reference took is noise of a zero eigenvalue, far below the true gap
            assert 0 < fh(case['reference_lambda1']) < 1e-12 < lam[c], case['name']


def test_fixture_bounds_are_clear_of_rounding_boundaries(fixture):
    """No recorded lambda_1 / 2 or sqrt(2 lambda_1) within 1e-6 relative of a value where ' .2e' changes its last digit."""
    for case in fixture['graphs']:
        lam = fh(case['eigenvalues'][case['components']])
        for x in (lam / 2, np.sqrt(2 * lam)):
            m = x / 10.0 ** np.floor(np.log10(x)) * 100.0
            assert abs(m - (np.floor(m) + 0.5)) / m >= 1e-6, (case['name'], x)


@pytest.mark.parametrize('name', [c[0] for c in spectral_ref.closed_forms()])
def test_closed_forms_hold_for_the_restatement(name):
    (ei, n), want = {c[0]: c[1:] for c in spectral_ref.closed_forms()}[name]
    got = spectral_ref.lambda1(ei, n)
    print(name, got, want)
    assert abs(got - want) <= 8 * n * spectral_ref.EPS


def test_components_and_null_vectors_of_the_restatement():
    ei = np.array([[0, 1, 1, 2, 4, 5], [1, 0, 2, 1, 5, 4]])
    c, labels = spectral_ref.components(ei, 7)
    assert c == 4 and labels.tolist() == [0, 0, 0, 3, 4, 4, 6]
    K = spectral_ref.null_vectors(ei, 7)
    L = spectral_ref.laplacian(ei, 7)
    assert K.shape == (4, 7) and np.abs(L @ K.T).max() <= 4 * spectral_ref.EPS
    assert np.abs(K @ K.T - np.eye(4)).max() <= 4 * spectral_ref.EPS
    with pytest.raises(ValueError):
        spectral_ref.lambda1(np.zeros((2, 0), dtype=np.int64), 3)


def test_module_surface_and_format():
    """Fails before the feature: experiment.cheeger_bounds does not exist."""
    import inspect
    import experiment.cheeger_bounds as cb
    from dcr import _lib
    from dcr.graph import DcrGraph, SpectralGap
    assert list(inspect.signature(cb.cheeger_bounds).parameters) == ['data']
    assert cb.format_bounds(0.046309425394 / 2, np.sqrt(2 * 0.046309425394)) == (' 2.32e-02', ' 3.04e-01')   # the recorded 8x8 grid
    assert cb.format_bounds(2.5e-18, 3.2e-9) == (' 2.50e-18', ' 3.20e-09')
    with pytest.raises(TypeError):
        cb.cheeger_bounds_values(None, tolerance=1e-3)
    assert SpectralGap._fields == ('lambda1', 'residual', 'steps', 'restarts', 'components', 'converged', 'vector')
    assert SpectralGap(0.5, 1e-11, 10, 0, 1, True).vector is None
    sig = inspect.signature(DcrGraph.spectral_gap).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [('tol', 1e-10), ('max_steps', 20000), ('max_basis', None), ('seed', 0),
                                                            ('return_vector', False)]
    assert hasattr(DcrGraph, 'connected_components')
    assert {'dcr_spectral_gap', 'dcr_connected_components'} <= set(_lib.SIGNATURES)
    assert [f[0] for f in _lib.SpectralOpts._fields_] == ['tol', 'max_steps', 'max_basis', 'seed']
    assert [f[0] for f in _lib.SpectralResult._fields_] == ['lambda1', 'residual', 'steps', 'restarts', 'components', 'converged']
    assert 'cheeger_bounds.py:16' in cb.__doc__ or ':16' in cb.__doc__
