"""The host oracles of the heat-kernel diffusion (tests/heat_ref.py) against each other and against what exact arithmetic says of
the Taylor sum, and the Python surface that needs no device: the option structure and the `kernel` switch."""
import ctypes

import numpy as np
import pytest

import heat_ref as ref

L = np.longdouble
HUB_SOURCES = [0, 1, 2, 17, 2100, 2101, 2102, 2103, 5, 900, 1500, 2099, 3, 4, 6, 7, 8]


@pytest.mark.parametrize('name', list(ref.graphs()))
def test_the_two_oracles_agree(name):
    """The recurrence in np.longdouble with 40 terms past K against the spectral form: independent routes, within the allowance
    of the dense one (the recurrence's own tail and rounding are far below it)."""
    ei, n = ref.graphs()[name]
    src = HUB_SOURCES if name == 'hub2100' else list(range(n))
    for t in ref.HEAT_TS:
        K = ref.terms(t, ref.TOL)
        x = ref.taylor_long(ei, n, t, src, K + ref.ORACLE_EXTRA)
        S = ref.dense(ei, n, t, key=name)
        dev = float(np.abs(x - S[src]).max())
        print(f'  {name} t {t}: K {K}, |taylor - dense| = {dev:.3e}, allow {ref.dense_allow(n):.3e}')
        assert ref.tail(t, K + ref.ORACLE_EXTRA) <= 1e-30 and dev <= ref.dense_allow(n), (name, t)


@pytest.mark.parametrize('tol', [1e-6, 1e-10])
@pytest.mark.parametrize('t', [0.5, 5, 20])
def test_terms_is_the_smallest_count_with_its_tail_within_half_tol(t, tol):
    K = ref.terms(t, tol)
    assert K >= 1 and ref.tail(t, K) <= L(tol) / 2 < ref.tail(t, K - 1), (t, tol, K)
    assert abs(float(ref.thetas(t).sum()) - 1.0) <= 4 * ref.EPS            # the thetas are the Poisson weights
    assert ref.terms(t, tol, max_terms=3) == 3 and ref.terms(t, tol, max_terms=K + 7) == K


def test_missing_mass_is_the_tail():
    """sum_i r_i x_i = r_j (1 - rho_K) for the partial sum x of K terms after the first, because H r = r: the identity the
    reported deficit rests on, here in np.longdouble on a graph with a hub, leaves and an isolated node."""
    for name in ('barbell20_4', 'star6', 'random300'):
        ei, n = ref.graphs()[name]
        _, _, r, _ = ref.operator_long(ei, n)
        for t in ref.HEAT_TS:
            for K in (0, 3, ref.terms(t, ref.TOL)):
                src = [0, n // 2, n - 1]
                x = ref.taylor_long(ei, n, t, src, K)
                mass = x @ r
                want = r[src] * (L(1) - ref.tail(t, K))
                assert np.all(x >= 0) and float(np.abs(mass - want).max()) <= (K + 2) * n * float(np.finfo(L).eps) * float(r.max()), (name, t, K)
    ei, n = ref.graphs()['path8']
    x = ref.taylor_long(np.zeros((2, 0), dtype=np.int64), 3, 5.0, [1], 60)    # no edges: S = I
    assert abs(float(x[0, 1]) - 1.0) <= 1e-18 and x[0, 0] == 0 and x[0, 2] == 0


def test_allowance_counts_the_roundings_of_a_term():
    assert ref.allow(0, 0) == 12 * ref.EPS and ref.allow(24, 2100) == 25 * 2112 * ref.EPS
    assert ref.allow(ref.terms(20.0, ref.TOL), 2100) < 1e-10                 # far below the entries the selection keeps


def test_heat_opts_layout():
    from dcr import _lib
    assert [f[0] for f in _lib.HeatOpts._fields_] == ['t', 'tol', 'max_terms']
    assert [f[1] for f in _lib.HeatOpts._fields_] == [ctypes.c_double, ctypes.c_double, ctypes.c_int64]
    assert ctypes.sizeof(_lib.HeatOpts) == 24
    assert (_lib.HeatOpts.t.offset, _lib.HeatOpts.tol.offset, _lib.HeatOpts.max_terms.offset) == (0, 8, 16)
    assert {'dcr_heat_columns', 'dcr_heat_sparsify'} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES['dcr_heat_columns'][1]) == 7 and len(_lib.SIGNATURES['dcr_heat_sparsify'][1]) == 15
    assert _lib.SIGNATURES['dcr_heat_sparsify'][1][-2] == _lib._i64p        # K is one int64, not a step count per column


def test_bad_kernel_and_bad_t_are_value_errors_before_any_device_call():
    """No graph handle exists here: the checks come first."""
    from dcr.data import Data
    from dcr.graph import DcrGraph
    from rewiring.diffusion import digl
    G = object.__new__(DcrGraph)
    for bad in ('gauss', 'PPR', None, ''):
        with pytest.raises(ValueError, match='kernel'):
            G.diffusion(k=4, kernel=bad)
        with pytest.raises(ValueError, match='kernel'):
            digl(Data(num_nodes=3), kernel=bad)
    for bad in (0.0, -1.0, float('nan'), 257.0):
        with pytest.raises(ValueError, match='t must'):
            G.heat([0], t=bad)
