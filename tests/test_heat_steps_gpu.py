"""The heat kernel's Taylor recurrence on the GPU (k_heat_start, k_heat_term, k_heat_mass and the loop of diffusion_batches in
csrc/dcr_diffusion.hip), term by term and entry by entry, against the host replica tests/heat_steps_ref.py.

``G.heat(src, t=..., max_terms=k, return_info=True)`` returns the partial sum after exactly k terms, so the device can be cut at
every term.  The acceptance rule of tests/test_heat_gpu.py compares a column with the full column S_j inside a window as wide as
deficit_j / r_i and uses heat_ref.allow as an absolute number, below which most entries of a column lie on any graph of more than a
few hops: a long row that loses a small share of its gather, a dropped self term far from the source, a z buffer read on the wrong
parity or a relative error of 1e-3 in the entries below 1e-12 can pass it wherever the entries concerned lie below that number
(tests/test_heat_steps_cpu.py runs two such solvers through both rules and says what the old one answers).  Here every cut of every case goes through heat_steps_ref.compare, all of it derived and nothing tuned against the device:
    relative   |x_i - X_i| <= a X_i, X the np.longdouble partial sum of the same k terms, a = heat_ref.allow(k, d_max);
    support    x_i == 0.0 exactly outside the ball of radius k about the source, x_i > 0 inside;
    deficit    |deficit_j - r_j rho_k| <= ((n + 2) 2^-52 + a) r_j, also at small k where rho_k is O(1): a test of k_heat_mass.
Every other value comparison in this file is bytes against bytes.  A cut call warns by design (RuntimeWarning) and reports no
column as converged; the call at K must not warn.

    case  graph, sources                                      t          cuts
    A     barbell20_4, all 44 (two full batches, one padded)  5          every k = 1 .. 25     both buffer parities, padding columns
    B     the 8 graphs of PLAN_NAMES, plan_sources' picks     5          1, 2, 3, 24, 25       every row class at its boundaries
    C     hub2100, HUB_SOURCES                                0.5, 20    1, 2, K               the row of 2,100 slots
    D     path(300), sources 0, 150, 299                      20         1, 2, 5, 10 .. 50, 55 the support grows a node a term
    E     triangle_star_isolated, all 9                       0.5        every k = 1 .. 10     isolated source, components
    F     33,133 nodes, the 17 large_sources                  5          1, 2, 3, 25           second grid-stride trip, two launches
    G     path(8), sources 2 and 7                            256        1, 2, 366             v_0 = e^-256

What was seen on an MI355X (records, not thresholds; the thresholds are the derived ones above).  Per case, over all its cuts,
sources and entries: the |x - X| / X that came closest to its allowance a, the deficit distance |deficit - r rho_k| / r that came
closest to its own, and beside them the largest |x - X| / (a X) of the float64 replica of tests/test_heat_steps_cpu.py, which
restates the device's operation order on the CPU:
    case  K        |x - X| / X   of a          at k   device / a   CPU / a    deficit       of            at k
    A     25       1.0e-15       2.8e-14       3      0.035        0.035      1.1e-15       6.7e-14       7
    B     25       6.8e-15       8.1e-14       25     0.084        0.084      1.6e-15       1.4e-13       24     (mid0_short257; the other seven below 0.02)
    C     10, 55   1.3e-15       1.4e-12       2      0.0009       0.0009     3.4e-16       1.9e-12       2      (t = 20; t = 0.5 below it)
    D     55       6.2e-15       6.5e-14       20     0.095        0.095      5.3e-15       1.6e-13       30
    E     10       3.2e-16       7.1e-15       1      0.045        0.045      2.3e-16       1.3e-14       2
    F     25       1.1e-15       1.4e-12       2      0.0008       0.0008     7.5e-16       2.0e-11       25
    G     366      2.8e-16       6.2e-15       1      0.045        0.045      4.7e-14       1.1e-12       366
No kernel was found wrong: all 22 tests passed as first run, the whole file in under four seconds.  The smallest entries held
relatively: 3.4e-37 (D), 1.5e-22 (B, the 257-cycle), 5.7e-110 (G).

Run the file under a time limit (``timeout 300 pytest -m gpu ...``): no test loops around a failing step."""
import warnings

import numpy as np
import pytest

import diffusion_ref
import heat_steps_ref as ref

pytestmark = pytest.mark.gpu

_GRAPHS, _RUNS = {}, {}
TINY = float(np.nextafter(0.0, 1.0))     # the smallest positive float64


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


def device_graph(dcr, label):
    """One upload per unit."""
    if label not in _GRAPHS:
        u = ref.unit(label)
        _GRAPHS[label] = dcr(u['graph'], u['n'])
    return _GRAPHS[label]


def cut_call(dcr, label, k, sources=None):
    """(columns, info) of one call cut at max_terms = k over the unit's sources (or `sources`); it warns exactly when k < K."""
    u = ref.unit(label)
    src = u['sources'] if sources is None else sources
    G = device_graph(dcr, label)
    if k < u['K']:
        with pytest.warns(RuntimeWarning):
            x, info = G.heat(src, t=u['t'], max_terms=k, return_info=True)
        assert not info['converged'].any()
    else:
        with warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)
            x, info = G.heat(src, t=u['t'], max_terms=k, return_info=True)
        assert info['converged'].all()
    assert info['terms'] == k and x.dtype == np.float64 and x.shape == (len(src), u['n'])
    assert info['deficit'].dtype == np.float64 and info['deficit'].shape == (len(src),)
    return x, info


def runs(dcr, label):
    """{k: (columns, info)} over every cut of the unit, each called once."""
    if label not in _RUNS:
        _RUNS[label] = {k: cut_call(dcr, label, k) for k in ref.unit(label)['cuts']}
    return _RUNS[label]


def cut_sparse(dcr, label, cut, **kw):
    """diffusion(kernel='heat') cut at max_terms = cut over the unit's sources."""
    u = ref.unit(label)
    assert cut < u['K']
    with pytest.warns(RuntimeWarning):
        ei, w, info = device_graph(dcr, label).diffusion(kernel='heat', t=u['t'], max_terms=cut, sources=u['sources'], return_info=True, **kw)
    assert ei.dtype == np.int64 and ei.shape == (2, w.size) and w.dtype == np.float64 and info['value'].shape == w.shape
    assert info['ptr'][0] == 0 and info['ptr'][-1] == w.size and info['terms'] == cut and not info['converged'].any()
    return ei, w, info


# ---- 1. every case, every cut ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('label', ref.LABELS)
def test_every_cut_against_the_replica(dcr, label):
    u = ref.reference(label)
    got = runs(dcr, label)
    fails, worst = [], {}
    for k in u['cuts']:
        x, info = got[k]
        out = ref.compare_unit(label, k, x, info['deficit'])
        fails += out['fails']
        if 'rel' not in worst or out['rel'] / out['allow'] > worst['rel'][0] / worst['rel'][1]:
            worst['rel'] = (out['rel'], out['allow'], k)
        if 'deficit' not in worst or out['deficit'] / out['deficit_allow'] > worst['deficit'][0] / worst['deficit'][1]:
            worst['deficit'] = (out['deficit'], out['deficit_allow'], k)
    print(f'{label}: n {u["n"]}, {len(u["sources"])} sources, K {u["K"]}, {len(u["cuts"])} cuts; closest to the allowance: '
          f'|x - X| / X {worst["rel"][0]:.3e} of {worst["rel"][1]:.3e} at k = {worst["rel"][2]}; '
          f'|deficit - r rho_k| / r {worst["deficit"][0]:.3e} of {worst["deficit"][1]:.3e} at k = {worst["deficit"][2]}')
    assert not fails, '\n'.join(fails[:20])


def test_an_isolated_source_adds_up_the_thetas(dcr):
    """Case E, node 8: H_88 = 1, so x_88 after k terms is theta_0 + ... + theta_k and nothing else is written; compare holds it to
    the relative bound, this adds that the replica's entry is that sum, and that nothing crosses the components."""
    import heat_ref
    label = 'E triangle_star_isolated'
    u = ref.reference(label)
    th = heat_ref.thetas(u['t'])
    for k, (x, _) in runs(dcr, label).items():
        want = np.cumsum(th[:k + 1])[-1]
        assert abs(u['X'][k][8, 8] - want) <= 4 * (k + 1) * float(np.finfo(ref.L).eps) * want
        assert np.count_nonzero(x[8]) == 1 and np.all(x[:8, 8] == 0.0) and np.all(x[:3, 3:] == 0.0) and np.all(x[3:8, :3] == 0.0)


# ---- 2. cuts agree with themselves ----------------------------------------------------------------------------------------------------
def test_the_last_cut_is_the_uncut_call_and_company_does_not_matter(dcr):
    """Case A.  max_terms = K and no max_terms at all: the same bytes.  A column of the 44-source call (three groups of one launch,
    the last padded) and the same source alone (one group, 15 padding columns): the same bytes at k = 1 and at k = K."""
    label = 'A barbell20_4'
    u = ref.unit(label)
    got = runs(dcr, label)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        x, info = device_graph(dcr, label).heat(u['sources'], t=u['t'], return_info=True)
    assert info['terms'] == u['K'] and x.tobytes() == got[u['K']][0].tobytes() and info['deficit'].tobytes() == got[u['K']][1]['deficit'].tobytes()
    for k in (1, u['K']):
        for s in (0, 15, 16, 21, 31, 32, 43):      # first and last of each batch, a path node
            x1, i1 = cut_call(dcr, label, k, sources=[s])
            assert (x1[0].tobytes(), i1['deficit'][0].hex()) == (got[k][0][s].tobytes(), got[k][1]['deficit'][s].hex()), (k, s)


# ---- 3. the selection on cut columns: most of a column is exactly 0.0 --------------------------------------------------------------------
@pytest.mark.parametrize('label,k', [('A barbell20_4', 1), ('A barbell20_4', 2), ('E triangle_star_isolated', 1), ('E triangle_star_isolated', 2),
                                     ('F lattice33133', 1)])
def test_selection_on_cut_columns_takes_zeros_in_node_order(dcr, label, k):
    """Top-k with kk = 1, deg + 1 of a source (at k = 1 exactly its support), deg + 2 (one zero more) and n, for every degree the
    sources have: the kept set is the lexsort of the device's own cut column by (larger value, smaller id), so zeros come in id
    order; value and weight as bytes.  Threshold: eps = 0.0 keeps all n entries, the smallest positive float64 exactly the support."""
    u = ref.reference(label)
    n, src = u['n'], np.asarray(u['sources'])
    P = src.size
    x, hinfo = runs(dcr, label)[k]
    deg = ref.Gather(u['graph'], n).deg[src]
    order = np.lexsort((np.broadcast_to(np.arange(n), (P, n)), -x), axis=-1)
    for kk in sorted({1, n} | {int(d) + 1 for d in deg} | {int(d) + 2 for d in deg}):
        kk = min(kk, n)
        got_ei, w, info = cut_sparse(dcr, label, k, k=kk)
        assert info['deficit'].tobytes() == hinfo['deficit'].tobytes()
        assert np.array_equal(np.diff(info['ptr']), np.full(P, kk)), kk
        rows = got_ei[0].reshape(P, kk)
        assert np.array_equal(got_ei[1].reshape(P, kk), np.broadcast_to(src[:, None], (P, kk)))
        assert np.array_equal(rows, np.sort(order[:, :kk], axis=1)), (kk, 'kept sets')
        value = np.take_along_axis(x, rows, axis=1)
        assert info['value'].tobytes() == value.tobytes(), (kk, 'values')
        total = np.cumsum(value, axis=1)[:, -1:]           # added in id order, one after the other
        assert np.all(total > 0) and w.tobytes() == (value / total).tobytes(), (kk, 'weights')
    ball = (u['dist'] >= 0) & (u['dist'] <= k)
    for eps, keep in ((0.0, np.ones((P, n), dtype=bool)), (TINY, ball)):
        got_ei, w, info = cut_sparse(dcr, label, k, eps=eps)
        assert np.array_equal(keep, x >= eps)
        assert info['ptr'].tobytes() == np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64).tobytes(), eps
        jj, ii = np.nonzero(keep)                          # by column, then by node id
        assert np.array_equal(got_ei[0], ii) and np.array_equal(got_ei[1], src[jj]), eps
        assert info['value'].tobytes() == x[jj, ii].tobytes()
        assert w.tobytes() == np.concatenate([diffusion_ref.normalise(x[j, keep[j]]) for j in range(P)]).tobytes(), (eps, 'weights')
