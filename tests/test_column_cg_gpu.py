"""The batched column CG of csrc/dcr_analysis.h (k_col_start, k_col_matvec, k_col_update, k_col_direction, k_col_scale, col_cg_solve),
step by step, against the host replica tests/column_cg_ref.py, through the two public calls that run it.

``ppr(..., max_steps=k, return_info=True)`` returns the whole iterate x_k, the true residual of the closing mat-vec and the step
count; ``effective_resistance(..., max_steps=k, return_info=True)`` lower_k, the true residual and the step count.  In exact
arithmetic these are functions of the graph, the right-hand side and k, and the replica states them in np.longdouble.  The
acceptance rules of tests/test_resistance_gpu.py and tests/test_diffusion_gpu.py hold for EVERY CG iterate; a beta or a step length
from the wrong step's |r|^2, a column frozen late, a step counted for a frozen column or a frozen column still written pass them
as long as the solve ends below tol.  Here every cut is compared (ref.compare, the function tests/test_column_cg_cpu.py shows to
catch such solvers): steps == min(k, f) with f the replica's freeze step, which the threshold condition of the CPU test licenses
column by column (|r_f| and every earlier |r_j| at least 1 % and 16 float64-against-longdouble distances clear of the threshold);
the iterate, lower and the residual within the allowance; `converged` exactly k >= f; and the bytes of a frozen column the same
at every later cut.

The allowance rule (ref.allow, the rule of tests/spectral_lanczos_ref.py): 16 times the larger of ref.counted, a counted
first-order float64 rounding bound of k steps (the longest row's accumulation, two inner products of length n and two updates a
step, times the size of what is bounded: 1 for PageRank, |c| / lambda_1 for the resistance), and the distance between the replica's
float64 and longdouble runs at the same cut, measured on the CPU.  Nothing in it is tuned against the device.  The largest CPU
distances per case (test_column_cg_cpu.py prints them all; the counted bound is the larger of the two at every cut):
    A  irregular330, PageRank, 40 sources, cuts 1 .. 30          x 2.2e-16  residual 2.8e-17
    B  long3_mid9_short63, PageRank, 5 sources, 10 cuts          x 1.0e-15  residual 2.1e-16
    C  barbell(20, 4), resistance, 17 + 1 pairs, cuts 1 .. 10    y 3.2e-12  residual 1.0e-13  lower 1.2e-12
    D  irregular330, resistance, 6 + 1 pairs, cuts 1 .. 24       y 4.4e-16  residual 6.3e-17  lower 8.4e-16
    E  33,133 nodes, cuts 1, 2, 3, 9: PageRank, 3 sources        x 4.8e-16  residual 4.7e-17
                                      resistance, 1 pair         y 1.6e-15  residual 1.7e-16  lower 6.2e-16
    F  two 22-cycles, tol = 0, pair (0, 11), cuts 1 .. 17        y 1.3e-14  residual 3.0e-15  lower 2.0e-14
On A every column but the isolated nodes' freezes after 22 steps (the isolated after 1), so the three groups of the 40-source call
go quiet in the same step: what differs between them is the padding of the last.

Run the file under a time limit (``timeout 300 pytest -m gpu ...``): no test loops around a failing step."""
import warnings

import numpy as np
import pytest

import column_cg_ref as ref
import scale_ref

pytestmark = pytest.mark.gpu

_GRAPHS, _RUNS = {}, {}


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


@pytest.fixture(scope='module')
def lattice_references():
    """The sparse longdouble replica of the two cases at 33,133 nodes, computed once."""
    out = {name: ref.reference(name) for name in ('E-ppr', 'E-resistance')}
    print('  replica of case E on the CPU: ' + ', '.join(f'{name} {r["seconds"]:.2f} s' for name, r in out.items()))
    return out


def device_graph(dcr, key):
    """One upload per graph."""
    if key not in _GRAPHS:
        ei, n = ref.graph(key)
        _GRAPHS[key] = dcr(ei, n)
    return _GRAPHS[key]


def call(dcr, name, k, columns=None, unconverged=None):
    """One call cut at max_steps = k over all columns of the case (or `columns`), in the layout ref.compare takes.  It must warn
    exactly when the replica says that a column has not converged by then."""
    R = ref.reference(name)
    case = R['case']
    G = device_graph(dcr, case['graph'])
    cols = ref.columns_array(name) if columns is None else columns
    if unconverged is None:
        unconverged = any(c.decided is None and not ref.expect_converged(c, k) for c in R['columns'])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        if case['kind'] == 'ppr':
            x, info = G.ppr(cols, alpha=case['alpha'], tol=case['tol'], max_steps=k, return_info=True)
            got = dict(x=x)
        else:
            lower, info = G.effective_resistance(cols, tol=case['tol'], max_steps=k, return_info=True)
            got = dict(lower=lower)
    warned = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    assert bool(warned) == unconverged, (name, k, [str(w.message) for w in warned])
    got.update(residual=info['residual'], steps=info['steps'], converged=info['converged'])
    assert got['residual'].dtype == np.float64 and got['steps'].dtype == np.int32
    return got


def runs(dcr, name):
    """{k: result} over every cut of the case, each called once."""
    if name not in _RUNS:
        _RUNS[name] = {k: call(dcr, name, k) for k in ref.reference(name)['cuts'] if k in ref.reference(name)['pinned']}
    return _RUNS[name]


def column_bytes(got, i):
    value = got['x'][i].tobytes() if 'x' in got else float(got['lower'][i]).hex()
    return value, float(got['residual'][i]).hex(), int(got['steps'][i]), bool(got['converged'][i])


def test_the_batch_width_is_the_header_s(dcr):
    import dcr.graph as graph
    assert graph.RESISTANCE_BATCH == graph.DIFFUSION_BATCH == scale_ref.column_and_hops_constants()['COL_B']


# ---- 1. every case, every cut ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ref.CASES))
def test_every_cut_against_the_replica(dcr, name, lattice_references):
    """A: three groups in one launch, columns that freeze at steps 1 and 22, cuts through the window after the freeze.  B: a
    workgroup-class row, a wave-class row, a short row, a leaf and an isolated node beside 11 padding columns, around both looks of
    the host and the full solve.  C: finite termination, a same-node pair, a second batch of one pair.  D: a degree-1 endpoint, a
    pair across components.  E: the element-wise kernels' second, ragged grid-stride trip and 1,024 partials.  F: tol = 0, steps == k."""
    R = ref.reference(name)
    got = runs(dcr, name)
    fails, worst = [], {}
    for k in R['pinned']:
        fails += ref.compare(name, k, got[k], R)
        for i, c in enumerate(R['columns']):
            if c.decided is not None:
                continue
            d = dict(residual=abs(float(ref.L(got[k]['residual'][i]) - c.want[k]['residual'])))
            if 'x' in got[k]:
                d['x'] = float(np.abs(got[k]['x'][i].astype(ref.L) - c.want[k]['x']).max())
            else:
                d['lower'] = abs(float(ref.L(got[k]['lower'][i]) - c.want[k]['lower']))
            for q, dist in d.items():
                if q not in worst or dist / c.allow[k][q] > worst[q][0] / worst[q][1]:
                    worst[q] = (dist, c.allow[k][q], k, i)
    solved = [i for i, c in enumerate(R['columns']) if c.decided is None]
    last = R['pinned'][-1]
    print(f'{name}: {len(R["pinned"])} cuts, {len(solved)} columns; steps at the last cut {sorted(set(int(got[last]["steps"][i]) for i in solved))} '
          f'(replica {sorted(set(R["columns"][i].want[last]["steps"] for i in solved))})')
    for q, (dist, a, k, i) in worst.items():
        print(f'    closest to its allowance: |d {q}| {dist:.3e} of {a:.3e} at k = {k}, column {i}')
    assert not fails, '\n'.join(fails[:20])


# ---- 2. a frozen column is no longer written -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['A', 'B', 'C', 'E-ppr'])
def test_frozen_columns_stay_frozen(dcr, name, lattice_references):
    """For k > f a column's bytes are those of the call with max_steps = f: in the same window of SP_CHECK_EVERY steps, where the
    launches go on after every column of the group has frozen until the host looks, and in the next one."""
    R = ref.reference(name)
    got = runs(dcr, name)
    compared = same_window = next_window = 0
    for i, c in enumerate(R['columns']):
        if c.decided is not None or c.f is None:
            continue
        assert c.f in got, (name, c.column, c.f)
        want = column_bytes(got[c.f], i)
        for k in R['pinned']:
            if k > c.f:
                assert column_bytes(got[k], i) == want, (name, c.column, c.f, k)
                compared += 1
                window = -(-c.f // ref.SP_CHECK_EVERY) * ref.SP_CHECK_EVERY
                same_window += k <= window
                next_window += k > window
    print(f'{name}: {compared} comparisons, {same_window} within the window of the freeze, {next_window} past it')
    assert compared and next_window
    if name in ('A', 'C'):
        assert same_window


def test_a_column_alone_and_among_forty(dcr):
    """Node 0 of case A: the same bytes in a call of its own (one group, 15 padding columns) and as column 0 of the 40-source call
    (three groups), at k = f - 1, f and f + 1."""
    R = ref.reference('A')
    c = R['columns'][0]
    assert c.column == 0 and c.f >= 2
    got = runs(dcr, 'A')
    for k in (c.f - 1, c.f, c.f + 1):
        alone = call(dcr, 'A', k, columns=np.array([0], dtype=np.int32), unconverged=k < c.f)
        assert column_bytes(alone, 0) == column_bytes(got[k], 0), k
