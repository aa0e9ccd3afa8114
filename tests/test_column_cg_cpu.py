"""The host replica of the batched column CG (tests/column_cg_ref.py) against facts that do not depend on it, so that the step-by-step
comparison on the GPU (tests/test_column_cg_gpu.py) is a comparison with something that is itself pinned: its full solves against
the dense solutions, the distance between its float64 and its longdouble run at every (case, column, cut), which the GPU test's
allowance rests on, the margin of every freeze step the GPU test asserts, and that the shared comparison function tells a solver
with a broken recurrence from a right one (all printed: run with -s)."""
import re

import numpy as np
import pytest

import column_cg_ref as ref
import diffusion_ref
import resistance_ref
import scale_ref
import spectral_lanczos_ref

L = np.longdouble
TIGHT = 1e-17       # the tolerance of the replica's full solves below: the recurrence runs until float64 could not tell
DENSE_CASES = ('A', 'B', 'C', 'D')


# ---- host sync ------------------------------------------------------------------------------------------------------------------------
def test_the_host_looks_where_the_replica_says():
    header = ref._source('dcr_analysis.h')
    for pattern in ref.HOST_LOOKS:
        assert len(re.findall(pattern, header)) == 1, pattern
    assert ref.SP_CHECK_EVERY == spectral_lanczos_ref.SP_CHECK_EVERY >= 2
    assert ref.ORDER_FACTOR is spectral_lanczos_ref.ORDER_FACTOR
    assert ref.allow(1.0, 0.5) == ref.ORDER_FACTOR and ref.allow(0.5, 2.0) == 2 * ref.ORDER_FACTOR


def test_the_cases_are_laid_out_as_planned():
    c = scale_ref.column_and_hops_constants()
    c.update(DIF_MAX_GROUPS=scale_ref.constant(scale_ref.source('dcr_diffusion.hip'), 'DIF_MAX_GROUPS'),
             DIF_GROUP_NODES=scale_ref.constant(scale_ref.source('dcr_diffusion.hip'), 'DIF_GROUP_NODES'))
    B = c['COL_B']
    # A: 40 sources are three batches, which share every launch as three groups; node 0, the largest row, the isolated last node
    n = ref.graph('irregular330')[1]
    cols = ref.CASES['A']['columns']()
    assert len(cols) == 40 and -(-len(cols) // B) == 3 and scale_ref.diffusion_batches(n, len(cols), c)[0] == 3
    deg = ref._degrees('irregular330')
    assert cols[:3] == [0, int(np.argmax(deg)), n - 1] and deg[n - 1] == 0
    # B: a workgroup-class row, a wave-class row, a short row, a leaf of a hub, the isolated node; the rest of the batch is padding
    deg = ref._degrees('long3_mid9_short63')
    d = [int(deg[v]) for v in ref.CASES['B']['columns']()]
    assert d[0] > 2048 and 32 < d[1] <= 2048 and 1 < d[2] <= 32 and 1 <= d[3] <= d[2] and d[4] == 0 and len(d) < B
    # C: 17 pairs that take a column (one full batch and one pair beside 15 padding columns) and a same-node pair
    op = ref.operators('C')['long']
    decided = [op.host_decided(p) for p in ref.CASES['C']['columns']()]
    assert decided.count(None) == B + 1 and decided.count(0.0) == 1 and len(decided) == B + 2
    # D: six columns, one with a degree-1 endpoint, and a pair across components
    op = ref.operators('D')['long']
    pairs = ref.CASES['D']['columns']()
    decided = [op.host_decided(p) for p in pairs]
    assert decided.count(None) == 6 and decided[-1] == float('inf') and min(op.deg[list(pairs[1])]) == 1
    # E: the element-wise kernels take a second, ragged trip, and the second-trip node, the hub and the isolated node are there
    n = ref.graph('lattice')[1]
    assert n == scale_ref.RESISTANCE_SIZE and scale_ref.resistance_elementwise(n, c)[1] == 2
    deg = ref._degrees('lattice')
    hub, second, iso = ref.CASES['E-ppr']['columns']()
    assert deg[hub] > 2048 and second >= scale_ref.SECOND_TRIP and deg[second] > 0 and deg[iso] == 0
    assert tuple(ref.CASES['E-resistance']['columns']()[0]) == tuple(scale_ref.resistance_pairs()[0][2])
    assert ref._E_CUTS == [1, 2, 3, ref.SP_CHECK_EVERY + 1]
    # F: two 22-cycles, the pair opposite on the first
    ei, n = ref.graph('two_cycles22')
    assert n == 44 and ei.shape == (2, 88) and (np.bincount(ei[0], minlength=n) == 2).all()
    assert {(int(a), int(b)) for a, b in ei.T if a == 0} == {(0, 1), (0, 21)} and {int(b) for a, b in ei.T if a == 22} == {23, 43}
    assert resistance_ref.components(ei, n)[0] == 2


# ---- the replica against truth ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', DENSE_CASES)
def test_full_solves_reach_the_dense_solution(name):
    """The longdouble replica run until the recurrence's residual is below 1e-17 |rhs|, against numpy's dense solve or scipy's LU
    (PageRank) and the pseudo-inverse (resistance), within diffusion_ref.allow / resistance_ref.allow, the rounding allowances of
    those references."""
    case, op = ref.CASES[name], ref.operators(name)['long']
    ei, n = ref.graph(case['graph'])
    cols = case['columns']()
    if case['kind'] == 'ppr':
        if n <= 1024:
            want = diffusion_ref.ppr_columns(ei, n, case['alpha'], cols)
        else:
            want = diffusion_ref.lu_columns(diffusion_ref.sparse_operator(ei, n, case['alpha'])[0], cols, case['alpha'])
        worst = 0.0
        for j, w in zip(cols, want):
            run = op.solve(j, TIGHT, ref.DEFAULT_MAX_STEPS)
            assert run.reason == 'converged'
            worst = max(worst, float(np.abs(run.x(run.steps) - w).max()))
        print(f'{name}: {len(cols)} columns, largest |x - S| {worst:.3e}, allowed {diffusion_ref.allow(n):.3e}')
        assert worst <= diffusion_ref.allow(n)
        return
    dense = resistance_ref.Dense(ei, n)
    want = dense.resistance(cols)
    for pair, w in zip(cols, want):
        decided = op.host_decided(pair)
        if decided is not None:
            assert decided == w
            continue
        run = op.solve(pair, TIGHT, ref.DEFAULT_MAX_STEPS)
        resid, lower = op.closing(run.x(run.steps), pair)
        a = resistance_ref.allow(n, w)
        print(f'{name} {pair}: steps {run.steps} ({run.reason}) lower - R {float(lower) - w:.3e} (allowed {a:.3e}) residual {float(resid):.3e}')
        assert run.reason in ('converged', 'breakdown') and abs(float(lower) - w) <= a and float(resid) <= 1e-14


def test_the_barbell_agrees_with_resistance_ref():
    """resistance_ref.Dense.cg is the same iteration written once before: the float64 replica takes the same steps to the same
    lower bound."""
    ei, n = ref.graph('barbell20_4')
    dense, op = resistance_ref.Dense(ei, n), ref.operators('C')['f64']
    for pair in ref.CASES['C']['columns']():
        lower, resid, steps = dense.cg(*pair, tol=1e-10)
        if op.host_decided(pair) is not None:
            assert (lower, resid, steps) == (op.host_decided(pair), 0.0, 0)
            continue
        run = op.solve(pair, 1e-10, ref.DEFAULT_MAX_STEPS)
        mine = op.closing(run.x(run.steps), pair)
        assert run.steps == steps and abs(float(mine[1]) - lower) <= resistance_ref.allow(n, lower) and abs(float(mine[0]) - resid) <= 1e-12


def test_breakdown_counts_no_step():
    """The p.q branch on an operator that has a null space in exact small integers: rhs (1, 1) under diag(1, 0) takes one step to
    p = (0, 2), whose p.q is 0: frozen with one step counted, the iterate of that step kept."""
    run = ref.cg(lambda p: np.array([p[0], 0 * p[1]]), [1.0, 1.0], 0.0, 9, np.float64)
    assert (run.steps, run.launch, run.reason) == (1, 2, 'breakdown') and run.x(9).tolist() == [2.0, 2.0] and run.steps_at(9) == 1
    assert not run.frozen_at(1) and run.frozen_at(2)


# ---- measured distances -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ref.CASES))
def test_distances_between_the_two_precisions(name):
    """Every (case, column, cut): |float64 - longdouble| of the replica for the iterate, the residual and lower: the `measured`
    input of ref.allow.  The docstring of tests/test_column_cg_gpu.py quotes the largest per case."""
    R = ref.reference(name)
    worst = dict(x=0.0, residual=0.0, lower=0.0)
    governs = dict(x=0, residual=0, lower=0)
    for i, c in enumerate(R['columns']):
        if c.decided is not None:
            continue
        col = {q: max((c.dist[k][q] or 0.0) for k in R['cuts']) for q in worst}
        print(f'{name} column {i} {c.column}: ' + ' '.join(f'{q} {col[q]:.3e}' for q in col) +
              f'; smallest allowances x {min(c.allow[k]["x"] for k in R["cuts"]):.3e} residual {min(c.allow[k]["residual"] for k in R["cuts"]):.3e}')
        for q in worst:
            worst[q] = max(worst[q], col[q])
            governs[q] += sum(1 for k in R['cuts'] if c.allow[k][q] is not None and c.allow[k][q] == ref.ORDER_FACTOR * c.dist[k][q])
        for k in R['cuts']:
            assert all(np.isfinite(v) for v in c.allow[k].values() if v is not None)
    print(f'{name}: n {R["n"]} d_max {R["d_max"]} cuts {len(R["cuts"])} (largest {R["cuts"][-1]}); largest distances ' +
          ' '.join(f'{q} {worst[q]:.3e}' for q in worst) + f'; cuts at which the measured term governs: {governs}; {R["seconds"]:.2f} s')


def test_case_F_pins_the_cuts_below_the_cap():
    R = ref.reference('F')
    c = R['columns'][0]
    assert R['cuts'] == list(range(1, ref.F_PROBED + 1))
    below = [k for k in R['cuts'] if max(c.allow[k].values()) < ref.F_ALLOWANCE_CAP]
    print('F: allowances below the cap at k =', below, 'the largest', max(max(c.allow[k].values()) for k in below), '; |r| of the float64 recurrence', [f'{float(t):.1e}' for t in c.f64.rnorm])
    assert tuple(below) == ref.F_CUTS == tuple(R['pinned'])
    # neither precision freezes: steps == k is what the device is held to
    assert c.long.launch is None and c.f64.launch is None and c.long.steps == c.f64.steps == ref.F_PROBED


# ---- the threshold condition: a condition, not a measurement --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in ref.CASES if n != 'F'])
def test_freeze_steps_are_clear_of_the_threshold(name):
    """For every column whose freeze step f the GPU test asserts: |r_f| (1 + m) <= stop and stop (1 + m) <= |r_j| for every j < f
    (the issue asks it of j = f - 1; a dip at an earlier step would freeze the device as well), m = max(0.01, 16 ||r|_f64 - |r|_long| /
    stop) at those steps, and both precisions freeze at the same step for the same reason.  A column that fails is replaced in the
    case table."""
    R = ref.reference(name)
    for i, c in enumerate(R['columns']):
        if c.decided is not None:
            continue
        stop = L(c.stop)
        rl, r64 = c.long.rnorm, c.f64.rnorm
        assert (c.long.steps, c.long.launch, c.long.reason) == (c.f64.steps, c.f64.launch, c.f64.reason), (name, c.column)
        f = c.f
        upto = f if f is not None else c.long.steps + 1       # not frozen within the cuts: every step is a step before the freeze
        m = max([0.01] + [ref.ORDER_FACTOR * abs(float(rl[j] - L(r64[j]))) / float(stop) for j in range(upto + (f is not None))])
        before = min(float(rl[j] / stop) for j in range(upto))
        line = f'{name} column {i} {c.column}: f {f} ({c.long.reason}) m {m:.3e} min |r_j| / stop before {before:.3f}'
        assert stop * (1 + m) <= min(rl[:upto]), line
        if f is not None:
            assert c.long.reason == 'converged' and c.long.launch == f
            line += f' |r_f| / stop {float(rl[f] / stop):.3e}'
            assert rl[f] * (1 + m) <= stop, line
        print(line)


# ---- the comparison can tell a wrong solver from a right one -----------------------------------------------------------------------------------
def counted_when_frozen(name, k):
    """A device that goes on counting a frozen column's steps: the float64 replica's result with steps = k."""
    got = ref.replica_result(name, k)
    solved = [i for i, c in enumerate(ref.reference(name)['columns']) if c.decided is None]
    got['steps'][solved] = k
    return got


@pytest.mark.parametrize('name', ['A', 'C'])
def test_the_unmutated_float64_replica_passes(name):
    R = ref.reference(name)
    for k in R['pinned']:
        assert ref.compare(name, k, ref.replica_result(name, k), R) == []


@pytest.mark.parametrize('name', ['A', 'C'])
def test_mutations_are_caught(name):
    """The float64 replica with its recurrence broken on purpose, through ref.compare, the function the GPU test asserts with: each
    mutation fails at a pinned cut k >= 2, by an iterate (or lower, or the residual) beyond the allowance or by another step count.
    The old suite's acceptance rules hold for every CG iterate, so they pass all of these as long as the solve still converges.

    'counted breakdown' cannot be seen on these two cases by any cut: M is positive definite, and the barbell's columns freeze as
    converged, so the p.q branch is never entered (asserted).  ref.cg's branch is held by test_breakdown_counts_no_step, the
    mutation is shown to change its step count there, and on the device the steps == k assertions of case F are what a step
    counted in that branch would break.  What IS seen here in its place: a device that counts the steps of a frozen column."""
    R = ref.reference(name)
    cuts = [k for k in R['pinned'] if k >= 2]

    def first_catch(result):
        for k in cuts:
            fails = ref.compare(name, k, result(k), R)
            if fails:
                kinds = sorted({'steps' if ': steps ' in f else 'converged' if ': converged ' in f else 'value' for f in fails})
                return k, kinds, fails[0]
        return None, [], None

    for mutate in ref.MUTATIONS[:3]:
        k, kinds, first = first_catch(lambda k: ref.replica_result(name, k, mutate=mutate))
        if name == 'C' and mutate == 'late freeze':
            # the one pair that no cut can show: the barbell's columns terminate, |r_f| is far below stop / 16 as well, so this
            # mutant IS the right solver here (case A, whose |r_f| / stop is 0.46 .. 0.86, is where it is caught)
            assert k is None and all(c.long.rnorm[c.f] * 16 * 1000 <= c.stop for c in R['columns'] if c.decided is None)
            print(f'{name} "{mutate}": the same solver on this case: every |r_f| is below stop / 16000')
            continue
        print(f'{name} "{mutate}": first caught at k = {k} by {kinds}: {first}')
        assert k is not None, mutate
        assert ('value' if mutate in ('stale beta', 'stale gain') else 'steps') in kinds
    k, kinds, first = first_catch(lambda k: counted_when_frozen(name, k))
    print(f'{name} "steps counted for a frozen column": first caught at k = {k} by {kinds}: {first}')
    assert k is not None and kinds == ['steps']
    # 'counted breakdown': the branch is not entered on this case, in either precision, mutated or not
    runs = [c.long for c in R['columns'] if c.decided is None] + [c.f64 for c in R['columns'] if c.decided is None]
    assert all(r.reason == 'converged' for r in runs)
    for k in (2, R['f_max'], cuts[-1]):
        a, b = ref.replica_result(name, k), ref.replica_result(name, k, mutate='counted breakdown')
        assert all(np.array_equal(a[q], b[q]) for q in a)
    print(f'{name} "counted breakdown": the p.q branch is never entered on this case; see test_breakdown_mutation_changes_the_count')


def test_breakdown_mutation_changes_the_count():
    apply = lambda p: np.array([p[0], 0 * p[1]])      # noqa: E731
    base = ref.cg(apply, [1.0, 1.0], 0.0, 9, np.float64)
    mutant = ref.cg(apply, [1.0, 1.0], 0.0, 9, np.float64, mutate='counted breakdown')
    print(f'"counted breakdown": steps {mutant.steps} against {base.steps}: caught by the step count')
    assert (base.steps, mutant.steps) == (1, 2) and mutant.x(9).tolist() == base.x(9).tolist()
