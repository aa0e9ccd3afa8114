"""The host replica of the heat kernel's recurrence (tests/heat_steps_ref.py) against facts that do not depend on it, so that the
term-by-term comparison on the GPU (tests/test_heat_steps_gpu.py) is a comparison with something that is itself pinned: the
one-run partial sums against heat_ref.taylor_long bit for bit, the cases laid out as planned, the float64 replica in the device's
operation order inside the derived relative allowance at every cut of every case (the ratios are printed: run with -s; the
docstring of the GPU file quotes them), six mutations of that replica shown to be caught by the shared comparison function or shown
to be invisible at a case for a stated reason, and what the acceptance rule of tests/test_heat_gpu.py says to two of them."""
import contextlib
import io

import numpy as np
import pytest

import heat_ref
import heat_steps_ref as ref
import scale_ref

L = np.longdouble
_RUNS = {}


def replica(label, mutate=None):
    """({k: x}, {k: deficit}) of the float64 replica at the unit's cuts, 'm5' and 'm6' applied to the finished columns of the
    unmutated run (the deficit is then that of the spoiled column, as k_heat_mass would add it up), and {k: entries spoiled}."""
    if (label, mutate) not in _RUNS:
        u = ref.reference(label)
        if mutate in ('m5', 'm6'):
            xs, _, _ = replica(label)
            deg = ref.Gather(u['graph'], u['n']).deg
            spoiled = {k: ref.spoil(x, mutate, (u['dist'] >= 0) & (u['dist'] <= k)) for k, x in xs.items()}
            _RUNS[label, mutate] = ({k: s[0] for k, s in spoiled.items()}, {k: ref.deficit_f64(s[0], deg, u['sources']) for k, s in spoiled.items()},
                                    {k: s[1] for k, s in spoiled.items()})
        else:
            _RUNS[label, mutate] = ref.partial_sums_f64(u['graph'], u['n'], u['t'], u['sources'], u['cuts'], mutate=mutate) + (None,)
    return _RUNS[label, mutate]


# ---- the replica against itself and the cases against the plan ------------------------------------------------------------------------------
def test_one_run_returns_what_taylor_long_returns_cut_by_cut():
    ei, n = heat_ref.graphs()['barbell20_4']
    K = heat_ref.terms(5.0, heat_ref.TOL)
    src = [0, 21, 43]
    X = ref.partial_sums(ei, n, 5.0, src, [0, 1, 3, K, K + heat_ref.ORACLE_EXTRA])
    for k in X:
        assert X[k].dtype == L and np.array_equal(X[k], heat_ref.taylor_long(ei, n, 5.0, src, k)), k    # == on every entry: a longdouble has padding bytes


def test_the_cases_are_laid_out_as_planned():
    c = scale_ref.column_and_hops_constants()
    c.update(DIF_MAX_GROUPS=scale_ref.constant(scale_ref.source('dcr_diffusion.hip'), 'DIF_MAX_GROUPS'),
             DIF_GROUP_NODES=scale_ref.constant(scale_ref.source('dcr_diffusion.hip'), 'DIF_GROUP_NODES'))
    B = c['COL_B']
    assert [len(ref.labels(case)) for case in 'ABCDEFG'] == [1, 8, 2, 1, 1, 1, 1] and sum(len(ref.labels(case)) for case in 'ABCDEFG') == len(ref.LABELS)
    for label in ref.LABELS:
        u = ref.unit(label)
        # every cut below K leaves more than tol of the mass out, so the call reports no column as converged and warns; the call
        # at K has its tail within tol / 2.  (At t = 20 and t = 256 the cut K - 1 would already be within tol: it is in no list.)
        assert all(heat_ref.tail(u['t'], k) >= 1.5 * heat_ref.TOL for k in u['cuts'][:-1]), label
        assert heat_ref.tail(u['t'], u['K']) <= heat_ref.TOL / 2 and u['cuts'][-1] == u['K'] == heat_ref.terms(u['t'], heat_ref.TOL)
    u = ref.unit('A barbell20_4')    # 44 sources: two full batches and one of 12 beside padding, three groups of one launch; both parities of every cut
    assert len(u['sources']) == 44 == u['n'] and 44 % B and scale_ref.diffusion_batches(44, 44, c)[0] == 3 and u['cuts'] == list(range(1, 26))
    for label in ref.labels('B'):    # a source of every row class the graph has
        u = ref.unit(label)
        deg = ref.Gather(u['graph'], u['n']).deg
        classes = {0 if d > ref.LONG_DEG else 2 if d <= ref.SHORT_DEG else 1 for d in deg}
        assert {0 if d > ref.LONG_DEG else 2 if d <= ref.SHORT_DEG else 1 for d in deg[u['sources']]} == classes, label
        assert u['cuts'] == [1, 2, 3, 24, 25]
    for label in ref.labels('C'):    # the row of 2,100 slots, a leaf beside it and the end of the tail, five hops from the other leaves
        u = ref.reference(label)
        assert ref.Gather(u['graph'], u['n']).deg[0] == 2100 and u['sources'][:2] == [0, 1] and u['dist'][u['sources'].index(2103)].max() == 5
    u = ref.reference('D path300')   # the ball grows by one node a term from an end, by two from the middle
    assert [int(((u['dist'][0] >= 0) & (u['dist'][0] <= k)).sum()) for k in u['cuts']] == [k + 1 for k in u['cuts']]
    assert [int((u['dist'][1] <= k).sum()) for k in u['cuts']] == [2 * k + 1 for k in u['cuts']]
    assert float(u['X'][u['K']][u['X'][u['K']] > 0].min()) < 1e-36
    u = ref.unit('E triangle_star_isolated')
    assert u['sources'] == list(range(9)) and u['cuts'] == list(range(1, 11))
    u = ref.unit('F lattice33133')   # the element-wise kernels' second trip; 17 sources are two launches of one group
    groups, _, trips = scale_ref.diffusion_batches(u['n'], len(u['sources']), c)
    assert u['n'] == 33133 and (groups, trips) == (1, 2) and len(u['sources']) == B + 1 and u['cuts'] == [1, 2, 3, 25]
    u = ref.reference('G path8 t 256')
    assert u['K'] == 366 and 6e-112 < np.exp(-L(256)) < 7e-112 and 1e-110 < float(u['X'][1][u['X'][1] > 0].min()) < 1e-109


# ---- the float64 replica inside the derived allowance --------------------------------------------------------------------------------------
@pytest.mark.parametrize('label', ref.LABELS)
def test_the_float64_replica_is_inside_the_relative_allowance(label):
    """Every cut of every case: the device's arithmetic restated in float64 against the longdouble run, through the comparison
    function the GPU test asserts with.  The largest |x - X| / (a X) says how much room the derived bound has."""
    u = ref.reference(label)
    xs, ds, _ = replica(label)
    worst = dict(ratio=0.0, rel=0.0, deficit=0.0)
    for k in u['cuts']:
        out = ref.compare_unit(label, k, xs[k], ds[k])
        assert out['fails'] == [], out['fails'][:5]
        for q in worst:
            worst[q] = max(worst[q], out[q])
        last = out
    smallest = min(float(u['X'][k][u['X'][k] > 0].min()) for k in u['cuts'])
    print(f'{label}: n {u["n"]}, {len(u["sources"])} sources, K {u["K"]}, {len(u["cuts"])} cuts; largest |x - X| / (a X) {worst["ratio"]:.4f}, '
          f'largest |x - X| / X {worst["rel"]:.3e} (a at K {last["allow"]:.3e}), largest deficit distance / r {worst["deficit"]:.3e} '
          f'(allowed at K {last["deficit_allow"]:.3e}), smallest positive X {smallest:.3e}')
    assert worst['ratio'] <= 0.5      # the factor of two heat_ref.allow says it keeps in hand


# ---- the comparison can tell a wrong recurrence from a right one ---------------------------------------------------------------------------
def verdicts(label, mutate):
    """{k: (lines of compare, whether a byte of x differs from the unmutated replica's)}"""
    u = ref.reference(label)
    xs, ds, _ = replica(label, mutate)
    base, _, _ = replica(label)
    return {k: (ref.compare_unit(label, k, xs[k], ds[k])['fails'], xs[k].tobytes() != base[k].tobytes()) for k in u['cuts']}


@pytest.mark.parametrize('label', ref.labels('A', 'B'))
def test_mutations_are_caught(label):
    """m1 .. m6 of ref.partial_sums_f64 and ref.spoil through ref.compare.  Where a mutation cannot be seen at a case, that is
    asserted with its reason: the mutant is then byte for byte the right solver there."""
    u = ref.reference(label)
    deg = ref.Gather(u['graph'], u['n']).deg
    has_long = bool((deg > ref.LONG_DEG).any())
    assert has_long == (label in ('B long3_mid9_short63', 'B long1_mid0_short0'))
    for mutate in ('m1', 'm2'):
        # the first term reads z_0 with c = t / 1 either way: cut 1 cannot see them, cut 2 must
        v = verdicts(label, mutate)
        caught = [k for k in u['cuts'] if v[k][0]]
        print(f'{label} {mutate}: caught at k = {caught}: {v[2][0][0]}')
        assert v[1] == ([], False) and caught == u['cuts'][1:], (mutate, caught)
    for mutate in ('m3', 'm4'):
        v = verdicts(label, mutate)
        caught = [k for k in u['cuts'] if v[k][0]]
        if not has_long:
            # no row above 2,048 slots: the workgroup class is not entered, the mutant is the right solver
            assert not caught and not any(differs for _, differs in v.values())
            print(f'{label} {mutate}: no row above {ref.LONG_DEG} slots (largest {int(deg.max())}): the same bytes at every cut')
            continue
        print(f'{label} {mutate}: caught at k = {caught}: {v[caught[0]][0][0]}')
        # a long row is a source.  m3: its own entry lacks theta_1 H_jj from the first term on.  m4: the first term gathers one
        # non-zero entry a row, the source's, and no source sits in a long row's slots from 1,536 on: the second term is the first
        # that reads a slot left out
        assert caught == (u['cuts'] if mutate == 'm3' else u['cuts'][1:]), (mutate, caught)
    for mutate in ('m5', 'm6'):
        v = verdicts(label, mutate)
        spoiled = replica(label, mutate)[2]
        caught = [k for k in u['cuts'] if v[k][0]]
        assert caught == [k for k in u['cuts'] if spoiled[k] > 0], (mutate, caught)      # caught wherever there was an entry to spoil
        assert all(v[k][1] == (spoiled[k] > 0) for k in u['cuts'])
        print(f'{label} {mutate}: entries spoiled per cut {[spoiled[k] for k in u["cuts"]]}, caught at k = {caught}' +
              (f': {v[caught[0]][0][0]}' if caught else ''))
        if mutate == 'm5':
            # an entry outside the ball exists until the ball is the source's component: up to k = 6 on the barbell, whose
            # diameter is 7, at no cut on the complete graph, at every cut where there is an isolated node or a 257-cycle
            if label == 'A barbell20_4':
                assert caught == [1, 2, 3, 4, 5, 6]
            assert (caught == []) == (label == 'B mid34_short0') and (1 in caught or label == 'B mid34_short0')
        else:
            # entries below 1e-12 need a long way at t = 5: the smallest positive entry of any cut is above it (asserted) on every
            # graph here but the 257-cycle, where theta_25 / 3^25 is 1.5e-22
            smallest = min(float(u['X'][k][u['X'][k] > 0].min()) for k in u['cuts'])
            assert bool(caught) == (smallest < ref.M6_BELOW) == (label == 'B mid0_short257'), (label, smallest)


# ---- what the old rule accepted -------------------------------------------------------------------------------------------------------------
def old_rule_accepts(label, mutate):
    """The converged column (cut K) of the mutated float64 replica through `accept`, the rule of tests/test_heat_gpu.py, against the
    oracle that file uses: the longdouble recurrence with 40 terms more."""
    u = ref.reference(label)
    xs, ds, _ = replica(label, mutate)
    K = u['K']
    want = heat_ref.taylor_long(u['graph'], u['n'], u['t'], u['sources'], K + heat_ref.ORACLE_EXTRA)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ref.accept(xs[K], dict(terms=K, deficit=ds[K]), want, heat_ref.tail(u['t'], K + heat_ref.ORACLE_EXTRA), u['graph'], u['n'],
                       u['sources'], u['t'], label)
    except AssertionError as e:
        return False, str(e)
    return True, ''


def test_what_the_old_rule_says_to_m4_and_m6():
    """The statement of the gap: `accept` takes the unmutated replica, takes m6 (a relative error of 1e-3 on every entry below
    1e-12: far inside its absolute allowance), and rejects m4 on these two graphs by its second deficit statement: a long row is a
    source here and the slots from 1,536 on are a quarter of its row, so the column's total mass is off by far more than the
    allowance.  That statement pins the total alone; where the lost share is small against the column's mass it says nothing,
    and the entries are held by no more than m6's are.  The new rule rejects both (test_mutations_are_caught)."""
    seen = {}
    for label, mutate in (('B mid0_short257', None), ('B long3_mid9_short63', None), ('D path300', None),
                          ('B mid0_short257', 'm6'), ('D path300', 'm6'), ('B long3_mid9_short63', 'm4'), ('B long1_mid0_short0', 'm4')):
        seen[label, mutate] = old_rule_accepts(label, mutate)
        print(f'old rule, {label}, {mutate or "unmutated"}: {"accepts" if seen[label, mutate][0] else "rejects: " + seen[label, mutate][1][:160]}')
    assert all(seen[key][0] for key in seen if key[1] is None)
    spoiled = {label: replica(label, 'm6')[2][ref.unit(label)['K']] for label in ('B mid0_short257', 'D path300')}
    assert min(spoiled.values()) >= 30 and seen['B mid0_short257', 'm6'][0] and seen['D path300', 'm6'][0]
    assert not seen['B long3_mid9_short63', 'm4'][0] and not seen['B long1_mid0_short0', 'm4'][0]
