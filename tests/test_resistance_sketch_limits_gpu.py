"""The resistance sketch (csrc/dcr_resistance_sketch.hip) past its group, grid and long-row limits: launches of 1, 2, 3 and 4 groups
and their tails, k_sketch_pairs past one workgroup and past SKT_PAIR_BLOCKS, a row above SP_LONG_DEG whose slots all hold different
reference values, node ids of 2^16 and above in the Philox key, and an edit that relocates the long row between two calls.  The
sizes are those tests/test_scale_thresholds_cpu.py asserts from the sources; the references are those of
tests/resistance_sketch_ref.py that do not grow with n^2 (a grounded sparse LU, and the closed form of the windmill), computed once.

Every solve runs at tol 1e-12 and must report `converged`.  The acceptance rule is that of tests/test_resistance_sketch_gpu.py with
lambda_1 replaced by the certified lam_lo of resistance_ref.lambda1_lower, the reference's own error e_a added and the rounding
allowance measured at scale (SCALE_ROUNDING_ALLOW, which is zero: see resistance_sketch_ref):

    |R~ - R~_ref| <= 1/k sum_j (2 |a_j| eps_j sqrt(R~_ref) + eps_j^2 R~_ref) + 1/k sum_j (2 |a_j| e_a + e_a^2) + SCALE_ROUNDING_ALLOW max(1, R~_ref)

with eps_j = rho_j / sqrt(lam_lo), rho_j the residuals the call returns.  The two graphs of at most 300 nodes keep pinv as reference
and ROUNDING_ALLOW as rounding term, with lam_lo in eps_j."""
import warnings

import numpy as np
import pytest

import resistance_ref as ref
import resistance_sketch_ref as skref
import scale_ref as sc

pytestmark = pytest.mark.gpu

TOL = 1e-12
BIG_SEED = 0x9E3779B97F4A7C15
WORST = {'ratio': 0.0, 'label': ''}   # the largest gap / bound seen in this run, printed after every comparison


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


@pytest.fixture(scope='module')
def c():
    return sc.constants()


@pytest.fixture(scope='module')
def three(dcr):
    """sketch_three_groups on the device, for the tests that do not edit it."""
    case = skref.large_case('sketch_three_groups')
    return case, dcr(case.ei, case.n)


def sketch(G, k, **kw):
    """resistance_sketch at tol 1e-12 that must converge: ((eu, ev, R) or None, pair values or None, info)."""
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        out = G.resistance_sketch(columns=k, tol=TOL, return_info=True, **kw)
    out = out if isinstance(out, tuple) and isinstance(out[-1], dict) else (out,)
    info = out[-1]
    assert info['columns'] == k and info['batches'] == -(-k // 16) and info['converged'].all() and info['residual'].shape == (k,)
    assert np.isfinite(info['residual']).all() and info['residual_max'] == info['residual'].max()
    edges = out[0] if kw.get('edges', True) else None
    pairs = None if kw.get('pairs') is None else out[-2]
    return edges, pairs, info


def accept(got, a, bound, label):
    """got [P] against the reference differences a [k, P] under bound [P]; returns the largest gap / bound."""
    want = (a ** 2).mean(axis=0)
    gap = np.abs(got - want)
    ratio = float((gap / bound).max())
    if ratio > WORST['ratio']:
        WORST.update(ratio=ratio, label=label)
    print(f'  {label}: {len(got)} values, max |R~ - R~_ref| = {gap.max():.3e}, bound there {bound[gap.argmax()]:.3e}, smallest bound '
          f'{bound.min():.3e}, max gap / bound {ratio:.3e} (largest so far {WORST["ratio"]:.3e}, {WORST["label"]})')
    assert np.isfinite(got).all() and np.all(gap <= bound), (label, np.flatnonzero(~(gap <= bound))[:5], gap.max())
    return ratio


def edge_columns(case, eu, ev):
    """The column of case.e (and of case.a) for every edge of G.edges(), each edge exactly once."""
    lo, hi = np.minimum(eu, ev).astype(np.int64), np.maximum(eu, ev).astype(np.int64)
    keys = case.e[:, 0] * case.n + case.e[:, 1]
    at = np.searchsorted(keys, lo * case.n + hi)
    assert len(at) == len(keys) and np.array_equal(np.sort(at), np.arange(len(keys))) and np.array_equal(keys[at], lo * case.n + hi)
    return at


def check_case(case, G, k, env_label=''):
    """All edges in G.edges() order and pairs_of(n) of one call against the case's reference; returns (R, Rp, info, the column of
    case.a per edge, the bound per column of case.a)."""
    assert k == case.k
    pairs = skref.pairs_of(case.n)
    (eu, ev, R), Rp, info = sketch(G, k, seed=case.seed, pairs=pairs)
    geu, gev = G.edges()
    assert np.array_equal(eu, geu) and np.array_equal(ev, gev) and R.shape == eu.shape
    at = edge_columns(case, eu, ev)
    bound = case.bound(info['residual']) + skref.SCALE_ROUNDING_ALLOW * np.maximum(1.0, (case.a ** 2).mean(axis=0))
    accept(R, case.a[:, at], bound[at], f'{case.name}{env_label} k = {k}, edges')
    solved = case.solved[len(case.e):]
    cols = (np.cumsum(case.solved) - 1)[len(case.e):][solved]
    same, across = pairs[:, 0] == pairs[:, 1], case.labels[pairs[:, 0]] != case.labels[pairs[:, 1]]
    assert np.all(Rp[same] == 0.0) and not np.signbit(Rp[same]).any() and np.all(np.isposinf(Rp[across & ~same]))
    assert np.array_equal(solved, ~same & ~across) and solved.sum() >= 10
    accept(Rp[solved], case.a[:, cols], bound[cols], f'{case.name}{env_label} k = {k}, pairs')
    return R, Rp, info, at, bound


# ---- a. every edge and the pairs at each group count -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(sc.SKETCH_LARGE))
def test_every_edge_and_pairs_at_three_two_and_one_groups(dcr, c, three, name):
    case = skref.large_case(name)
    _, k, launches = sc.SKETCH_LARGE[name]
    assert sc.sketch_launches(case.n, k, c) == launches
    G = three[1] if name == 'sketch_three_groups' else dcr(case.ei, case.n)
    R, _, info, at, bound = check_case(case, G, k)
    assert info['batches'] == sum(launches)
    hub = np.isin(at, case.hub_edges)
    assert hub.sum() == 2100 > c['SP_LONG_DEG']                          # the long row's edges are among the compared values
    want = (case.a[:, at[hub]] ** 2).mean(axis=0)
    gap, largest = np.diff(np.sort(want)).min(), bound[at[hub]].max()
    print(f'  {name}: long row: values at least {gap:.3e} apart, largest bound {largest:.3e} (with the device residuals), ratio {gap / largest:.1f}')
    # so one of these values under another of these edges would have failed above.  The hub's id is above its neighbours' here, so
    # these sums are made in the neighbours' short rows and the long row is walked without a write; the row that writes its own
    # slots is the windmill's (test_windmill_against_its_closed_form) and the edited hub's one slot to the joined node.
    assert gap > 100.0 * largest and len(case.hub_kept) == 0


@pytest.mark.parametrize('k', list(sc.SKETCH_SMALL_COLUMNS))
@pytest.mark.parametrize('name', ['random300', 'barbell_20_4'])
def test_three_groups_alone_and_four_then_three(dcr, c, name, k):
    ei, n = skref.GENERAL[name]()
    assert sc.sketch_launches(n, k, c) == sc.SKETCH_SMALL_COLUMNS[k]
    d = ref.Dense(ei, n)
    lam_lo = ref.lambda1_lower(ei, n, 0)[0]
    G = dcr(ei, n)
    pairs = skref.pairs_of(n)
    (eu, ev, R), Rp, info = sketch(G, k, pairs=pairs)
    want = skref.Sketch(ei, n, k, seed=0, dense=d)
    e = np.stack([np.minimum(eu, ev), np.maximum(eu, ev)], axis=1).astype(np.int64)
    assert np.array_equal(e[np.lexsort((e[:, 1], e[:, 0]))], want.edges)
    solved = pairs[:, 0] != pairs[:, 1]
    assert np.all(Rp[~solved] == 0.0) and not np.signbit(Rp[~solved]).any()
    for got, pr, what in ((R, e, 'edges'), (Rp[solved], pairs[solved], 'pairs')):
        a = want.diffs(pr)
        accept(got, a, skref.residual_bound(a, info['residual'], lam_lo) + skref.allow((a ** 2).mean(axis=0)), f'{name} k = {k}, {what}')


# ---- b. a column's solve does not depend on its neighbours ---------------------------------------------------------------------------
def test_first_batch_alone_and_in_a_launch_of_three(three, c, monkeypatch):
    """dcr_sketch_info carries the steps of a call in one total, not per batch; the first batch's own steps are the k = 16 call's
    total, and a column whose step count changed could not keep the bits of its residual.  The totals of the k = 80 call are held
    against the same call with one group a launch."""
    case, G = three
    assert sc.sketch_launches(case.n, 80, c) == [3, 2] and sc.sketch_launches(case.n, 16, c) == [1]
    _, _, i80 = sketch(G, 80, seed=case.seed)
    _, _, i16 = sketch(G, 16, seed=case.seed)
    assert i16['residual'].tobytes() == i80['residual'][:16].tobytes()
    assert 0 < i16['steps_total'] < i80['steps_total']
    monkeypatch.setenv('DCR_SKETCH_GROUPS', '1')
    (_, _, R1), _, one = sketch(G, 80, seed=case.seed)
    assert one['residual'].tobytes() == i80['residual'].tobytes() and one['steps_total'] == i80['steps_total']
    _, _, one16 = sketch(G, 16, seed=case.seed)
    assert one16['steps_total'] == i16['steps_total'] and one16['residual'].tobytes() == i16['residual'].tobytes()


def test_group_cap_of_one_to_four_on_random300(dcr, c, monkeypatch):
    ei, n = skref.GENERAL['random300']()
    d = ref.Dense(ei, n)
    lam_lo = ref.lambda1_lower(ei, n, 0)[0]
    G = dcr(ei, n)
    k = 112
    want = skref.Sketch(ei, n, k, seed=0, dense=d)
    runs = []
    for cap in (1, 2, 3, 4):
        monkeypatch.setenv('DCR_SKETCH_GROUPS', str(cap))
        (eu, ev, R), _, info = sketch(G, k)
        e = np.stack([np.minimum(eu, ev), np.maximum(eu, ev)], axis=1).astype(np.int64)
        a = want.diffs(e)
        accept(R, a, skref.residual_bound(a, info['residual'], lam_lo) + skref.allow((a ** 2).mean(axis=0)),
               f'random300, launches of {sc.sketch_launches(n, k, c, cap)}, k = {k}, edges')
        runs.append((info['residual'].tobytes(), info['steps_total'], R))
    assert all(r[0] == runs[0][0] and r[1] == runs[0][1] for r in runs)    # residuals and steps: the same bytes
    print(f'  values across the caps differ by at most {max(np.abs(r[2] - runs[0][2]).max() for r in runs):.3e}')


# ---- c. pairs past the cap of k_sketch_pairs -----------------------------------------------------------------------------------------
def test_pairs_past_the_grid_cap(three, c):
    case, G = three
    names = sc.sketch_three_groups()[2]
    pairs, marks = sc.sketch_pairs_past_cap(case.n, names, c, 130)
    assert sc.sketch_pair_grid(len(pairs), c)[1] == 2
    k = case.k
    none, Rp, info = sketch(G, k, seed=case.seed, pairs=pairs, edges=False)
    assert none is None and Rp.shape == (len(pairs),)
    same, across = pairs[:, 0] == pairs[:, 1], case.labels[pairs[:, 0]] != case.labels[pairs[:, 1]]
    assert np.all(Rp[same] == 0.0) and not np.signbit(Rp[same]).any()     # +0.0 wherever it sits
    assert np.all(np.isposinf(Rp[across & ~same])) and (across & ~same).sum() == 4
    for key in ('same', 'isolated', 'isolated_last'):
        assert all((same | across)[i] for i in marks[key])
    finite = ~same & ~across
    assert np.isfinite(Rp[finite]).all() and finite.sum() > len(pairs) - 10
    a, e_a = case.diffs(pairs[finite])
    print(f'  e_a over {finite.sum()} pairs: {e_a:.3e}')
    bound = case.bound(info['residual'], a, e_a) + skref.SCALE_ROUNDING_ALLOW * np.maximum(1.0, (a ** 2).mean(axis=0))
    accept(Rp[finite], a, bound, f'{case.name} k = {k}, {len(pairs)} pairs in two trips')
    f0, f1, f2 = marks['fixed']
    _, alone, _ = sketch(G, k, seed=case.seed, pairs=np.array([marks['pair']]), edges=False)
    assert Rp[f2].tobytes() == alone[0].tobytes() == Rp[f0].tobytes() == Rp[f1].tobytes() and np.isfinite(alone[0]) and alone[0] > 0.0
    _, again, info2 = sketch(G, k, seed=case.seed, pairs=pairs, edges=False)
    assert again.tobytes() == Rp.tobytes() and info2['residual'].tobytes() == info['residual'].tobytes()


# ---- d. the closed form ------------------------------------------------------------------------------------------------------------
def test_windmill_against_its_closed_form(dcr, c):
    case = skref.large_case('windmill')
    assert case.e_a == 0.0 and sc.sketch_launches(case.n, case.k, c) == [4, 3]
    G = dcr(case.ei, case.n)
    R, _, info, at, bound = check_case(case, G, case.k)
    hub = np.isin(at, case.hub_edges)
    assert hub.sum() == len(case.hub_edges) > c['SP_LONG_DEG']
    want = (case.a[:, at[hub]] ** 2).mean(axis=0)
    distinct = skref.distinct_values(want, 100.0 * bound[at[hub]].max())
    kept = np.isin(at, case.hub_kept)                                    # the slots the long row sums itself: the centre is the smaller id
    own = skref.distinct_values((case.a[:, at[kept]] ** 2).mean(axis=0), 100.0 * bound[at[hub]].max())
    print(f'  windmill: {hub.sum()} slots in the long centre row, {distinct} reference values more than 100 bounds apart; {kept.sum()} slots '
          f'summed by the row itself, {own} such values among them')
    assert distinct >= 1000 and kept.sum() > c['SP_LONG_DEG'] and own >= 1000
    # 200 pairs: across blades of the first centre, and across the bridge
    first = np.concatenate([nodes[:, 1:].ravel() for _, nodes in case.parts[1:1 + len(skref.WINDMILL_LONG)]])
    second = np.concatenate([nodes[:, 1:].ravel() for _, nodes in case.parts[1 + len(skref.WINDMILL_LONG):]])
    rng = np.random.default_rng(8)
    pairs = np.concatenate([rng.choice(first, size=(100, 2), replace=False), np.stack([rng.choice(first, 100), rng.choice(second, 100)], axis=1)])
    _, Rp, info = sketch(G, case.k, seed=case.seed, pairs=pairs, edges=False)
    a, _ = case.diffs(pairs)
    accept(Rp, a, case.bound(info['residual'], a, 0.0) + skref.SCALE_ROUNDING_ALLOW * np.maximum(1.0, (a ** 2).mean(axis=0)),
           f'windmill k = {case.k}, 200 pairs across blades and across the bridge')


# ---- e. right-hand sides by == where ids and offsets are large --------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['whole_small', 'sketch_two_groups'])
def test_rhs_with_large_ids_and_offsets(dcr, name):
    ei, n = sc.whole_small() if name == 'whole_small' else sc.sketch_two_groups()[:2]
    assert name != 'whole_small' or n > 2 ** 16
    G = dcr(ei, n)
    for seed, batch in ((0, 0), (BIG_SEED, 3), (0, 2 ** 32 + 3), (0, 2 ** 48 - 1)):
        got = G.resistance_sketch_rhs(seed, batch)
        want = skref.batch_rhs(ei, n, seed, batch)
        assert got.shape == want.shape == (n, 16)
        assert np.array_equal(got, want), (name, seed, batch, np.argwhere(got != want)[:5])
    with pytest.raises(ValueError):
        G.resistance_sketch_rhs(0, 2 ** 48)


# ---- f. a relocated long row between calls ---------------------------------------------------------------------------------------------
def test_long_row_relocated_between_two_calls(dcr, c):
    ei, n, names = sc.sketch_three_groups()
    G = dcr(ei, n)
    hub, iso = names['hub0'], names['isolated']
    sketch(G, 16)                                                        # the slot accumulator exists before the edits
    before = G.number_of_edges()
    row = G.neighbors(hub)
    assert len(row) == 2100
    slack = max(8, len(row) // 4)                                        # slack_for of csrc/dcr_graph.hip: the row's room at creation
    fresh = np.setdiff1d(np.arange(130 * 130), row)[::7][:slack + 5]     # more than the row has room for: it is laid out again
    assert len(fresh) == slack + 5
    for v in fresh:
        G.add_edge(hub, int(v))
    gone = G.neighbors(hub)[len(row) // 2]                               # from the middle of the row
    G.remove_edge(hub, int(gone))
    assert not G.has_edge(hub, iso)
    G.add_edge(hub, iso)
    assert G.number_of_edges() == before + slack + 5 - 1 + 1 and len(G.neighbors(hub)) == 2100 + slack + 5
    now = G.to_edge_index()
    assert now.shape[1] == 2 * G.number_of_edges()
    case = skref.Case('sketch_three_groups after the edits', now, n, 48, 0, hub)
    assert case.labels[iso] == case.labels[hub] and len(case.hub_edges) == 2100 + slack + 5
    print(f'  after the edits: e_a = {case.e_a:.3e}, lam_lo = {case.lam_lo:.4e}')
    check_case(case, G, 48)
