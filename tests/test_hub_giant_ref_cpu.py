"""tests/hub_giant_ref.py against the C oracle, with hubs of a few hundred neighbours: every family that
tests/test_hub_giant_limits_gpu.py runs at the kernels' limits, the same builders with smaller parameters.  For every edge with
a closed form: the oracle's ingredients in both orientations and the bits of its value.  No GPU: a mistake in a builder or in a
closed form is caught here, not on the device."""
import numpy as np
import pytest

import hub_giant_ref as R


@pytest.fixture(scope='module')
def oracle():
    from oracle import c_oracle
    return c_oracle


def check_edge(C, oracle, u, v, e6, label):
    assert tuple(int(t) for t in C.ingredients(u, v)) == tuple(e6), (label, u, v)
    assert tuple(int(t) for t in C.ingredients(v, u)) == R.flip(e6), (label, v, u)
    want = 0.0 if min(e6[:2]) == 1 else R.bfc_formula(*e6)
    assert R.bits(C.curv_edge(u, v)) == R.bits(want) == R.bits(C.curv_edge(v, u)), (label, u, v)
    if min(e6[:2]) > 1:
        assert R.bits(want) == R.bits(oracle.bfc_formula(*e6))
    for ct, val in R.tri_values(e6).items():
        assert C.curv_edge(u, v, ct) == val, (label, ct)


def test_restated_rules():
    L = R.limits()
    assert (L['NC_MAXD'], L['HUB_OTHER_MAX'], L['HUB_TOUCH_CAP'], L['BLOCK'], L['GRID_CAP'], L['STREAM_GRID'], L['FIND_GRID']) == \
        (8190, 1022, 1024, 256, 1024, 4096, 2048)
    assert L['TRIP'] == 262144 and L['HUB_CNT_MB'] == 512 and L['HUB_WAVES_MAX'] == 2048
    # 2,048 waves up to 65,536 neighbours; then the budget: 70,001 -> 1,917 -> 1,916, no power of two
    assert [R.hub_waves(d) for d in (8191, 12000, 65536, 65537, 70001, 3)] == [2048, 2048, 2048, 2044, 1916, 4]
    assert R.hub_waves(70001) & (R.hub_waves(70001) - 1)
    assert R.slack_full_degree(8190) == 6552 and R.slack_full_degree(8191) == 6553 and R.slack_full_degree(62) == 50


@pytest.mark.parametrize('base,dc', [(300, 40), (257, 61)])
def test_three_hubs(oracle, base, dc):
    ei, n, info = R.three_hubs(base, dc)
    C = oracle.CGraph(ei, n)
    a, b, c = info['a'], info['b'], info['c']
    assert (C.degree(a), C.degree(b), C.degree(c)) == info['deg'] and info['deg'][0] > info['deg'][1] > dc == info['deg'][2]
    for (u, v), e6 in info['edges'].items():
        check_edge(C, oracle, u, v, e6, ('three_hubs', base))
        assert e6[2] > 1 and e6[3] > 1 and e6[4] > 1 and e6[5] > 1
    # every edge its own numbers: a value taken from another edge's state is a different value
    assert len({e6[2:] for e6 in info['edges'].values()}) == 3
    # the members that matter sit behind position base of the hubs' rows
    row = lambda k: ei[1][ei[0] == k]
    ra, rb, rc = row(a), row(b), row(c)
    for k in info['C'] + info['XL'] + info['OA']:
        assert np.flatnonzero(ra == k)[0] > base
    for k in info['C'] + info['YR'] + info['OB'] + info['FBL']:
        assert np.flatnonzero(rb == k)[0] > base
    # what a missed unmark of a (of b) leaves behind is met by the next edge: c's row holds OA (OB), no neighbours of b (of a)
    assert set(info['OA']) <= set(rc.tolist()) and not set(info['OA']) & set(rb.tolist())
    assert set(info['OB']) <= set(rc.tolist()) and not set(info['OB']) & set(ra.tolist())


@pytest.mark.parametrize('gamma_by', ['row', 'corner'])
def test_stream_fan(oracle, gamma_by):
    grid, block = 40, 8
    ei, n, info = R.stream_fan(300, grid, block, gamma_by)
    C = oracle.CGraph(ei, n)
    a, b = info['a'], info['b']
    e6 = info['edges'][(a, b)]
    check_edge(C, oracle, a, b, e6, ('stream_fan', gamma_by))
    rb = ei[1][ei[0] == b]
    assert all(np.flatnonzero(rb == y)[0] >= grid for y in info['Y2']) and all(np.flatnonzero(rb == y)[0] < grid for y in info['Y1'])
    rows, first = info['rows'], len(info['Y1'])
    assert e6[1] - e6[2] - 1 > grid                                     # more rows in DY than workgroups
    assert any(l > block for l in info['row_len'][:first]) and any(p > block and not cols for p, cols in rows)
    # a second-trip row longer than two blocks whose hits all sit in its last partial trip
    y, (pads, cols) = info['Y2'][0], rows[first]
    ry = ei[1][ei[0] == y]
    assert len(ry) > 2 * block and len(cols) > 0 and len(ry) - len(cols) >= (len(ry) - 1) // block * block >= 2 * block
    assert set(ry[len(ry) - len(cols):].tolist()) == {info['X'][j] for j in cols}
    col = np.bincount([j for _, cs in rows for j in cs])
    longest = max(len(cs) for _, cs in rows)
    assert e6[4] == sum(1 for _, cs in rows if cs) < len(rows)          # the row without a hit is not counted
    if gamma_by == 'row':
        assert e6[5] == longest > col.max()
    else:
        assert e6[5] == col.max() > longest


def check_stars(S, C, oracle, label, dh=None):
    eu, ev, cv = C.curv_all('bfc', nthreads=4)
    for k in range(S.H):
        d = S.deg[k] if dh is None else dh[k]
        at = np.flatnonzero(eu == k)
        pos = ev[at] - S.base[k]
        keep = (pos >= 0) & (pos < S.deg[k])
        want = S.values(k, d)
        assert np.array_equal(cv[at][keep].view(np.int64), want[pos[keep]].view(np.int64)), (label, k)
        for g in np.unique(S.kind[k]).tolist():
            p = int(np.flatnonzero(S.kind[k] == g)[-1])
            check_edge(C, oracle, k, S.base[k] + p, S.six(k, p, d), (label, k, g))


@pytest.mark.parametrize('K', [9, 10, 11, 12])
def test_touch_star(oracle, K):
    S, late = R.touch_star(100, K, 16, 5)
    C = oracle.CGraph(S.ei, S.n)
    assert S.six(0, late) == (100, 2, 0, K, 1, K) == S.six(0, 5) and (late - (5 + K - 1)) % 16 == 0
    check_stars(S, C, oracle, ('touch_star', K))


def test_budget_stars_and_growth(oracle):
    S = R.budget_stars(200, 700, 210, waves_of=lambda d: 16)
    assert all(len({int(g) for g in np.unique(k)}) == 4 for k in S.kind)        # plain, pair, two groups of different sizes
    C = oracle.CGraph(S.ei, S.n)
    check_stars(S, C, oracle, 'budget_stars')
    # leaves appended to a hub change its degree and nothing else; removing them again restores the values
    S = R.Stars([{'deg': 200, 'groups': [[3, 4, 5, 9]], 'pairs': [(20, 21)]}, {'deg': 210, 'groups': [[1, 2]]}], spare=30)
    C = oracle.CGraph(S.ei, S.n)
    for w in range(S.spare0, S.spare0 + 30):
        C.add_edge(1, w)
    check_stars(S, C, oracle, 'grown', dh=[200, 240])
    for w in range(S.spare0 + 29, S.spare0 + 4, -1):
        C.remove_edge(1, w)
    check_stars(S, C, oracle, 'shrunk', dh=[200, 215])


@pytest.mark.parametrize('second_hub', [None, 63])
def test_crossing(oracle, second_hub):
    limit = 62 if second_hub is None else 63
    ei, n, info = R.crossing(limit, (30, 62), 5, second_hub=second_hub, n_common=4)
    C = oracle.CGraph(ei, n)
    d0 = R.slack_full_degree(limit)
    assert C.degree(0) == d0 == info['d0'] and d0 + max(8, d0 // 4) == limit
    assert [C.degree(k) for k in info['centres']] == ([30, 62] if second_hub is None else [63])
    for w in info['grow']:
        assert not C.has_edge(0, w)
        C.add_edge(0, w)
    assert C.degree(0) == limit and all(C.has_edge(0, k) for k in info['centres'])
    assert len(info['fresh']) >= 4 and not any(C.has_edge(0, w) or any(C.has_edge(k, w) for k in info['centres']) for w in info['fresh'])
    assert max(C.degree(w) for w in range(1, limit + 41)) < 40
    if second_hub:
        u, v = 0, info['centres'][0]
        assert C.degree(u) + C.degree(v) + 2 == 2 * limit + 2 and int(C.ingredients(u, v)[2]) == 4
