"""The device-memory curvature paths (csrc/dcr_bfc_giant.hip) at their own limits, on the graphs of tests/hub_giant_ref.py,
whose integer ingredients are known in closed form (tests/test_hub_giant_ref_cpu.py proves them against the oracle with small
hubs): the second grid-stride trip of k_giant_mark / sweep / unmark, the strides of k_giant_stream, the list of touched slots
of k_hub_edges at 1,023 .. 1,026 entries, a wave budget below its cap with the per-wave counters re-allocated in a known order,
and edits that carry a node over the hub-supplement threshold (8,190) and an edge onto the giant list (16,384 keys).
Everything is compared by bits."""
import numpy as np
import pytest

import hub_giant_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


@pytest.fixture(scope='module')
def oracle():
    from oracle import c_oracle
    return c_oracle


def same_bits(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64).view(np.int64), np.asarray(want, dtype=np.float64).view(np.int64))


def whole_buffer(G, C, label):
    """The buffer of the last pass against the oracle's pass, edge list and bits."""
    eu, ev, cv = G.curvature_read()
    ou, ov, oc = C.curv_all('bfc', nthreads=8)
    assert np.array_equal(eu, ou) and np.array_equal(ev, ov), label
    bad = np.flatnonzero(cv.view(np.int64) != oc.view(np.int64))
    assert bad.size == 0, (label, int(bad.size), [(int(eu[i]), int(ev[i]), C.degree(int(eu[i])), C.degree(int(ev[i])), float(cv[i]),
                                                   float(oc[i])) for i in bad[:6]])
    return eu, ev, cv


def single_edge(G, u, v, e6, label):
    """Both orientations of the single-edge calls against the closed form; returns the bits of the Balanced Forman value."""
    got = tuple(int(t) for t in G.bfc_ingredients(u, v))
    assert got == tuple(e6), (label, '(deg u, deg v, T, |sq u|, |sq v|, gamma)', got, e6)
    got = tuple(int(t) for t in G.bfc_ingredients(v, u))
    assert got == R.flip(e6), (label, 'other orientation', got, R.flip(e6))
    val = G.curvature_edge(u, v, 'bfc')
    assert R.bits(val) == R.bits(R.bfc_formula(*e6)) == R.bits(G.curvature_edge(v, u, 'bfc')), (label, val, e6)
    for ct, want in R.tri_values(e6).items():
        assert G.curvature_edge(u, v, ct) == want, (label, ct)
    return R.bits(val)


# ------------------------------------------------------------------------------------------------ 1: mark / sweep / unmark
def test_second_trip_of_mark_sweep_and_unmark(dcr, oracle):
    """Hubs a and b with 262,176 and 262,170 neighbours: the grids of k_giant_mark, k_giant_sweep and k_giant_unmark are capped
    at 1,024 x 256 threads, so positions from 262,144 on belong to the second trip — and every common neighbour, every corner of
    a 4-cycle and every row with hits sits there, in both rows (asserted on G.neighbors).  Single-edge calls only.  {a, b} marks
    a; then {b, c} marks b, and c's row holds nodes of a's second-trip slots that are no neighbours of b: they count as
    triangles unless k_giant_unmark cleared them; then {a, c} marks a again and meets b's second-trip slots the same way; then
    {a, b} again, same bits (the counters behind 262,144 are cleared by the second trip of k_giant_mark).  The oracle's
    single-edge queries take a few milliseconds here (measured), so each closed form is asserted against it as well."""
    L = R.limits()
    ei, n, info = R.three_hubs(L['TRIP'], L['NC_MAXD'] + 10)
    a, b, c = info['a'], info['b'], info['c']
    G = dcr(ei, n)
    C = oracle.CGraph(ei, n)
    da, db, dc = (G.degree(k) for k in (a, b, c))
    assert (da, db, dc) == info['deg'] and da > db > L['TRIP'] and dc > L['NC_MAXD'] and dc + db + 2 > L['GIANT_KEYS']
    ra, rb = np.array(G.neighbors(a)), np.array(G.neighbors(b))
    assert np.array_equal(ra, ei[1][ei[0] == a]) and np.array_equal(rb, ei[1][ei[0] == b])
    for row, members in ((ra, info['C'] + info['XL'] + info['OA']), (rb, info['C'] + info['YR'] + info['OB'] + info['FBL'])):
        assert min(int(np.flatnonzero(row == k)[0]) for k in members) >= L['TRIP']
    first = None
    for u, v in ((a, b), (b, c), (a, c), (a, b)):
        e6 = info['edges'][(u, v)]
        assert tuple(int(t) for t in C.ingredients(u, v)) == e6 and R.bits(C.curv_edge(u, v)) == R.bits(R.bfc_formula(*e6))
        got = single_edge(G, u, v, e6, ('three_hubs', u, v))
        if (u, v) == (a, b):
            assert first in (None, got)
            first = got


# ------------------------------------------------------------------------------------------------ 2: k_giant_stream
@pytest.mark.parametrize('gamma_by', ['row', 'corner'])
def test_stream_strides(dcr, oracle, gamma_by):
    """One giant edge {a, b}: deg a = 16,400 (above every owner's limit), DY = N(b) \\ N(a) with more than 4,096 rows, so the
    workgroups of k_giant_stream take a second row; among the second rows one of 528 entries whose 7 hits sit in positions 521
    .. 527 (the last partial trip of the 256 threads), among the first a row of 301 entries ('row': all hits, gamma = 300 by
    row_hits; 'corner': one hit, gamma = 9 by the counter of a corner that nine rows share) and a row of 267 entries without a
    hit, which must not count into |sq b|.  Ingredients by closed form, then a full pass: the value in the buffer by closed
    form and the whole buffer by the oracle."""
    L = R.limits()
    ei, n, info = R.stream_fan(L['NC_MAXOTHER'] + 18, L['STREAM_GRID'], L['BLOCK'], gamma_by)
    assert n <= 40000
    a, b = info['a'], info['b']
    e6 = info['edges'][(a, b)]
    G = dcr(ei, n)
    C = oracle.CGraph(ei, n)
    rb = np.array(G.neighbors(b))
    assert all(int(np.flatnonzero(rb == y)[0]) >= L['STREAM_GRID'] for y in info['Y2'])
    assert G.degree(info['Y2'][0]) > 2 * L['BLOCK'] and max(G.degree(y) for y in info['Y1']) > L['BLOCK']
    assert e6[5] == (L['BLOCK'] + 44 if gamma_by == 'row' else 9)
    assert tuple(int(t) for t in C.ingredients(a, b)) == e6
    single_edge(G, a, b, e6, ('stream_fan', gamma_by))
    G.curvature_pass('bfc')
    eu, ev, cv = whole_buffer(G, C, ('stream_fan', gamma_by))
    at = np.flatnonzero((eu == a) & (ev == b))
    assert at.size == 1 and R.bits(cv[at[0]]) == R.bits(R.bfc_formula(*e6))
    single_edge(G, a, b, e6, ('stream_fan', gamma_by, 'after the pass'))


# ------------------------------------------------------------------------------------------------ hub-side sweep
def check_stars(G, C, S, label, dh=None, oracle_all=True, sample=0):
    """Every creation-time hub-leaf edge of the buffer against the closed form; the whole buffer against the oracle, or a sample
    of hub-leaf edges per hub against single oracle queries."""
    eu, ev, cv = G.curvature_read() if not oracle_all else whole_buffer(G, C, label)
    for k in range(S.H):
        d = S.deg[k] if dh is None else dh[k]
        assert G.degree(k) == d
        at = np.flatnonzero(eu == k)
        pos = ev[at] - S.base[k]
        keep = (pos >= 0) & (pos < S.deg[k])
        assert int(keep.sum()) == S.deg[k]
        got, want = cv[at][keep], S.values(k, d)[pos[keep]]
        bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
        assert bad.size == 0, (label, 'hub', k, int(bad.size), [(int(pos[keep][i]), int(S.kind[k][pos[keep][i]]), float(got[i]),
                                                                 float(want[i])) for i in bad[:6]])
        if sample:
            groups, pairs = np.flatnonzero(S.kind[k] > 0), np.flatnonzero(S.kind[k] < 0)
            pick = np.unique(np.concatenate([groups, pairs[:: max(1, pairs.size // sample)], np.arange(0, S.deg[k], S.deg[k] // 40)]))
            assert pick.size >= sample and set(groups.tolist()) <= set(pick.tolist())
            want = C.curv_edges(np.full(pick.size, k), S.base[k] + pick, 'bfc', nthreads=8)
            lookup = dict(zip(pos[keep].tolist(), got.tolist()))
            assert same_bits([lookup[int(p)] for p in pick], want), (label, 'hub', k, 'sample')


@pytest.mark.parametrize('ntouch', [1023, 1024, 1025, 1026])
def test_touched_list_boundary(dcr, oracle, ntouch):
    """A hub of 8,191 neighbours and one partner w adjacent to K + 1 of its leaves, K = ntouch - 1: each of those edges {h, v}
    flags its own slot and finds K unflagged slots, so the wave's list of touched slots ends at exactly ``ntouch`` entries
    (HUB_TOUCH_CAP = 1,024: the list path up to 1,024, the walk over everything from 1,025).  Closed form: (8191, 2, 0, K, 1, K).
    K of the leaves sit side by side; the last one sits 2,048 positions (the number of waves for this degree, from the
    launcher's rule) behind the K-th, so the same wave takes it one round later and its partner's row hits the very slots the
    earlier edge touched: a counter left non-zero changes |sq h| and gamma of the later edge.  Two passes, each compared with
    the closed form and the oracle: in the second the earlier edge meets what the later one left."""
    L = R.limits()
    dh, K = L['NC_MAXD'] + 1, ntouch - 1
    waves = R.hub_waves(dh)
    assert waves == L['HUB_WAVES_MAX'] and ntouch - L['HUB_TOUCH_CAP'] in (-1, 0, 1, 2)
    S, late = R.touch_star(dh, K, waves, 100)
    first = 100 + K - 1
    assert late % waves == first % waves and late // waves == first // waves + 1 and S.kind[0][late] == K + 1 == S.kind[0][first]
    assert S.six(0, late) == (dh, 2, 0, K, 1, K)
    G = dcr(S.ei, S.n)
    C = oracle.CGraph(S.ei, S.n)
    assert G.neighbors(0) == list(range(S.base[0], S.base[0] + dh)) and G.neighbors(S.base[0] + late) == [0, S.partner[0]]
    for turn in range(2):
        G.curvature_pass('bfc')
        check_stars(G, C, S, ('touch_star', ntouch, 'pass', turn))


def test_wave_budget_below_its_cap(dcr, oracle):
    """Hubs of 8,195, 70,001 and 8,200 neighbours in one graph: 512 MB of counters give the middle one 1,917 waves, rounded to
    1,916 (no power of two, below the cap of 2,048: 37 rounds per wave, cnt_stride = 70,001), the others 2,048.  Every hub has a
    group of leaves side by side, a group whose leaves all fall to ONE wave (positions 7 + r * waves: that wave meets the same
    slots in consecutive rounds) and 500 pairs (triangles).  All hub-leaf edges by closed form; at least 200 of each hub's, and
    every group leaf among them, against single queries of the oracle (its full pass would take minutes at 70,001).  Two
    passes.  The graph is built at full size (70,000 single adds are too slow for a test), so the order in which the hubs
    arrive, and with it the order of the counter re-allocations, is k_find_hubs's: test_counters_regrow_in_a_known_order
    forces it."""
    S = R.budget_stars(8195, 70001, 8200)
    assert [R.hub_waves(d) for d in S.deg] == [2048, 1916, 2048]
    G = dcr(S.ei, S.n)
    C = oracle.CGraph(S.ei, S.n)
    for turn in range(2):
        G.curvature_pass('bfc')
        check_stars(G, C, S, ('budget_stars', turn), oracle_all=False, sample=200 if turn == 0 else 0)
    eu, ev, cv = G.curvature_read()
    small = np.flatnonzero((eu == 0) | (eu == 2))
    assert same_bits(cv[small], C.curv_edges(eu[small], ev[small], 'bfc', nthreads=8))
    for ct in ('augmented', 'haantjes'):
        G.curvature_pass(ct)
        eu, ev, cv = G.curvature_read()
        for k in range(S.H):
            at = np.flatnonzero(eu == k)
            tri = (S.kind[k][ev[at] - S.base[k]] < 0).astype(np.float64)
            want = 4.0 - S.deg[k] - np.where(S.kind[k][ev[at] - S.base[k]] == 0, 1, 2) + 3 * tri if ct == 'augmented' else tri
            assert np.array_equal(cv[at], want), (ct, k)


def test_counters_regrow_in_a_known_order(dcr, oracle):
    """The per-wave counter array is re-allocated when a hub needs more than it holds.  Hubs of 8,191 and 8,200 neighbours, a
    pass; a third node grown from 8,000 to 12,000 by single adds (its row overflows once on the way), a pass: the array grows
    behind smaller hubs and is used with a stride of 12,000; the node shrunk to 8,150 again, a pass: the small hubs reuse the
    larger array with their own strides.  Every pass against the closed form and the oracle's whole pass."""
    S = R.Stars([{'deg': 8191, 'groups': [list(range(10, 60)), [7, 7 + 2048, 7 + 4096]], 'pairs': [(100 + 2 * i, 101 + 2 * i) for i in range(300)]},
                 {'deg': 8000, 'groups': [list(range(20, 90)), [9, 9 + 2048, 9 + 4096]], 'pairs': [(200 + 2 * i, 201 + 2 * i) for i in range(300)]},
                 {'deg': 8200, 'groups': [list(range(30, 70))], 'pairs': [(300 + 2 * i, 301 + 2 * i) for i in range(300)]}], spare=4000)
    G = dcr(S.ei, S.n)
    C = oracle.CGraph(S.ei, S.n)
    G.curvature_pass('bfc')
    check_stars(G, C, S, 'two hubs')
    extra = list(range(S.spare0, S.spare0 + 4000))
    for w in extra:
        G.add_edge(1, w)
        C.add_edge(1, w)
    G.curvature_pass('bfc')
    check_stars(G, C, S, 'the third grown', dh=[8191, 12000, 8200])
    for w in extra[:149:-1]:
        G.remove_edge(1, w)
        C.remove_edge(1, w)
    G.curvature_pass('bfc')
    check_stars(G, C, S, 'and shrunk', dh=[8191, 8150, 8200])


# ------------------------------------------------------------------------------------------------ 5: edits across the thresholds
def grown(dcr, oracle, limit, **kw):
    ei, n, info = R.crossing(limit, (1000, 1023, R.limits()['NC_MAXD']), limit, **kw)
    G = dcr(ei, n)
    C = oracle.CGraph(ei, n)
    assert G.degree(0) == info['d0']
    for w in info['grow']:                              # capacity d0 + d0 // 4 == limit: the row is now full
        G.add_edge(0, w)
        C.add_edge(0, w)
    assert G.degree(0) == limit == C.degree(0)
    return G, C, info


@pytest.mark.parametrize('how', ['add_edge', 'fused_tail'])
def test_edit_crosses_the_hub_supplement_threshold(dcr, oracle, monkeypatch, how):
    """tests/test_gpu_parity.py: test_fused_tail_replay_when_the_add_crosses_a_degree_class one limit further: the hub sits at
    exactly 8,190 neighbours, the largest degree of the node-centric classes, and its row is full.  One add — G.add_edge and an
    incremental pass, or the add inside dcr_sdrf_tail_at_pass_argmin, which overflows, lays out again and replays — takes it to
    8,191: from then on its edges to nodes of at most 1,022 neighbours are the hub-side sweep's, launched only if the host's
    bound on the degrees was raised with the add.  Its neighbours include nodes of 1,000, 1,023 and 8,190 neighbours; the whole
    buffer equals the oracle's.  Then one edge is removed: the hub is back at 8,190, the bound stays, the supplement finds no
    hub and the node-centric classes own the edges again."""
    monkeypatch.setenv('DCR_PASS', 'nc')
    L = R.limits()
    limit = L['NC_MAXD']
    G, C, info = grown(dcr, oracle, limit)
    assert [G.degree(k) for k in info['centres']] == [1000, 1023, limit] and all(G.has_edge(0, k) for k in info['centres'])
    G.curvature_pass('bfc')
    assert G.pass_engine() == 'node-centric'
    whole_buffer(G, C, 'at the limit')
    if how == 'add_edge':
        pair = (0, info['fresh'][0])
        G.add_edge(*pair)
        C.add_edge(*pair)
        G.curvature_pass('bfc', incremental=True)
        whole_buffer(G, C, 'one above, incremental')
    else:
        y = next(v for v in G.neighbors(0) if G.degree(v) < 40 and any(not G.has_edge(0, j) and j != 0 for j in G.neighbors(v)))
        imp, ci, cj = G.improvements(0, y, 'bfc', want_candidates=True)
        idx = next(k for k in range(len(ci)) if 0 in (int(ci[k]), int(cj[k])))
        pair = (int(ci[idx]), int(cj[idx]))
        added, removed, (mu, mv, mval) = G.sdrf_tail_at_pass_argmin(idx, False, 0.0, 'bfc')
        assert tuple(added) == pair and removed is None
        C.add_edge(*pair)
        eu, ev, cv = whole_buffer(G, C, 'one above, fused tail')
        k = int(np.argmin(cv))
        assert (mu, mv, mval) == (int(eu[k]), int(ev[k]), float(cv[k]))
    assert G.degree(0) == limit + 1
    G.remove_edge(*pair)
    C.remove_edge(*pair)
    assert G.degree(0) == limit
    G.curvature_pass('bfc', incremental=True)
    whole_buffer(G, C, 'back at the limit, incremental')


def test_edit_moves_an_edge_onto_the_giant_list(dcr, oracle, monkeypatch):
    """Two adjacent hubs of 8,191 neighbours each: 16,384 keys, the largest table of the edge-centric kernels, which take the
    edge in the hub supplement.  One add to either takes it to 16,385 keys: between two passes the edge moves onto the giant
    list, which exists only if the host's bound went to 8,192 with the add.  Four common neighbours; whole buffer by the
    oracle before, after, and after the removal that takes the edge back."""
    monkeypatch.setenv('DCR_PASS', 'nc')
    L = R.limits()
    limit = L['NC_MAXD'] + 1
    G, C, info = grown(dcr, oracle, limit, second_hub=limit, n_common=4)
    u, v = 0, info['centres'][0]
    assert G.degree(u) + G.degree(v) + 2 == L['GIANT_KEYS'] and G.has_edge(u, v)
    G.curvature_pass('bfc')
    whole_buffer(G, C, '16,384 keys')
    want = R.bits(C.curv_edge(u, v))
    assert R.bits(G.curvature_edge(u, v)) == want
    w = info['fresh'][0]
    G.add_edge(v, w)
    C.add_edge(v, w)
    assert G.degree(u) + G.degree(v) + 2 == L['GIANT_KEYS'] + 1
    G.curvature_pass('bfc', incremental=True)
    eu, ev, cv = whole_buffer(G, C, '16,385 keys, incremental')
    at = np.flatnonzero((eu == u) & (ev == v))
    assert at.size == 1 and R.bits(cv[at[0]]) == R.bits(C.curv_edge(u, v)) != want
    assert R.bits(G.curvature_edge(u, v)) == R.bits(cv[at[0]]) and int(G.bfc_ingredients(u, v)[2]) == 4
    G.remove_edge(v, w)
    C.remove_edge(v, w)
    G.curvature_pass('bfc', incremental=True)
    eu, ev, cv = whole_buffer(G, C, '16,384 keys again')
    assert R.bits(cv[np.flatnonzero((eu == u) & (ev == v))[0]]) == want
