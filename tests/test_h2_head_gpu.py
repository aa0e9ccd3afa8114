"""The head of the two-hop pass (csrc/dcr_bfc_h2.hip) once the node weights W(u) = sum of deg(k) over k in N(u) are kept current by
the edit kernels (csrc/dcr_graph.hip: dev_weight_edit) and the clearing work of k_h2_clear / k_h2_retry_zero is done by the two
plan kernels.  After every batch of edits a two-hop pass of the edited graph equals a node-centric pass of a twin graph bit for
bit, and DcrGraph.h2_weight_check() — W recomputed from the rows against the kept array — finds no difference."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEADY = {'launches': 1, 'weight_kernels': 0, 'clear_kernels': 0}   # one launch, its head the two plan kernels alone
FIRST = 'first'   # a graph's first pass: the weights computed once, every launch of the call with the full head


@pytest.fixture()
def twins(monkeypatch):
    """(H, D): the same graph under the two-hop engine and under the node-centric one."""
    from dcr.graph import DcrGraph

    def make(ei, n):
        monkeypatch.setenv('DCR_PASS', 'h2')
        H = DcrGraph(ei, n)
        monkeypatch.setenv('DCR_PASS', 'nc')
        D = DcrGraph(ei, n)
        monkeypatch.setenv('DCR_PASS', 'h2')
        return H, D
    return make


def same_values(H, D, what=None):
    """H's curvature buffer against a fresh node-centric pass of D."""
    hu, hv, hc = H.curvature_read()
    du, dv, dc = D.curvature_all('bfc')
    assert D.pass_engine() == 'node-centric'
    assert np.array_equal(hu, du) and np.array_equal(hv, dv), what
    bad = np.flatnonzero(hc.view(np.int64) != dc.view(np.int64))
    assert bad.size == 0, (what, bad.size, hu[bad[:5]], hv[bad[:5]], hc[bad[:5]], dc[bad[:5]])


def check(H, D, what=None, head=None):
    """A full two-hop pass of H against D, and the kept weights against the rows."""
    H.curvature_pass('bfc')
    assert H.pass_engine() == 'two-hop', what
    info = dict(H.h2_head_info(), launches=H.h2_launch_info()['launches'])
    print(what, H.h2_launch_info(), info)
    if head == FIRST:
        assert info['weight_kernels'] == 1 and info['clear_kernels'] == info['launches'] >= 1, (what, info)
    elif head is not None:
        assert info == head, (what, info)
    same_values(H, D, what)
    assert H.h2_weight_check() == 0, what
    return info


def both(H, D, op, u, v):
    getattr(H, op)(int(u), int(v))
    getattr(D, op)(int(u), int(v))


def powerlaw(n, m, seed):
    from dcr import synthetic
    return synthetic.powerlaw_graph(n, m, seed=seed)


def hubs_of(ei, n, k):
    deg = np.bincount(ei[0], minlength=n)
    return [int(u) for u in np.argsort(-deg, kind='stable')[:k]]


def test_fresh_graph_runs_the_full_head_then_the_two_plan_kernels(twins):
    """No weights are kept before the first two-hop pass (the array is allocated by it) and the result block is fresh: k_h2_weight
    and the stand-alone clear run.  From the second pass on neither does — with edits in between or without."""
    ei, n = powerlaw(3000, 5, 1)
    H, D = twins(ei, n)
    assert H.h2_weight_check() == -1
    assert H.h2_head_info() == {'weight_kernels': 0, 'clear_kernels': 0}    # (no launch yet)
    check(H, D, 'first', FIRST)
    check(H, D, 'second', STEADY)
    both(H, D, 'add_edge', 17, 2900)
    check(H, D, 'third', STEADY)
    H2, D2 = twins(ei, n)                        # another graph object: its own array, its own first pass
    both(H2, D2, 'add_edge', 17, 2900)           # (an edit before any pass: there is nothing to keep yet)
    assert H2.h2_weight_check() == -1
    check(H2, D2, 'first of the second graph', FIRST)
    check(H, D, 'fourth', STEADY)


def test_edits_at_the_top_hub_and_between_hubs_with_common_neighbours(twins):
    ei, n = powerlaw(4000, 8, 2)
    H, D = twins(ei, n)
    check(H, D, 'start', FIRST)
    h0, h1 = hubs_of(ei, n, 2)
    common = set(D.neighbors(h0)) & set(D.neighbors(h1))
    assert len(common) >= 2                      # every one of them gets +2 / -2
    first, second = ('remove_edge', 'add_edge') if D.has_edge(h0, h1) else ('add_edge', 'remove_edge')
    both(H, D, first, h0, h1)
    check(H, D, 'hub-hub ' + first, STEADY)
    both(H, D, second, h0, h1)
    check(H, D, 'hub-hub ' + second, STEADY)
    far = next(w for w in range(n - 1, 0, -1) if not D.has_edge(h0, w))
    both(H, D, 'add_edge', h0, far)
    check(H, D, 'hub-far add', STEADY)
    c = sorted(common)[0]
    both(H, D, 'remove_edge', h0, c)             # a removal at the top hub, of an edge inside a triangle with the other hub
    check(H, D, 'hub-common remove', STEADY)
    both(H, D, 'remove_edge', h0, far)
    both(H, D, 'add_edge', h0, c)                # two edits between two passes
    check(H, D, 'two edits', STEADY)


def test_degree_one_degree_zero_and_remove_then_re_add(twins):
    ei, n = powerlaw(3000, 5, 3)
    H, D = twins(ei, n)
    check(H, D, 'start', FIRST)
    z = n - 7
    nb = D.neighbors(z)
    assert len(nb) >= 3
    for w in nb[1:]:
        both(H, D, 'remove_edge', z, w)
    assert H.degree(z) == 1
    check(H, D, 'down to degree 1', STEADY)
    other = next(w for w in range(100, n) if w != z and not D.has_edge(z, w))
    both(H, D, 'add_edge', z, other)             # an add onto a degree-1 node
    check(H, D, 'add onto degree 1', STEADY)
    both(H, D, 'remove_edge', z, other)
    both(H, D, 'remove_edge', z, nb[0])          # leaves z with degree 0
    assert H.degree(z) == 0
    check(H, D, 'degree 0', STEADY)
    both(H, D, 'add_edge', z, nb[0])             # the same edge back, a pass in between ...
    check(H, D, 're-add', STEADY)
    both(H, D, 'remove_edge', z, nb[0])
    both(H, D, 'add_edge', z, nb[0])             # ... and none in between
    check(H, D, 'remove and re-add', STEADY)


def test_edits_that_do_not_happen_leave_the_weights_alone(twins):
    ei, n = powerlaw(3000, 6, 4)
    H, D = twins(ei, n)
    check(H, D, 'start', FIRST)
    h0 = hubs_of(ei, n, 1)[0]
    w = D.neighbors(h0)[3]
    ne = H.number_of_edges()
    H.add_edge(h0, w)                            # exists: add_status 2
    assert H.number_of_edges() == ne and H.h2_weight_check() == 0
    absent = next(v for v in range(n - 1, 0, -1) if not D.has_edge(h0, v))
    with pytest.raises(KeyError):
        H.remove_edge(h0, absent)
    assert H.number_of_edges() == ne and H.h2_weight_check() == 0
    check(H, D, 'nothing happened', STEADY)


def test_add_into_a_full_row_is_replayed_behind_a_relayout(twins):
    """The top hub's row is filled to its capacity; the add inside dcr_sdrf_tail_at_pass_argmin overflows (nothing is edited, the
    pass runs on the unedited graph), the rows are laid out again — the kept weights survive that, no degree changes — the tail
    is replayed and the pass redone.  Had the failed attempt moved a weight, the check behind the replay would see it."""
    ei, n = powerlaw(3000, 6, 5)
    H, D = twins(ei, n)
    x = hubs_of(ei, n, 1)[0]
    d0 = D.degree(x)
    cap = d0 + max(8, d0 // 4)
    check(H, D, 'start', FIRST)
    fill = [w for w in range(n - 1, 0, -1) if w != x and not D.has_edge(x, w)][:cap - d0]
    for w in fill:
        both(H, D, 'add_edge', x, w)
    assert H.degree(x) == cap
    check(H, D, 'row full', STEADY)
    y = next(v for v in D.neighbors(x) if any(j != x and not D.has_edge(x, j) for j in D.neighbors(v)))
    imp, ci, cj = H.improvements(x, y, 'bfc', want_candidates=True)
    idx = next(k for k in range(len(ci)) if x in (int(ci[k]), int(cj[k])))
    pair = (int(ci[idx]), int(cj[idx]))
    added, removed, _ = H.sdrf_tail_at_pass_argmin(idx, False, 0.0, 'bfc')
    assert tuple(added) == pair and removed is None and H.degree(x) == cap + 1
    assert H.pass_engine() == 'two-hop' and H.h2_head_info()['weight_kernels'] == 0
    D.add_edge(*pair)
    same_values(H, D, 'behind the replay')
    assert H.h2_weight_check() == 0
    check(H, D, 'next pass', STEADY)


def test_undecided_device_draw_edits_nothing(twins, monkeypatch):
    ei, n = powerlaw(3000, 5, 6)
    H, D = twins(ei, n)
    check(H, D, 'start', FIRST)
    x, y, _ = H.curvature_pass_argmin('bfc')
    monkeypatch.setenv('DCR_DRAW_MARGIN_SCALE', '1e30')
    ne = H.number_of_edges()
    status, n_cand, _, _, _ = H.sdrf_iteration_device_draw(x, y, 'bfc', 163.0, 0.37, True, 0.5)
    assert status == 1 and H.number_of_edges() == ne
    assert H.h2_weight_check() == 0
    monkeypatch.delenv('DCR_DRAW_MARGIN_SCALE')
    check(H, D, 'nothing was edited', STEADY)
    # the same iteration with the margins as they are: where the draw decides, the add and the removal happen on the device
    x, y, _ = H.curvature_pass_argmin('bfc')
    status, _, added, removed, _ = H.sdrf_iteration_device_draw(x, y, 'bfc', 163.0, 0.37, True, 0.5)
    if status == 0:
        D.add_edge(*added)
        if removed:
            D.remove_edge(*removed)
        same_values(H, D, 'behind the device-side iteration')
    assert H.h2_weight_check() == 0


def kept_weight(G, u):
    return sum(G.degree(k) for k in G.neighbors(u))


@pytest.mark.parametrize('boundary', [1024, 4096])
def test_weight_exactly_at_a_class_boundary(twins, boundary):
    """A node of at most 64 neighbours whose W is brought to exactly h2_maxw(0) = 1,024 (the last weight of wave class 0) or
    h2_maxw(2) = 4,096 (the last of the wave classes: the next one is a block class) by edges added at its neighbours; one
    more add next to it changes its class, one removal brings it back."""
    ei, n = powerlaw(5000, 8 if boundary == 1024 else 10, 7)
    H, D = twins(ei, n)
    deg = np.bincount(ei[0], minlength=n)
    W = np.bincount(ei[0], weights=deg[ei[1]], minlength=n).astype(np.int64)
    ok = np.flatnonzero((deg <= 60) & (deg >= 4) & (W <= boundary - 4) & (W >= boundary - 40))
    if ok.size == 0:                             # (4,096 at <= 64 neighbours: a node next to hubs; take the nearest below)
        below = np.flatnonzero((deg <= 60) & (deg >= 4) & (W <= boundary - 4))
        ok = below[np.argsort(-W[below], kind='stable')[:1]]
    x = int(ok[0])
    check(H, D, 'start', FIRST)
    assert kept_weight(D, x) == int(W[x])
    nb = D.neighbors(x)
    outside = (w for w in range(n - 1, 0, -1) if w != x and w not in nb)
    i = 0
    w_now = int(W[x])
    while w_now < boundary:                      # every add at a neighbour of x, to a node outside N(x), gives W[x] + 1
        k, w = nb[i % len(nb)], next(outside)
        i += 1
        if D.has_edge(k, w):
            continue
        both(H, D, 'add_edge', k, w)
        w_now += 1
    assert kept_weight(D, x) == boundary and D.degree(x) <= 64
    check(H, D, 'at the boundary', STEADY)
    k, w = nb[0], next(w for w in outside if not D.has_edge(nb[0], w))
    both(H, D, 'add_edge', k, w)
    assert kept_weight(D, x) == boundary + 1
    check(H, D, 'one above', STEADY)
    both(H, D, 'remove_edge', k, w)
    assert kept_weight(D, x) == boundary
    check(H, D, 'back at the boundary', STEADY)


def test_eight_passes_with_edits_and_incremental_passes_in_between(twins):
    """Both parities of the bucket halves several times over, and the node-centric route of an incremental pass between two
    full ones: it reads the node flags and the list of flagged nodes that the first plan kernel now clears."""
    ei, n = powerlaw(4000, 6, 8)
    H, D = twins(ei, n)
    rng = np.random.Generator(np.random.PCG64(8))
    hubs = hubs_of(ei, n, 30)
    check(H, D, 'start', FIRST)
    for rnd in range(8):
        for _ in range(int(rng.integers(1, 4))):
            a, b = hubs[int(rng.integers(0, 30))], int(rng.integers(0, n))
            if rng.random() < 0.5:
                nbs = D.neighbors(a)
                both(H, D, 'remove_edge', a, nbs[int(rng.integers(0, len(nbs)))])
            elif a != b and not D.has_edge(a, b):
                both(H, D, 'add_edge', a, b)
        if rnd in (2, 3, 6):
            H.curvature_pass('bfc', incremental=True)
            assert H.pass_engine() == 'node-centric' and H.h2_launch_info()['launches'] == 0
            same_values(H, D, ('incremental', rnd))
            assert H.h2_weight_check() == 0
            a, b = hubs[rnd], hubs[rnd + 1]
            both(H, D, 'remove_edge' if D.has_edge(a, b) else 'add_edge', a, b)
            if rnd == 3:                         # two incremental passes in a row
                H.curvature_pass('bfc', incremental=True)
                same_values(H, D, ('incremental again', rnd))
        check(H, D, ('round', rnd), STEADY)


def test_a_pass_that_reports_a_status_is_followed_by_the_full_head(twins):
    """An edit makes a later pass of the graph need the triangle stage it is launched without (status 4, nothing written): the
    launch that follows inside the same call starts from the stand-alone clear again, with the kept weights."""
    from test_h2_triangle_stage_gpu import JOIN_MAXM, joining_graph
    ei, n, (x, y, nb) = joining_graph(seed=1, twin_rows=JOIN_MAXM)
    H, D = twins(ei, n)
    check(H, D, 'start')
    check(H, D, 'second', STEADY)
    assert not H.h2_launch_info()['triangle_stage']
    both(H, D, 'add_edge', int(y), int(nb[JOIN_MAXM]))
    check(H, D, 'refused and launched again', {'launches': 2, 'weight_kernels': 0, 'clear_kernels': 1})
    assert H.h2_launch_info()['triangle_stage']
    check(H, D, 'steady again', STEADY)


def test_sixty_sdrf_iterations_on_the_engine_against_the_oracle(monkeypatch):
    import torch
    from dcr.data import Data
    from oracle import c_oracle
    from rewiring.sdrf_no_cuda import SdrfRun
    ei, n = powerlaw(4000, 5, 9)
    loops = 60
    np.random.seed(5)
    want = c_oracle.sdrf(ei, n, 'bfc', loops, True, 0.5, 163.0, nthreads=8)
    monkeypatch.setenv('DCR_PASS', 'h2')
    np.random.seed(5)
    run = SdrfRun(Data(edge_index=torch.from_numpy(ei), num_nodes=n), 'bfc', True, 0.5, 163.0, incremental=False)
    for i in range(loops):
        if not run.step(more=i + 1 < loops):
            break
        if i == 1:
            assert run.G.pass_engine() == 'two-hop' and run.G.h2_head_info() == {'weight_kernels': 0, 'clear_kernels': 0}
    assert run.G.pass_engine() == 'two-hop'
    assert np.array_equal(run.result().edge_index.numpy(), want)
    assert run.G.h2_weight_check() == 0
