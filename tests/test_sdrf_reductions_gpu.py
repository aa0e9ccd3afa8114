"""The reductions and the tail of an SDRF step (csrc/dcr_sdrf.hip: the edge-slot walker behind the arg-extremum sweeps, the
array arg-max, the reduction of partial extrema, the draw's blocks and segments, the tail runner) at the sizes where their loops
change shape.  Everything expected comes from numpy on data the wrappers download (edges and curvatures in G.edges order, the
improvement list) or from the C oracle's step; everything is compared exactly."""
import numpy as np
import pytest

from test_gpu_parity import _numpy_cdf

pytestmark = pytest.mark.gpu

INF = float('inf')


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


# ---- 1. edge sweeps at their round boundaries -------------------------------------------------------------------------------
def tied_gadgets(units):
    """``units`` groups of 16 nodes: a star of 4 leaves, two stars of 3 leaves, a path of 3 nodes — every edge at 0.  In the
    second half of the groups the path is closed into a triangle (the only positive Balanced Forman value, 1.5 on each of its
    edges), in the last 1 % the two hubs are joined (that edge is the only negative one, -1): the extrema are attained many
    times, "first in G.edges order" decides, and the first of each lies deep in the slot range — past the first stride, the
    minimum past the first round of four where there is a second.
    Returns (edge_index, nodes, negative edges, positive edges, adjacency slots: a row holds its degree + max(8, degree / 4)
    free places, 8 here)."""
    pairs = []
    first_pos, first_neg = units // 2, int(0.99 * units)
    for g in range(units):
        base = 16 * g
        pairs += [(base, base + k) for k in range(1, 5)]
        a, b = base + 5, base + 9
        pairs += [(a, a + k) for k in range(1, 4)] + [(b, b + k) for k in range(1, 4)] + ([(a, b)] if g >= first_neg else [])
        t = base + 13
        pairs += [(t, t + 1), (t + 1, t + 2)] + ([(t, t + 2)] if g >= first_pos else [])
    p = np.array(pairs, dtype=np.int64)
    ei = np.concatenate([p.T, p.T[::-1]], axis=1)
    ei = ei[:, np.lexsort((ei[1], ei[0]))]
    return ei, 16 * units, units - first_neg, 3 * (units - first_pos), ei.shape[1] + 8 * 16 * units


# a sweep launches min(ceil(slots / 256), 1024) workgroups; a thread takes slots s0 + q * stride, q = 0 .. 3, per round
SWEEP_UNITS = {'one_workgroup': 1, 'some_q_out_of_range': 4000, 'two_rounds': 7000}


@pytest.mark.parametrize('size', list(SWEEP_UNITS))
def test_edge_sweeps_at_their_round_boundaries(dcr, monkeypatch, size):
    ei, n, n_neg, n_pos, slots = tied_gadgets(SWEEP_UNITS[size])
    full = 1024 * 256
    if size == 'one_workgroup':
        assert slots <= 256
    elif size == 'some_q_out_of_range':
        assert 2 * full < slots < 3 * full               # q = 0, 1 and part of 2 in range, q = 3 never
    else:
        deg = np.bincount(ei[0], minlength=n)
        first_neg_hub = 16 * int(0.99 * SWEEP_UNITS[size]) + 5
        assert slots > int((deg[:first_neg_hub] + 8).sum()) > 4 * full   # the first minimum is met in the second round only
    monkeypatch.delenv('DCR_PASS', raising=False)
    G = dcr(ei, n)
    eu, ev, cv = G.curvature_all('bfc')
    lo, hi = int(np.argmin(cv)), int(np.argmax(cv))      # numpy: the first of equal values
    assert ((cv == cv[lo]).sum(), (cv == cv[hi]).sum()) == (n_neg, n_pos) and cv[lo] == -1.0 and cv[hi] == 1.5
    assert (lo > hi > len(cv) // 3) or size == 'one_workgroup'

    def at(k):
        return int(eu[k]), int(ev[k]), float(cv[k])

    assert G.argext(False) == at(lo)
    assert G.argext(True) == at(hi)
    rest = np.where(np.arange(len(cv)) == hi, -np.inf, cv)
    assert G.argext(True, exclude=(int(eu[hi]), int(ev[hi]))) == at(int(np.argmax(rest)))
    assert G.argext(True, exclude=(int(ev[hi]), int(eu[hi]))) == at(int(np.argmax(rest)))
    # the one sweep for both extrema and the reduction of its partials (node-centric pass), the closing kernel's partials and
    # the same reduction (two-hop pass, where that engine takes the graph)
    for engine, name in (('nc', 'node-centric'), ('h2', 'two-hop')):
        monkeypatch.setenv('DCR_PASS', engine)
        H = dcr(ei, n)
        first = H.curvature_pass_argmin('bfc')
        if H.pass_engine() != name:
            assert engine == 'h2'
            continue
        hu, hv, hc = H.curvature_read()
        assert np.array_equal(hu, eu) and np.array_equal(hv, ev) and np.array_equal(hc, cv)
        assert first == at(lo), (engine, first)
        imp, _, _ = H.improvements(first[0], first[1], 'bfc')     # leaves the stale arg-max from the partial maxima
        assert len(imp) > 0
        _, mx = H.sdrf_tail(None, True, 1e9)                      # (bound too high: nothing removed, the maximum reported)
        assert mx == cv[hi], (engine, mx)


# ---- 2. the array arg-max from both entry points, 3. the draw across blocks and segments -----------------------------------------
def hub_pair(target):
    """Two hubs x = 0, y = 1 joined by an edge, with lx and ly leaves: (lx + 1)(ly + 1) - 1 candidates exactly (every leaf of x
    with every leaf of y and with y, x with every leaf of y) — the factor pair of target + 1 nearest to a square."""
    a = next(a for a in range(int(np.sqrt(target + 1)), 1, -1) if (target + 1) % a == 0)
    lx, ly = a - 1, (target + 1) // a - 1
    assert 1 <= lx <= ly <= 1200
    pairs = [(0, 1)] + [(0, 2 + k) for k in range(lx)] + [(1, 2 + lx + k) for k in range(ly)]
    p = np.array(pairs, dtype=np.int64)
    ei = np.concatenate([p.T, p.T[::-1]], axis=1)
    return ei[:, np.lexsort((ei[1], ei[0]))], 2 + lx + ly


# either side of: one workgroup of the reductions (256), the second stride of the device draw's 256 workgroups (256 * 256), the
# host-n grid's saturation at 1,024 workgroups (1024 * 256)
ARGMAX_SIZES = [255, 257, 256 * 256 - 1, 256 * 256 + 1, 1024 * 256 - 1, 1024 * 256 + 5]
_hub_cache = {}


def hub_case(dcr, target):
    """(edge_index, nodes, improvements, ci, cj) of the hub pair, downloaded once per size and left unchanged."""
    if target not in _hub_cache:
        ei, n = hub_pair(target)
        G = dcr(ei, n)
        imp, ci, cj = G.improvements(0, 1, 'bfc', want_candidates=True)
        _hub_cache[target] = (ei, n, np.array(imp), np.array(ci), np.array(cj), G.improvements_argmax(),
                              [G.candidate_at(k) for k in (0, len(imp) - 1)])
    return _hub_cache[target]


@pytest.mark.parametrize('target', ARGMAX_SIZES)
def test_array_argmax_from_both_entry_points(dcr, target):
    ei, n, imp, ci, cj, host_n_argmax, ends = hub_case(dcr, target)
    assert len(imp) == target
    k = int(np.argmax(imp))
    assert (imp == imp[k]).sum() > 1 and np.unique(imp).size <= 4          # ties: the first index decides
    assert host_n_argmax == k
    assert ends == [(int(ci[0]), int(cj[0])), (int(ci[-1]), int(cj[-1]))]
    G = dcr(ei, n)                                                           # a fresh copy: the draw edits the graph
    status, n_cand, added, removed, _ = G.sdrf_iteration_device_draw(0, 1, 'bfc', INF, 0.5, False, 0.0)
    assert (status, n_cand, removed) == (0, target, None)
    assert tuple(added) == (int(ci[k]), int(cj[k])), (target, k, added)      # device-draw entry == numpy == host-n entry
    assert G.has_edge(*added) and G.number_of_edges() == ei.shape[1] // 2 + 1


DRAW_TAU = 1.0   # flat: every step of the cdf is about 1 / n, thousands of margins wide, so numpy alone decides every midpoint


def draw_indices(n):
    """The indices the draw has to land on: the ends of the list, of a block and of a thread's segment (csrc/dcr_sdrf.hip,
    draw_segment: 256 blocks of L = ceil(n / 256), a block in 256 segments of l = ceil(L / 256))."""
    L = -(-n // 256)
    seg = -(-L // 256)
    b = (n // L) // 2                                   # a block in the middle of those that hold anything
    t = min(37, (L - 1) // seg)
    idx = {'first': 0, 'last': n - 1, 'block_first': b * L, 'block_last': min((b + 1) * L, n) - 1,
           'segment_first': b * L + t * seg, 'segment_last': min(b * L + (t + 1) * seg, (b + 1) * L, n) - 1}
    assert all(0 <= i < n for i in idx.values())
    return idx


@pytest.mark.parametrize('target', [257, 256 * 256 + 1, 1024 * 256 - 1])
def test_finite_tau_draw_across_block_and_segment_edges(dcr, target):
    ei, n, imp, ci, cj, _, _ = hub_case(dcr, target)
    cdf = _numpy_cdf(imp, DRAW_TAU)
    margin = (target + 1024) * 2.0 ** -51               # the documented margin, relative to the total
    undecided = 0
    for where, i in draw_indices(target).items():
        below = 0.0 if i == 0 else float(cdf[i - 1])
        u = 0.5 * (below + float(cdf[i]))               # the midpoint of numpy's own cdf step
        assert 0.0 <= u < 1.0 and int(np.searchsorted(cdf, u, side='right')) == i
        gap = min(u - below, float(cdf[i]) - u)
        assert gap > 64 * margin, (where, gap, margin)  # numpy alone decides this uniform, far outside the margin
        G = dcr(ei, n)
        status, n_cand, added, removed, _ = G.sdrf_iteration_device_draw(0, 1, 'bfc', DRAW_TAU, u, False, 0.0)
        assert n_cand == target
        if status != 0:
            assert status == 1 and gap < margin, (where, i, status, gap, margin)   # undecided only inside the margin
            undecided += 1
            continue
        assert tuple(added) == (int(ci[i]), int(cj[i])), (target, where, i, added)
    assert undecided == 0


# ---- 4. every tail entry point gives the same edit -----------------------------------------------------------------------------
def overflowing_step():
    """A 300-node power-law graph plus edges to fresh nodes that fill, to the last free place, the rows of BOTH ends of the edge
    the first SDRF iteration (tau = inf) adds: found on the host with the oracle.  A row has max(8, degree / 4) free places
    when the graph is laid out (the construction of test_one_handle_across_sizes_and_edits)."""
    from dcr import synthetic
    from oracle import c_oracle
    ei, n0 = synthetic.powerlaw_graph(300, 3, seed=5)
    deg0 = np.bincount(ei[0], minlength=n0)
    spare = 200
    n = n0 + spare
    fillers, filled, nxt = [], set(), n0
    for _ in range(12):
        p = np.array(fillers, dtype=np.int64).reshape(-1, 2)
        full = synthetic.coalesced_edge_index(np.concatenate([ei[0], p[:, 0]]), np.concatenate([ei[1], p[:, 1]]), n)
        trace = []
        c_oracle.sdrf(full, n, 'bfc', 1, True, TAIL_BOUND, INF, trace=trace, nthreads=4)
        k, l = trace[0]['added']
        todo = [u for u in (k, l) if u not in filled]
        if not todo:
            return ei, n, fillers, full, trace[0], {u: int(deg0[u]) + max(8, int(deg0[u]) // 4) for u in (k, l)}
        for u in todo:
            assert u < n0
            slack = max(8, int(deg0[u]) // 4)
            fillers += [(u, nxt + s) for s in range(slack)]
            nxt += slack
            filled.add(u)
        assert nxt <= n
    raise AssertionError('no edge found whose two rows stay the ones the step adds to')


TAIL_BOUND = 0.3
_tail_cache = []


@pytest.mark.parametrize('entry', ['sdrf_tail', 'sdrf_tail_at', 'sdrf_tail_at_pass_argmin', 'device_draw'])
def test_every_tail_entry_point_gives_the_same_edit(dcr, entry):
    from oracle import c_oracle
    if not _tail_cache:
        ei, n, fillers, full, rec, caps = overflowing_step()
        C = c_oracle.CGraph(full, n)
        C.add_edge(*rec['added'])
        assert rec['removed'] is not None
        C.remove_edge(*rec['removed'])
        ou, ov, oc = C.curv_all('bfc', nthreads=4)
        m = int(np.argmin(oc))
        _tail_cache.append((ei, n, fillers, rec, caps, C.num_edges(), (int(ou[m]), int(ov[m]), float(oc[m])), C.to_edge_index()))
    ei, n, fillers, rec, caps, want_edges, want_next, want_ei = _tail_cache[0]
    G = dcr(ei, n)
    for u, w in fillers:
        G.add_edge(u, w)
    for u, cap in caps.items():
        assert G.degree(u) == cap                        # both rows are full: the step's add has to lay out again
    x, y, _ = G.curvature_pass_argmin('bfc')
    assert [x, y] == rec['argmin']
    if entry == 'device_draw':
        status, _, added, removed, nxt = G.sdrf_iteration_device_draw(x, y, 'bfc', INF, 0.5, True, TAIL_BOUND)
        assert status == 0
    else:
        imp, ci, cj = G.improvements(x, y, 'bfc', want_candidates=True)
        k = int(np.argmax(np.array(imp)))
        assert k == rec['choice']
        added = (int(ci[k]), int(cj[k]))
        if entry == 'sdrf_tail':
            removed, _ = G.sdrf_tail(added, True, TAIL_BOUND)
            nxt = G.curvature_pass_argmin('bfc')
        elif entry == 'sdrf_tail_at':
            added, removed, _ = G.sdrf_tail_at(k, True, TAIL_BOUND)
            nxt = G.curvature_pass_argmin('bfc')
        else:
            added, removed, nxt = G.sdrf_tail_at_pass_argmin(k, True, TAIL_BOUND, 'bfc')
    assert list(added) == rec['added'] and list(removed) == rec['removed'], (entry, added, removed)
    assert G.number_of_edges() == want_edges
    assert nxt == want_next, (entry, nxt, want_next)
    for u, cap in caps.items():
        assert G.degree(u) in (cap + 1, cap)             # (cap: the removal took an edge of the same row away again)
    assert np.array_equal(G.to_edge_index(), want_ei)
