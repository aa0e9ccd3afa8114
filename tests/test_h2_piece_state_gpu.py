"""Two pieces of state of the two-hop engine (csrc/dcr_bfc_h2.hip).

The wave classes (h2s_node) keep ONE 32-bit word per 16-byte piece of a node — valid-entry mask and row — and take the reverse
slot of every edge {u, v} (where u sits in row v) in sweep A, from the row descriptors, into a per-wave array that no later clear
touches.  The cases put u where that can go wrong: every entry position of a piece, the first and the last piece of a long row,
rows 32-63, nodes that use every piece of their class, a row that is the single entry u, and a node whose exact-path queue is
drained several times between the slot being taken and being published.

The edge set the block classes probe is kept across passes and brought up to date from the edit journal by one thread of
k_h2_plan<1> (no launch of its own).  The cases edit a graph that has had a two-hop pass through the public edit calls — an edge
the join probes, a tombstone followed by a re-insert, edits that do not happen, a full journal and an overflowing one, a pass that
is refused and launched again — each followed by a forced two-hop pass: one launch, the two plan kernels as its whole head.

Every case forces the engine with DCR_PASS=h2 and compares every edge's curvature, bit for bit, with the node-centric engine on
a twin graph (DCR_PASS=nc) and with the C oracle, and asserts that no node went to the retry list and no unit to the probe path
(the refused pass aside, which is about exactly that).  The graphs have a few hundred nodes (a few thousand entries where a
class's weight limit is the case) and are built here, node by node."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'discrete-curvature-rewiring_amd', 'csrc')


def _constants():
    """H2_QCAP, the wave classes' weight limits, their degree limit and the journal's capacity, read from the source."""
    src = open(os.path.join(_CSRC, 'dcr_bfc_h2.hip')).read()
    qcap = int(re.search(r'constexpr int H2_QCAP = (\d+);', src).group(1))
    deg = int(re.search(r'constexpr int H2_SMALL_DEG = (\d+);', src).group(1))
    m = re.search(r'h2_maxw\(int c\) \{ return c == 0 \? (\d+) : c == 1 \? (\d+) : c == 2 \? (\d+) :', src)
    log = int(re.search(r'constexpr int EDIT_LOG_CAP = (\d+);', open(os.path.join(_CSRC, 'dcr_internal.h')).read()).group(1))
    return qcap, deg, tuple(int(x) for x in m.groups()), log


QCAP, SMALL_DEG, MAXW, EDIT_LOG_CAP = _constants()
STEADY = {'launches': 1, 'weight_kernels': 0, 'clear_kernels': 0}   # one launch, its head the two plan kernels alone


def _rows(ei, n):
    order = np.lexsort((ei[1], ei[0]))
    src, dst = ei[0][order], ei[1][order]
    ptr = np.searchsorted(src, np.arange(n + 1))
    return [dst[ptr[i]:ptr[i + 1]] for i in range(n)]


def _weight(rows, u):
    return int(sum(len(rows[v]) for v in rows[u]))


def _queue_total(rows, u):
    """Entries of node u that go to the exact path: occurrences of keys that occur more than once in the rows of u's
    neighbours, plus the members of N(u) met there (u itself is left out)."""
    keys = np.concatenate([rows[v] for v in rows[u]])
    keys = keys[keys != u]
    uniq, cnt = np.unique(keys, return_counts=True)
    return int(cnt[(cnt > 1) | np.isin(uniq, rows[u])].sum())


def _edges(pairs, n):
    from dcr import synthetic
    a = np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)
    return synthetic.coalesced_edge_index(a[:, 0], a[:, 1], n)


def _twins(monkeypatch, ei, n):
    """(H, D): the same graph under the two-hop engine and under the node-centric one."""
    from dcr.graph import DcrGraph
    monkeypatch.setenv('DCR_PASS', 'h2')
    H = DcrGraph(ei, n)
    monkeypatch.setenv('DCR_PASS', 'nc')
    D = DcrGraph(ei, n)
    monkeypatch.setenv('DCR_PASS', 'h2')
    return H, D


def _compare(H, D, ei, n, what=None, clean=True):
    """A forced two-hop pass of H against a node-centric pass of D and against the C oracle on the edge list `ei`, bit for bit."""
    from oracle import c_oracle
    hu, hv, hc = H.curvature_all('bfc')
    assert H.pass_engine() == 'two-hop', what
    info, stats = dict(H.h2_launch_info(), **H.h2_head_info()), H.h2_stats()
    if clean:
        assert stats['retry'] == 0 and stats['fallback'] == 0 and not info['retry_stage'] and not info['triangle_stage'], (what, stats, info)
    du, dv, dc = D.curvature_all('bfc')
    assert D.pass_engine() == 'node-centric', what
    assert np.array_equal(hu, du) and np.array_equal(hv, dv), what
    # (an edited graph lists its edges in the order they came: the oracle is asked edge by edge, and for the same set of edges)
    keep = ei[0] < ei[1]
    got = np.minimum(hu, hv).astype(np.int64) * n + np.maximum(hu, hv)
    assert np.array_equal(np.sort(got), np.sort(ei[0][keep].astype(np.int64) * n + ei[1][keep])), what
    oc = c_oracle.CGraph(ei, n).curv_edges(hu, hv, 'bfc', nthreads=8)
    for name, ref in (('node-centric', dc), ('oracle', oc)):
        bad = np.flatnonzero(hc.view(np.int64) != ref.view(np.int64))
        assert bad.size == 0, (what, name, bad.size, hu[bad[:5]], hv[bad[:5]], hc[bad[:5]], ref[bad[:5]])
    return info, stats


def _check(monkeypatch, ei, n):
    H, D = _twins(monkeypatch, ei, n)
    info, stats = _compare(H, D, ei, n)
    assert info['launches'] == 1, info
    H.close()
    D.close()
    return stats


# =====================================================================================================================
# the wave classes' piece state
# =====================================================================================================================
@pytest.mark.parametrize('start', [0, 1, 2, 3])
def test_u_in_every_entry_position(monkeypatch, start):
    """Node U has eight neighbours; neighbour p has start + p neighbours with smaller ids than U, so that U is entry start + p
    of its row: whatever the container makes of the rows' alignment, the eight rows put U into each of the four entry positions
    of a piece twice, in the first piece of a row and in the second.  (The smaller ids are shared by the rows: repeats.)"""
    low = 12                                   # ids 0 .. low - 1 sort before U
    U = low
    pairs, nxt = set(), U + 9
    for p in range(8):
        v = U + 1 + p
        pairs.add((U, v))
        for t in range(start + p):
            pairs.add((t, v))
        for _ in range(3 + p % 3):             # and a few ids above U behind it
            pairs.add((v, nxt))
            nxt += 1
    ei = _edges(pairs, nxt)
    rows = _rows(ei, nxt)
    where = sorted(int(np.flatnonzero(rows[U + 1 + p] == U)[0]) for p in range(8))
    assert where == [start + p for p in range(8)]
    _check(monkeypatch, ei, nxt)


@pytest.mark.parametrize('length', [37, 64, 131])
def test_u_in_the_first_and_in_the_last_piece_of_a_row(monkeypatch, length):
    """Rows of `length` entries (10, 16 and 33 pieces, or one more) whose smallest id is node A and whose largest is node B: A
    sits in the first piece of each, B in the last; both nodes read the same three rows, so every other key repeats."""
    A, vs = 0, [1, 2, 3]
    pairs, nxt = set(), 4
    for i, v in enumerate(vs):
        pairs.add((A, v))
        for _ in range(length - 2 + i):        # (three lengths in a row: three alignments of the last piece)
            pairs.add((v, nxt))
            nxt += 1
    B = nxt
    nxt += 1
    for v in vs:
        pairs.add((v, B))
    shared = 4                                 # one leaf of the first row also in the two others
    pairs |= {(2, shared), (3, shared)}
    ei = _edges(pairs, nxt)
    rows = _rows(ei, nxt)
    for i, v in enumerate(vs):
        assert rows[v][0] == A and rows[v][-1] == B and len(rows[v]) >= length + i
    _check(monkeypatch, ei, nxt)


def test_a_node_of_exactly_64_neighbours(monkeypatch):
    """Rows 32-63 take the high words of the row masks: triangles low-low, low-high and high-high among the neighbours, a
    common neighbour of the high rows alone, one of low and high rows, and a row of one entry."""
    pairs = {(0, v) for v in range(1, SMALL_DEG + 1)}
    pairs |= {(1, 2), (3, 40), (31, 32), (32, 33), (62, 63), (63, 64), (50, 64), (33, 64)}
    s = SMALL_DEG + 1
    pairs |= {(v, s) for v in range(33, 65)}            # high rows only
    pairs |= {(v, s + 1) for v in (2, 31, 32, 33, 64)}  # both halves
    pairs |= {(v, s + 2) for v in range(1, 65, 3)}
    n = s + 3
    ei = _edges(pairs, n)
    rows = _rows(ei, n)
    assert len(rows[0]) == SMALL_DEG and len(rows[5]) == 1
    _check(monkeypatch, ei, n)


def test_one_node_at_each_wave_class_weight_limit(monkeypatch):
    """W = the class limit, for each of the three, as a node of degree 1 (one row of W entries: every 64-piece step of the class
    is met, u in its first piece) and as a node of degree 64 (64 rows that share two common neighbours; private leaves fill the
    weight; u is the smallest id of every row).  All components of one graph."""
    pairs, nxt, want = set(), 0, []
    for lim in MAXW:
        u, v = nxt, nxt + 1
        nxt += 2
        pairs.add((u, v))
        for _ in range(lim - 1):
            pairs.add((v, nxt))
            nxt += 1
        want.append((u, 1, lim))
        u = nxt
        nb = list(range(nxt + 1, nxt + 1 + SMALL_DEG))
        s0, s1 = nxt + 1 + SMALL_DEG, nxt + 2 + SMALL_DEG
        nxt += SMALL_DEG + 3
        left = lim - 3 * SMALL_DEG
        for i, v in enumerate(nb):
            pairs |= {(u, v), (v, s0), (v, s1)}
            for _ in range(left // SMALL_DEG + (1 if i < left % SMALL_DEG else 0)):
                pairs.add((v, nxt))
                nxt += 1
        want.append((u, SMALL_DEG, lim))
    ei = _edges(pairs, nxt)
    rows = _rows(ei, nxt)
    for u, d, w in want:
        assert len(rows[u]) == d and _weight(rows, u) == w, (u, d, w)
    _check(monkeypatch, ei, nxt)


def test_a_neighbour_of_degree_1(monkeypatch):
    """Rows that are the single entry u, between rows that are not, at a node in the middle of the id range."""
    U = 40
    leaves, others = [3, 17, 41, 77, 78], [5, 39, 42, 60, 79]
    pairs = {(U, v) for v in leaves + others}
    nxt = 80
    for i, v in enumerate(others):
        pairs.add((v, 1))                      # a common neighbour below U
        pairs.add((v, 90))                     # and one above
        for _ in range(i):
            pairs.add((v, nxt))
            nxt += 1
    n = 91
    assert nxt <= 90
    ei = _edges(pairs, n)
    rows = _rows(ei, n)
    assert all(list(rows[v]) == [U] for v in leaves)
    _check(monkeypatch, ei, n)


def test_more_flagged_entries_than_the_queue_holds(monkeypatch):
    """The reverse slots are taken in sweep A and published after the last drain: H2_QCAP + 1 flagged entries at a node of 64
    rows of the lightest class (two rounds), and 2 x H2_QCAP + 1 at a node of three rows of the heaviest (three rounds, a long
    row): two components of one graph, nothing retried."""
    pairs = {(0, v) for v in range(1, SMALL_DEG + 1)}
    s = SMALL_DEG + 1
    total, counts = QCAP + 1, []
    while total > 0:
        c = min(SMALL_DEG, total)
        if total - c == 1:
            c -= 1
        counts.append(c)
        total -= c
    for c in counts:
        pairs |= {(s, v) for v in range(1, c + 1)}
        s += 1
    base = s
    length = MAXW[2] - QCAP - 64
    pairs |= {(base, base + 1), (base, base + 2), (base, base + 3)}
    pairs |= {(base + 1, base + 3 + p) for p in range(1, length)}
    pairs |= {(base + 2, base + 3 + 7 * p) for p in range(1, QCAP + 1)} | {(base + 3, base + 3 + 7)}
    n = base + length + 3
    ei = _edges(pairs, n)
    rows = _rows(ei, n)
    assert _queue_total(rows, 0) == QCAP + 1 and _weight(rows, 0) <= MAXW[0]
    assert MAXW[1] < _weight(rows, base) <= MAXW[2] and _queue_total(rows, base) == 2 * QCAP + 1
    _check(monkeypatch, ei, n)


# =====================================================================================================================
# the edge set's journal
# =====================================================================================================================
class Edited:
    """Three class-M nodes over 60 shared second neighbours, 30 leaves of its own each: x over nb[0:40], y over nb[20:60], z over
    nb[10:50] and y, pairs of the nb adjacent (triangles at every one of the three).  For the edges {z, nb[i]}, 20 <= i < 40, y
    is a triangle partner and x a candidate met in 30 rows: z's join asks the edge set whether x and y are adjacent.  The twin
    graphs are edited together, the edge list follows in a Python set."""

    def __init__(self, monkeypatch):
        nb = list(range(3, 63))
        self.x, self.y, self.z, self.nb = 0, 1, 2, nb
        pairs = {(0, v) for v in nb[0:40]} | {(1, v) for v in nb[20:60]} | {(2, v) for v in nb[10:50]} | {(1, 2)}
        pairs |= {(nb[2 * i], nb[2 * i + 1]) for i in range(30)}
        nxt = 63
        for hub in (0, 1, 2):
            pairs |= {(hub, nxt + i) for i in range(30)}
            nxt += 30
        for i, v in enumerate(nb):             # leaves, and second neighbours shared by two rows
            for _ in range(1 + i % 3):
                pairs.add((v, nxt))
                nxt += 1
            if i % 5 == 0 and i + 7 < 60:
                pairs |= {(v, nxt), (nb[i + 7], nxt)}
                nxt += 1
        self.n = nxt
        self.pairs = pairs
        ei = self.ei()
        deg = np.bincount(ei[0], minlength=self.n)
        for u in (0, 1, 2):                    # block class M: more than 64 neighbours, weight within the class
            assert SMALL_DEG < deg[u] and int(deg[ei[1][ei[0] == u]].sum()) <= 2 * MAXW[2]
        assert deg[3:].max() <= SMALL_DEG
        self.H, self.D = _twins(monkeypatch, ei, self.n)
        self.check('first pass', head=None)
        assert self.H.h2_stats()['units_m'] == 3
        self.check('second pass')

    def ei(self):
        return _edges(self.pairs, self.n)

    def add(self, a, b):
        self.H.add_edge(a, b)
        self.D.add_edge(a, b)
        self.pairs.add((min(a, b), max(a, b)))

    def remove(self, a, b):
        self.H.remove_edge(a, b)
        self.D.remove_edge(a, b)
        self.pairs.discard((min(a, b), max(a, b)))

    def check(self, what, head=STEADY):
        info, _ = _compare(self.H, self.D, self.ei(), self.n, what)
        if head is not None:
            assert {k: info[k] for k in head} == head, (what, info)

    def check_against_a_fresh_graph(self, monkeypatch, what):
        """The patched set against a rebuilt one: a new graph from the edited edge list builds its set from the rows."""
        from dcr.graph import DcrGraph
        monkeypatch.setenv('DCR_PASS', 'h2')
        F = DcrGraph(self.ei(), self.n)
        fu, fv, fc = F.curvature_all('bfc')
        hu, hv, hc = self.H.curvature_read()
        fo = np.argsort(np.minimum(fu, fv).astype(np.int64) * self.n + np.maximum(fu, fv))   # (the two list their edges in different orders)
        ho = np.argsort(np.minimum(hu, hv).astype(np.int64) * self.n + np.maximum(hu, hv))
        assert F.pass_engine() == 'two-hop' and np.array_equal(np.minimum(fu, fv)[fo], np.minimum(hu, hv)[ho]), what
        assert np.array_equal(np.maximum(fu, fv)[fo], np.maximum(hu, hv)[ho]), what
        assert np.array_equal(fc[fo].view(np.int64), hc[ho].view(np.int64)), what
        F.close()

    def close(self):
        self.H.close()
        self.D.close()


def test_an_added_edge_that_the_join_probes(monkeypatch):
    """x - y: x now meets y, a neighbour of z, so M_z(x) grows by one — and so does what the probes take off it again for the
    edges {z, nb[i]} that have y as a partner.  The values of those edges stay what they were only if the set answers yes."""
    g = Edited(monkeypatch)
    g.add(g.x, g.y)
    g.check('x - y added')
    g.check_against_a_fresh_graph(monkeypatch, 'x - y added')
    g.add(g.x, g.z)                                       # and a second one: x is now a partner at z, no candidate
    g.check('x - z added')
    g.close()


def test_a_tombstone_followed_by_a_re_insert(monkeypatch):
    g = Edited(monkeypatch)
    g.add(g.x, g.y)
    g.check('added')
    g.remove(g.x, g.y)
    g.add(g.x, g.y)                                       # both in one journal
    g.check('removed and added back between two passes')
    g.remove(g.x, g.y)
    g.check('removed')                                    # the tombstone alone: probes walk over it
    g.add(g.x, g.y)
    g.check('added back after a pass')
    g.remove(g.y, g.z)                                    # an edge of the first build
    g.add(g.y, g.z)
    g.remove(g.y, g.z)
    g.check('removed, added, removed')
    g.check_against_a_fresh_graph(monkeypatch, 'removed, added, removed')
    g.close()


def test_edits_that_do_not_happen(monkeypatch):
    g = Edited(monkeypatch)
    ne = g.H.number_of_edges()
    with pytest.raises(KeyError):
        g.H.remove_edge(g.x, g.y)                         # absent
    g.H.add_edge(g.y, g.z)                                # present
    assert g.H.number_of_edges() == ne
    g.check('nothing happened')
    g.add(g.x, g.y)
    g.H.add_edge(g.x, g.y)                                # present by now: journaled or not, the set holds it once
    g.remove(g.x, g.y)
    with pytest.raises(KeyError):
        g.H.remove_edge(g.x, g.y)
    g.check('an add, a repeated add, a removal, a repeated removal')
    g.check_against_a_fresh_graph(monkeypatch, 'edits that did not happen')
    g.close()


@pytest.mark.parametrize('extra', [0, 1])
def test_a_full_journal_and_one_edit_more(monkeypatch, extra):
    """EDIT_LOG_CAP edits between two passes are patched in; one more and the set is rebuilt beside the class kernels.  Either
    way the pass is one launch with the two plan kernels as its head, and the edits are gone from the journal afterwards: the
    pass after the next edit patches again."""
    g = Edited(monkeypatch)
    far = g.nb[40:40 + EDIT_LOG_CAP + extra - 1]            # rows of y and z, not of x
    g.add(g.x, g.y)
    for v in far:
        g.add(g.x, v)                                     # x gains rows that y and z read: more candidates and partners
    assert 1 + len(far) == EDIT_LOG_CAP + extra
    g.check('%d edits' % (EDIT_LOG_CAP + extra))
    g.check_against_a_fresh_graph(monkeypatch, 'journal')
    g.remove(g.x, g.y)
    g.check('one edit behind it')
    g.check('and none')
    g.close()


def test_a_refused_pass_followed_by_another(monkeypatch):
    """The means of tests/test_h2_head_gpu.py at a smaller size: twins that share exactly as many rows as a unit joins itself;
    one more shared row and the pass, launched without its triangle stage, is refused (status 4, nothing written) and launched
    again inside the same call.  The refused launch has applied the journal, the second finds nothing pending; the pass after the
    next edit patches the set again.  (The shared neighbours meet more keys twice than the lightest class's table holds: this
    graph uses the retry list from its first pass on, which is not what the case is about.)"""
    join_maxm = 256
    x, y, nb = 0, 1, list(range(2, 302))
    pairs = {(x, v) for v in nb} | {(y, v) for v in nb[:join_maxm]} | {(nb[2 * i], nb[2 * i + 1]) for i in range(20)}
    n = 302
    H, D = _twins(monkeypatch, _edges(pairs, n), n)

    def edit(op, a, b):
        getattr(H, op)(a, b)
        getattr(D, op)(a, b)
        (pairs.add if op == 'add_edge' else pairs.discard)((min(a, b), max(a, b)))

    info, stats = _compare(H, D, _edges(pairs, n), n, 'first', clean=False)
    assert stats['fallback'] == 0 and not info['triangle_stage'], (stats, info)
    info, stats = _compare(H, D, _edges(pairs, n), n, 'second', clean=False)
    assert info['launches'] == 1 and not info['triangle_stage'], info
    edit('add_edge', y, nb[join_maxm])
    info, stats = _compare(H, D, _edges(pairs, n), n, 'refused and launched again', clean=False)
    assert info['launches'] == 2 and info['triangle_stage'] and stats['fallback'] > 0, (info, stats)
    edit('add_edge', x, y)
    edit('remove_edge', y, nb[0])
    info, stats = _compare(H, D, _edges(pairs, n), n, 'the pass behind it', clean=False)
    assert {k: info[k] for k in STEADY} == STEADY, info
    edit('remove_edge', x, y)
    info, stats = _compare(H, D, _edges(pairs, n), n, 'steady again', clean=False)
    assert {k: info[k] for k in STEADY} == STEADY, info
    H.close()
    D.close()
