"""The exact-path queue of the two-hop engine's wave classes (h2s_node in csrc/dcr_bfc_h2.hip): the flagged entries of a node are
queued by LANE — one prefix over the lanes' flag counts gives each lane the queue indices of its own entries — and more than
H2_QCAP of them go in rounds cut by queue index.  Every case forces the engine with DCR_PASS=h2 and compares every edge's
curvature, bit for bit, with the node-centric engine on a twin graph (DCR_PASS=nc) and with the C oracle; the graphs are built
here, node by node, so that the node under test has the number of flagged entries the case names, and that number is counted
again with numpy from the edge list (occurrences of the 2-hop keys that occur more than once, plus the members of N(u) met in
the rows; u itself never counts).

Which lane owns which entry depends on where a row starts inside its aligned 16-byte piece, which the graph container decides:
the cases that want a lane's run of entries in a certain place are therefore run once per possible start (four), or once per
shift of the run (three), so that one of the runs meets the case whatever the layout is.

Not here: the block classes' copies of the queue loop (h2_node_fast, h2_for_pieces_queued) are unchanged, so there is no case
for class M's paths."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'discrete-curvature-rewiring_amd', 'csrc',
                    'dcr_bfc_h2.hip')


def _constants():
    """H2_QCAP, the wave classes' weight limits and their degree limit, read from the source."""
    src = open(_SRC).read()
    qcap = int(re.search(r'constexpr int H2_QCAP = (\d+);', src).group(1))
    deg = int(re.search(r'constexpr int H2_SMALL_DEG = (\d+);', src).group(1))
    m = re.search(r'h2_maxw\(int c\) \{ return c == 0 \? (\d+) : c == 1 \? (\d+) : c == 2 \? (\d+) :', src)
    return qcap, deg, tuple(int(x) for x in m.groups())


QCAP, SMALL_DEG, MAXW = _constants()


def _rows(ei, n):
    order = np.lexsort((ei[1], ei[0]))
    src, dst = ei[0][order], ei[1][order]
    ptr = np.searchsorted(src, np.arange(n + 1))
    return [dst[ptr[i]:ptr[i + 1]] for i in range(n)]


def _queue_total(rows, u):
    """Entries of node u that go to the exact path: occurrences of keys that occur more than once in the rows of u's
    neighbours, plus the members of N(u) met there (u itself is left out)."""
    keys = np.concatenate([rows[v] for v in rows[u]])
    keys = keys[keys != u]
    uniq, cnt = np.unique(keys, return_counts=True)
    return int(cnt[(cnt > 1) | np.isin(uniq, rows[u])].sum())


def _weight(rows, u):
    return int(sum(len(rows[v]) for v in rows[u]))


def _edges(pairs, n):
    from dcr import synthetic
    a = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    return synthetic.coalesced_edge_index(a[:, 0], a[:, 1], n)


def _check(monkeypatch, ei, n, no_retry=True):
    """One forced two-hop pass against the node-centric engine on a twin graph and against the C oracle, bit for bit."""
    from dcr.graph import DcrGraph
    from oracle import c_oracle
    monkeypatch.setenv('DCR_PASS', 'h2')
    H = DcrGraph(ei, n)
    monkeypatch.setenv('DCR_PASS', 'nc')
    D = DcrGraph(ei, n)
    monkeypatch.delenv('DCR_PASS')
    hu, hv, hc = H.curvature_all('bfc')
    assert H.pass_engine() == 'two-hop'
    info, stats = H.h2_launch_info(), H.h2_stats()
    assert info['launches'] >= 1
    if no_retry:
        assert stats['retry'] == 0 and not info['retry_stage'], (stats, info)
    du, dv, dc = D.curvature_all('bfc')
    assert D.pass_engine() == 'node-centric'
    ou, ov, oc = c_oracle.CGraph(ei, n).curv_all('bfc', nthreads=8)
    assert np.array_equal(hu, du) and np.array_equal(hv, dv) and np.array_equal(hu, ou) and np.array_equal(hv, ov)
    for name, ref in (('node-centric', dc), ('oracle', oc)):
        bad = np.flatnonzero(hc.view(np.int64) != ref.view(np.int64))
        assert bad.size == 0, (name, bad.size, hu[bad[:5]], hv[bad[:5]], hc[bad[:5]], ref[bad[:5]])
    H.close()
    D.close()


def _split_total(total, most):
    """`total` as a sum of counts between 2 and `most`: how many of u's neighbours each planted common neighbour gets."""
    counts = []
    while total > 0:
        c = min(most, total)
        if total - c == 1:  # (a planted node with ONE neighbour of u would not repeat)
            c -= 1
        counts.append(c)
        total -= c
    assert all(2 <= c <= most for c in counts)
    return counts


def _planted(counts, lead=0):
    """Node 0 with SMALL_DEG neighbours (1 .. SMALL_DEG) that share planted common neighbours and nothing else: planted node j
    is adjacent to the first counts[j] neighbours; `lead` more planted nodes are adjacent to the first two neighbours only.
    Every 2-hop key of node 0 repeats, so every entry of its sweep is flagged: Bloom collisions cannot add any."""
    pairs = [(0, v) for v in range(1, SMALL_DEG + 1)]
    s = SMALL_DEG + 1
    for c in list(counts) + [2] * lead:
        pairs += [(s, v) for v in range(1, c + 1)]
        s += 1
    return _edges(pairs, s), s


# ---- (a) no flagged entry, then one repeated key -----------------------------------------------------------------------
@pytest.mark.parametrize('forced', [False, True])
def test_no_flagged_entry_then_one_repeated_key(monkeypatch, forced):
    """A star of stars: no 2-hop key of node 0 repeats, the queue stays empty and the drain is never called.  Then ONE key is
    made to repeat (a leaf shared by two neighbours): two entries, the two occurrences of that key — the least a symmetric
    graph can queue, since a member of N(u) met in a row is met in its own row as well."""
    pairs, nxt = [], 6
    for v in range(1, 6):
        pairs.append((0, v))
        for _ in range(3):
            pairs.append((v, nxt))
            nxt += 1
    if forced:
        pairs.append((2, 6))  # node 6 is a leaf of neighbour 1
    ei = _edges(pairs, nxt)
    assert _queue_total(_rows(ei, nxt), 0) == (2 if forced else 0)
    _check(monkeypatch, ei, nxt)


# ---- (b) totals at the queue's capacity -----------------------------------------------------------------------------
@pytest.mark.parametrize('total', [QCAP, QCAP + 1, 2 * QCAP + 1])
def test_total_at_the_queue_capacity(monkeypatch, total):
    """Exactly H2_QCAP entries (one drain), one more (two), and 2 x H2_QCAP + 1 (three).  The node is of the lightest class,
    whose candidate list is shorter than 2 x H2_QCAP + 1: there the third round is followed by the retry list, by design, and
    only the two smaller totals assert that nothing was retried (the heaviest class's case below does for the largest)."""
    ei, n = _planted(_split_total(total, SMALL_DEG))
    rows = _rows(ei, n)
    assert len(rows[0]) == SMALL_DEG and _queue_total(rows, 0) == total and _weight(rows, 0) <= MAXW[0]
    _check(monkeypatch, ei, n, no_retry=total <= QCAP + 1)


def test_three_rounds_in_the_heaviest_wave_class(monkeypatch):
    """2 x H2_QCAP + 1 entries where the candidate list takes them: node 0 with three neighbours, a long row, a row of
    H2_QCAP keys out of it and a row with one of those (that key occurs three times).  Nothing is retried.  (The long row's
    other keys occur once; the few of them that the bitmaps flag by collision come on top of the counted total.)"""
    length = MAXW[2] - QCAP - 64
    pairs = [(0, 1), (0, 2), (0, 3)] + [(1, 3 + p) for p in range(1, length)]
    pairs += [(2, 3 + 7 * p) for p in range(1, QCAP + 1)] + [(3, 3 + 7)]
    n = length + 3
    ei = _edges(pairs, n)
    rows = _rows(ei, n)
    assert MAXW[1] < _weight(rows, 0) <= MAXW[2] and _queue_total(rows, 0) == 2 * QCAP + 1
    _check(monkeypatch, ei, n)


# ---- (c) one lane owns a long run; every lane owns one entry ----------------------------------------------------------
@pytest.mark.parametrize('start', [0, 1, 2, 3])
@pytest.mark.parametrize('cls', [0, 1, 2])
def test_one_lane_owns_a_whole_run(monkeypatch, cls, start):
    """Node 0 has two neighbours.  The row of the first is long (it fills the class's weight) and holds all the repeats: the
    second neighbour's row is made of the entries that ONE lane owns in the long row — four per 64-piece step, lane 37 — if the
    long row starts `start` entries into its first piece (one of the four values is the layout's).  That lane then queues a
    run of four entries per step of the row in one round, the lanes before it none; the other occurrences of the same keys
    are the second row's own.  In the heaviest class the total is H2_QCAP: a full round."""
    lane = 37
    length = MAXW[cls] - MAXW[cls] // 64 - 8    # the long row, node 0 included (the second row takes the rest of the weight)
    steps = (length + 255) // 256
    pos = [4 * (64 * q + lane) + j - start for q in range(steps) for j in range(4)]
    pos = [p for p in pos if 1 <= p < length]    # (position 0 of the row is node 0 itself)
    pairs = [(0, 1), (0, 2)] + [(1, 2 + p) for p in range(1, length)] + [(2, 2 + p) for p in pos]
    n = length + 2
    ei = _edges(pairs, n)
    rows = _rows(ei, n)
    assert len(rows[1]) == length and len(rows[2]) == len(pos) + 1
    w = _weight(rows, 0)
    assert (MAXW[cls - 1] if cls else 0) < w <= MAXW[cls]
    assert _queue_total(rows, 0) == 2 * len(pos) and len(pos) >= 4 * steps - 4
    if cls == 2:
        assert 2 * len(pos) == QCAP
    _check(monkeypatch, ei, n)


def test_every_lane_owns_one_entry(monkeypatch):
    """The mirror case: 64 neighbours, one planted common neighbour, one flagged entry in each row."""
    ei, n = _planted([SMALL_DEG])
    rows = _rows(ei, n)
    assert _queue_total(rows, 0) == SMALL_DEG and all(len(rows[v]) == 2 for v in rows[0])
    _check(monkeypatch, ei, n)


# ---- (d) a round boundary inside one lane's run -----------------------------------------------------------------------
@pytest.mark.parametrize('lead', [0, 1, 2])
def test_round_boundary_inside_a_run(monkeypatch, lead):
    """64 neighbours with three planted common neighbours each: in row order the runs are three entries long, so index
    H2_QCAP falls inside a run for at least two of the three shifts `lead` of all the runs, whichever lanes the layout gives
    the rows' pieces to: the lane's first index is below H2_QCAP and its last is not, and it goes on in the second round.
    (The totals reach the lightest class's candidate list: values only, the node may be redone from the retry list.)"""
    ei, n = _planted([SMALL_DEG] * 3, lead=lead)
    rows = _rows(ei, n)
    per_row = np.array([int(np.sum(rows[v] != 0)) for v in rows[0]])
    assert _queue_total(rows, 0) == int(per_row.sum()) == 3 * SMALL_DEG + 2 * lead > QCAP
    first = np.concatenate([[0], np.cumsum(per_row)[:-1]])
    last = first + per_row - 1
    straddles = int(np.sum((first < QCAP) & (last >= QCAP)))
    assert straddles == (1 if (QCAP - 2 * lead) % 3 else 0)   # in row order; two of the three values of `lead`
    _check(monkeypatch, ei, n, no_retry=False)


# ---- (e) the class limits -----------------------------------------------------------------------------------------------
def test_class_limits_degree_1_and_degree_64(monkeypatch):
    """W = the class limit - 1, the limit and the limit + 1, for each of the three limits, as a node of degree 1 (one row of W
    entries: every 64-piece step of the class is met, and a last piece that is only partly valid) and as a node of degree 64
    (64 rows that share two common neighbours: the repeats; private leaves fill the weight).  All components of one graph."""
    pairs, nxt = [], 0
    want = []
    for lim in MAXW:
        for w in (lim - 1, lim, lim + 1):
            u, v = nxt, nxt + 1                     # degree 1: u - v, v has w - 1 leaves more
            nxt += 2
            pairs.append((u, v))
            for _ in range(w - 1):
                pairs.append((v, nxt))
                nxt += 1
            want.append((u, 1, w))
            u = nxt                                 # degree 64
            nb = list(range(nxt + 1, nxt + 1 + SMALL_DEG))
            s0, s1 = nxt + 1 + SMALL_DEG, nxt + 2 + SMALL_DEG
            nxt += SMALL_DEG + 3
            left = w - 3 * SMALL_DEG               # every row has u and the two common neighbours
            for i, v in enumerate(nb):
                pairs += [(u, v), (v, s0), (v, s1)]
                for _ in range(left // SMALL_DEG + (1 if i < left % SMALL_DEG else 0)):
                    pairs.append((v, nxt))
                    nxt += 1
            want.append((u, SMALL_DEG, w))
    ei = _edges(pairs, nxt)
    rows = _rows(ei, nxt)
    for u, d, w in want:
        assert len(rows[u]) == d and _weight(rows, u) == w, (u, d, w)
    _check(monkeypatch, ei, nxt)


# ---- (f) a dense small graph forced onto the engine ---------------------------------------------------------------------
def test_dense_preferential_attachment_graph(monkeypatch):
    """Nearly every key repeats: many rounds per node, full tables, nodes on the retry list.  Values only — and that the
    two-hop pass itself ended with status 0 after its retries (pass_engine() names another engine otherwise)."""
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(2500, 10, seed=11)
    _check(monkeypatch, ei, n, no_retry=False)
