"""What the two sweeps of the two-hop engine's wave classes (h2s_node in csrc/dcr_bfc_h2.hip) hand to each other and carry from
one 64-piece step to the next: sweep A takes u's own entry out of a piece's valid mask, which sweep B then reads as it stands;
the hashes of both sweeps are bit fields of one product, and an entry that does not count takes mask 0 without a branch of its
own.  Every case forces the engine with DCR_PASS=h2 and compares every edge's curvature, bit for bit, with the node-centric
engine on a twin graph (DCR_PASS=nc) and with the C oracle, and asserts that nothing was retried or sent down the fallback
path unless the case says so.

The graphs are planted node by node.  A node under test u gets its rows (the rows of its neighbours) from a list of
(leaves below u, leaves above u, shared keys below u, shared keys above u): rows are kept in ascending order of the ids, so the
entries below u decide where u sits in the row, and the order of the list is the order of the rows in the piece list.  Where a
row starts inside its aligned 16-byte piece is the graph container's decision: every case is run for four `shift`s — node 0 is
given 1 + shift neighbours (the last nodes of the graph), which moves the start of every later row by one slot per shift — so
that each case meets every alignment whatever the layout is.

Not here: the block classes (their copies of the sweeps are unchanged)."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'discrete-curvature-rewiring_amd', 'csrc',
                    'dcr_bfc_h2.hip')


def _constants():
    """H2_QCAP, the wave classes' weight limits, their degree limit and their exact-table sizes, read from the source."""
    src = open(_SRC).read()
    qcap = int(re.search(r'constexpr int H2_QCAP = (\d+);', src).group(1))
    deg = int(re.search(r'constexpr int H2_SMALL_DEG = (\d+);', src).group(1))
    m = re.search(r'h2_maxw\(int c\) \{ return c == 0 \? (\d+) : c == 1 \? (\d+) : c == 2 \? (\d+) :', src)
    e = re.search(r'h2_exs\(int c\) \{ return c == 0 \? (\d+) : c == 1 \? (\d+) : c == 2 \? (\d+) :', src)
    return qcap, deg, tuple(int(x) for x in m.groups()), tuple(int(x) for x in e.groups())


QCAP, SMALL_DEG, MAXW, EXS = _constants()
STEPS = tuple(w // 256 + 1 for w in MAXW)   # 64-piece steps of a class: a row of MAXW entries that starts inside a piece


class _Planter:
    def __init__(self, shift):
        self.pairs, self.n, self.shift = [], 1, shift   # node 0: the hub that shifts the layout

    def new(self):
        self.n += 1
        return self.n - 1

    def node(self, rows, low_keys=0, high_keys=0):
        """A node u whose i-th row holds rows[i] = (leaves below u, leaves above u, indices of shared keys below u, indices of
        shared keys above u).  Returns u."""
        lows = [[self.new() for _ in range(r[0])] for r in rows]
        lk = [self.new() for _ in range(low_keys)]
        u = self.new()
        vs = [self.new() for _ in rows]
        hk = [self.new() for _ in range(high_keys)]
        for v, r, lo in zip(vs, rows, lows):
            self.pairs.append((u, v))
            self.pairs += [(v, x) for x in lo] + [(v, lk[i]) for i in r[2]] + [(v, hk[i]) for i in r[3]]
            self.pairs += [(v, self.new()) for _ in range(r[1])]
        return u

    def graph(self):
        from dcr import synthetic
        self.pairs += [(0, self.new()) for _ in range(1 + self.shift)]
        a = np.array(self.pairs, dtype=np.int64).reshape(-1, 2)
        return synthetic.coalesced_edge_index(a[:, 0], a[:, 1], self.n), self.n


def _rows(ei, n):
    order = np.lexsort((ei[1], ei[0]))
    src, dst = ei[0][order], ei[1][order]
    ptr = np.searchsorted(src, np.arange(n + 1))
    return [dst[ptr[i]:ptr[i + 1]] for i in range(n)]


def _row_starts(ei, n):
    """The slot at which the graph container starts each row: rows follow each other in node order, each with its degree plus
    a slack of max(8, degree // 4) slots (slack_for in csrc/dcr_graph.hip, mirrored here for the one case that leans on the
    layout: it asserts what it needs, so a container that lays rows out differently fails the case instead of hollowing it)."""
    deg = np.bincount(ei[0], minlength=n)
    cap = deg + np.maximum(8, deg // 4)
    return np.concatenate([[0], np.cumsum(cap)[:-1]])


def _weight(rows, u):
    return int(sum(len(rows[v]) for v in rows[u]))


def _in_class(rows, u, cls):
    w = _weight(rows, u)
    return (MAXW[cls - 1] if cls else 0) < w <= MAXW[cls] and len(rows[u]) <= SMALL_DEG


def _queue_total(rows, u):
    """Entries of node u that go to the exact path for certain: occurrences of keys that occur more than once in the rows of
    u's neighbours, plus the members of N(u) met there (u itself is left out).  Keys that occur once and are flagged by a
    collision in the bitmaps come on top."""
    keys = np.concatenate([rows[v] for v in rows[u]])
    keys = keys[keys != u]
    uniq, cnt = np.unique(keys, return_counts=True)
    return int(cnt[(cnt > 1) | np.isin(uniq, rows[u])].sum())


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
    assert info['launches'] >= 1 and stats['fallback'] == 0, (stats, info)
    if no_retry:
        assert stats['retry'] == 0 and not info['retry_stage'], (stats, info)
    else:
        assert stats['retry'] > 0 or info['retry_stage'], (stats, info)
    du, dv, dc = D.curvature_all('bfc')
    assert D.pass_engine() == 'node-centric'
    ou, ov, oc = c_oracle.CGraph(ei, n).curv_all('bfc', nthreads=8)
    assert np.array_equal(hu, du) and np.array_equal(hv, dv) and np.array_equal(hu, ou) and np.array_equal(hv, ov)
    for name, ref in (('node-centric', dc), ('oracle', oc)):
        bad = np.flatnonzero(hc.view(np.int64) != ref.view(np.int64))
        assert bad.size == 0, (name, bad.size, hu[bad[:5]], hv[bad[:5]], hc[bad[:5]], ref[bad[:5]])
    H.close()
    D.close()


def _pad_row(rows, cls):
    """One more row of leaves above u that brings the weight to the class's limit."""
    used = sum(1 + r[0] + r[1] + len(r[2]) + len(r[3]) for r in rows)
    assert used + 1 <= MAXW[cls]
    return (0, MAXW[cls] - used - 1, (), ())


# ---- u at each position of a piece ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 1, 2, 3])
@pytest.mark.parametrize('cls', [0, 1, 2])
def test_u_at_each_piece_position(monkeypatch, cls, shift):
    """u with 0 .. 8 entries below it and 0, 1 or 5 above it in a row: u at each of the four positions of a piece for every
    start of the row, alone in its row (the only valid entry of its piece), in the first and the last piece of a row, and as
    the only valid entry of a row's last piece.  Sweep A drops exactly that entry from the piece's mask; the entries beside it
    are still marked and still read in sweep B.  Two keys are shared by the rows, so entries beside u are flagged too."""
    rows = [(p, h, (), (0, 1) if (p + h) % 3 == 0 else ()) for p in range(9) for h in (0, 1, 5)]
    rows.append(_pad_row(rows, cls))
    g = _Planter(shift)
    u = g.node(rows, high_keys=2)
    ei, n = g.graph()
    r = _rows(ei, n)
    assert _in_class(r, u, cls) and _queue_total(r, u) == 2 * 9
    assert {int(np.searchsorted(r[v], u)) for v in r[u]} == set(range(9))
    _check(monkeypatch, ei, n)


# ---- u's piece at a step boundary -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 1, 2, 3])
def test_u_piece_at_a_step_boundary(monkeypatch, shift):
    """Nodes of degree 1: one long row with u at a chosen position.  Positions 244 .. 263 put u's piece at index 62, 63, 64
    and 65 of the piece list for every start of the row (the boundary between the first two 64-piece steps, where the row
    search changes its bracket and `meta` its register); the last eight positions of a row of the class's largest weight put
    it at 64 q - 1 and, when the row starts inside a piece, at 64 q for the last step q of each class.  All in one graph."""
    g = _Planter(shift)
    us = []
    for p in range(244, 264):
        us.append((g.node([(p, 400 - p - 1, (), ())]), 0, p))
    for cls in (0, 1, 2):
        for p in range(MAXW[cls] - 8, MAXW[cls]):
            us.append((g.node([(p, MAXW[cls] - p - 1, (), ())]), cls, p))
    ei, n = g.graph()
    r = _rows(ei, n)
    for u, cls, p in us:
        assert _in_class(r, u, cls) and len(r[u]) == 1 and int(np.searchsorted(r[r[u][0]], u)) == p
    assert (MAXW[2] - 1) // 4 == 64 * (STEPS[2] - 1) - 1
    _check(monkeypatch, ei, n)


# ---- steps with two kinds of row --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 1, 2, 3])
@pytest.mark.parametrize('where', ['last', 'first', 'middle'])
def test_many_short_rows_and_one_long_row(monkeypatch, where, shift):
    """63 rows of 4 .. 11 entries (one to four pieces each: the first steps hold twenty rows and more, bracketed by bisection)
    and one row that takes the rest of the class's weight and spans several steps (steps of one row: the bracket is empty).
    The long row comes last, first, or in the middle — a step then starts in a short row, runs into the long one, and a later
    step leaves it for short rows again.  One node per class in one graph; three keys are shared by some short rows and the
    long one."""
    g = _Planter(shift)
    us = []
    for cls in (0, 1, 2):
        short = [(i % 3, 3 + i % 5, (), (i % 3,) if i % 7 == 0 else ()) for i in range(63)]
        at = {'last': 63, 'first': 0, 'middle': 31}[where]
        used = sum(1 + r[0] + r[1] + len(r[3]) for r in short)
        long_row = (2, MAXW[cls] - used - 6, (), (0, 1, 2))
        us.append((g.node(short[:at] + [long_row] + short[at:], high_keys=3), cls))
    ei, n = g.graph()
    r = _rows(ei, n)
    for u, cls in us:
        assert _in_class(r, u, cls) and _weight(r, u) == MAXW[cls] and len(r[u]) == SMALL_DEG
        assert max(len(r[v]) for v in r[u]) > 2 * 256
    _check(monkeypatch, ei, n)


# ---- singletons and repeats together ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 1, 2, 3])
@pytest.mark.parametrize('cls', [0, 1, 2])
def test_repeats_across_steps_and_inside_one_instruction(monkeypatch, cls, shift):
    """Rows at the two ends of the piece list with a long row of keys that occur once between them.  Key 0: once in the first
    step, once in the last; key 1: once in the first step, twice in the last; key 2: in the long row and in the last step;
    key 3: twice in the first step, once in the last.  Low keys 0 and 1 sit at the same place of four and of two rows of four
    entries that follow each other (rows of four entries with their slack start alike): the same key in neighbouring lanes of
    ONE atomic instruction, of which only the later-served ones see both bits set."""
    rows = [(1, 1, (0,), ())] * 4 + [(1, 1, (1,), ())] * 2
    rows += [(0, 2, (), (3,)), (1, 3, (), (0, 1, 3))]
    tail = [(1, 3, (), (0, 1, 2, 3)), (0, 2, (), (1,))]
    used = sum(1 + r[0] + r[1] + len(r[2]) + len(r[3]) for r in rows + tail)
    rows += [(0, MAXW[cls] - used - 2, (), (2,))] + tail
    g = _Planter(shift)
    u = g.node(rows, low_keys=2, high_keys=4)
    ei, n = g.graph()
    r = _rows(ei, n)
    assert _in_class(r, u, cls) and _weight(r, u) == MAXW[cls]
    assert _queue_total(r, u) == 4 + 2 + 2 + 3 + 2 + 3
    # the low keys sit at the same entry position of their pieces in the four (two) rows, whose pieces are the first of the
    # piece list and so of one 64-piece step: the same key in neighbouring lanes of one atomic instruction
    start = _row_starts(ei, n)
    for vs in (r[u][:4], r[u][4:6]):
        key = [int(x) for x in r[vs[0]] if x != u and all(x in r[v] for v in vs)]
        assert len(key) == 1 and all(len(r[v]) == 4 for v in vs)
        assert len({int(start[v] + np.searchsorted(r[v], key[0])) % 4 for v in vs}) == 1
    _check(monkeypatch, ei, n)


# ---- flagged counts around the queue's capacity -----------------------------------------------------------------------------
def _split_total(total, most):
    counts = []
    while total > 0:
        c = min(most, total)
        if total - c == 1:  # (a planted key in ONE row would not repeat)
            c -= 1
        counts.append(c)
        total -= c
    assert all(2 <= c <= most for c in counts)
    return counts


def _planted_rows(total, weight):
    """64 rows that share planted keys, each key held by up to eight rows that follow each other (every occurrence is flagged:
    in each key's run the first-served occurrence only through B2, the others by their own atomic), and leaves that fill the
    weight.  The keys go round the rows, so that no row holds many of them: a row's own node meets every holder of its keys
    twice, and with a key in all 64 rows THAT node's candidate list would fill."""
    counts = _split_total(total, 8)
    per = [[] for _ in range(SMALL_DEG)]
    at = 0
    for j, c in enumerate(counts):
        for t in range(c):
            per[(at + t) % SMALL_DEG].append(j)
        at += c
    left = weight - SMALL_DEG - total
    assert left >= 0
    share = [left // SMALL_DEG + (1 if i < left % SMALL_DEG else 0) for i in range(SMALL_DEG)]
    below = [min(i % 2, share[i]) for i in range(SMALL_DEG)]   # (u is not the first entry of every row)
    return [(below[i], share[i] - below[i], (), tuple(per[i])) for i in range(SMALL_DEG)], len(counts)


@pytest.mark.parametrize('shift', [0, 2])
@pytest.mark.parametrize('cls', [0, 1, 2])
def test_flagged_counts_around_the_queue_capacity(monkeypatch, cls, shift):
    """0, 2 (the least a symmetric graph can plant: one flagged entry alone cannot be), H2_QCAP - 1, H2_QCAP, H2_QCAP + 1
    and 2 x H2_QCAP + 1 (three rounds) planted flagged entries, one node each, all in one graph per class.  In the lightest
    class the weight is the planted total and the counts are exact; in the other two the leaves that fill the weight occur once
    and the few of them the bitmaps flag by collision come on top.  The lightest class's candidate list is shorter than
    2 x H2_QCAP + 1: that node is planted in a graph of its own below."""
    g = _Planter(shift)
    us = []
    for total in (0, 2, QCAP - 1, QCAP, QCAP + 1, 2 * QCAP + 1):
        if cls == 0 and total > 2 * QCAP:
            continue
        weight = SMALL_DEG + max(total, 1) if cls == 0 else MAXW[cls]
        rows, nkeys = _planted_rows(total, weight)
        us.append((g.node(rows, high_keys=nkeys), total, weight))
    ei, n = g.graph()
    r = _rows(ei, n)
    for u, total, weight in us:
        assert _in_class(r, u, cls) and _weight(r, u) == weight and _queue_total(r, u) == total
    _check(monkeypatch, ei, n)


def test_three_rounds_in_the_lightest_class_are_redone(monkeypatch):
    """2 x H2_QCAP + 1 flagged entries in the lightest class: three rounds of the queue, then the candidate list is full, the
    node is not published and is redone from the retry list — with the right values."""
    g = _Planter(1)
    rows, nkeys = _planted_rows(2 * QCAP + 1, SMALL_DEG + 2 * QCAP + 1)
    u = g.node(rows, high_keys=nkeys)
    ei, n = g.graph()
    r = _rows(ei, n)
    assert _in_class(r, u, 0) and _queue_total(r, u) == 2 * QCAP + 1
    _check(monkeypatch, ei, n, no_retry=False)


# ---- the class limits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 1, 2, 3])
def test_class_limits_degree_1_and_degree_64(monkeypatch, shift):
    """Weights at each class's limit and one above it (the next class, or class M above the last), as a node of degree 1 —
    one row, u in the middle of it — and as a node of degree 64 whose rows share two keys.  All in one graph."""
    g = _Planter(shift)
    us = []
    for lim in MAXW:
        for w in (lim, lim + 1):
            us.append((g.node([(w // 2, w - w // 2 - 1, (), ())]), 1, w))
            left = w - 3 * SMALL_DEG
            rows = [(i % 4, left // SMALL_DEG + (1 if i < left % SMALL_DEG else 0) - i % 4, (), (0, 1)) for i in range(SMALL_DEG)]
            us.append((g.node(rows, high_keys=2), SMALL_DEG, w))
    ei, n = g.graph()
    r = _rows(ei, n)
    for u, d, w in us:
        assert len(r[u]) == d and _weight(r, u) == w, (u, d, w)
    _check(monkeypatch, ei, n)


# ---- one node whose exact table fills ---------------------------------------------------------------------------------------
def test_a_node_whose_exact_table_fills_is_redone(monkeypatch):
    """64 neighbours and more planted keys, two rows each, than the lightest class's exact table has slots left beside the
    neighbours: the table fills in the drain, nothing of the node is published (its reverse slots and the masks sweep A
    rewrote included), and the retry stage computes it again."""
    nkeys = EXS[0] - SMALL_DEG + 6
    per = [[] for _ in range(SMALL_DEG)]
    for j in range(nkeys):
        per[(2 * j) % SMALL_DEG].append(j)
        per[(2 * j + 1) % SMALL_DEG].append(j)
    g = _Planter(0)
    u = g.node([(i % 3, 1, (), tuple(per[i])) for i in range(SMALL_DEG)], high_keys=nkeys)
    ei, n = g.graph()
    r = _rows(ei, n)
    assert _in_class(r, u, 0) and _queue_total(r, u) == 2 * nkeys
    _check(monkeypatch, ei, n, no_retry=False)
