"""The triangle stage of the two-hop pass (the k_h2_triangles launches of csrc/dcr_bfc_h2.hip) is speculative: a graph none of
whose passes had a block-class unit on the probe path is launched without it, k_h2_final refuses to write when a unit listed for
the stage after all (DevResult::h2_status 4), and the host runs the pass again with the stage and keeps it for the graph
(dcr_graph::h2_expect_triangles) — the same arrangement as for the retry stage (status 3).  Each test builds, with numpy, the
smallest graph that reaches the case (checked on the CPU against a restatement of h2_classify), reads how the pass was launched
through DcrGraph.h2_launch_info() and compares every edge's curvature bit for bit with the C oracle (curvature/bfc_naive.py:7-40).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the limits of h2_classify / h2_parts_for and of the class tables (csrc/dcr_bfc_h2.hip)
SMALL_DEG, MAXW0, MAXW1, MAXW2, MAXW3, KEYCAP3, KEYCAP4, L1_SPLIT = 64, 1024, 2048, 4096, 8192, 2800, 5500, 17
EXS0 = 128               # slots of class 0's exact table (h2_exs(0))
FAST_ROWS = 256          # h2_node_fast: at most 64 rows per wave, 4 waves
H2_ITEMS = 2048          # exact-path items a wave's list holds
JOIN_MAXM = 256          # rows one key may occur in for a unit to join its triangle term itself
HOST_LOOP = 6            # launches the host loop of dcr_bfc.hip adds to the first one at most


def classify(d, S):
    """(class, partitions) of a node with d neighbours whose degrees sum to S."""
    if d <= SMALL_DEG and S <= MAXW2:
        return (0 if S <= MAXW0 else 1 if S <= MAXW1 else 2), 1
    if S <= MAXW3 and d + S // 4 <= KEYCAP3:
        return 3, 1
    room = KEYCAP4 - d
    if room <= 0:
        return 4, 65536
    keys = S // 3 + 64
    per = (1 << L1_SPLIT) // 8
    return 4, max(1, -(-keys // room), -(-S // per))


def degrees(ei, n):
    deg = np.bincount(ei[0], minlength=n)
    S = np.bincount(ei[0], weights=deg[ei[1]], minlength=n).astype(np.int64)
    return deg, S


def adjacency(ei):
    adj = {}
    for a, c in zip(ei[0].tolist(), ei[1].tolist()):
        adj.setdefault(a, set()).add(c)
    return adj


def most_rows_of_a_key(adj, u):
    """The largest number of rows of u one candidate (a second neighbour outside N(u)) occurs in."""
    cnt = {}
    for k in adj[u]:
        for w in adj[k]:
            if w != u and w not in adj[u]:
                cnt[w] = cnt.get(w, 0) + 1
    return max(cnt.values()) if cnt else 0


class Builder:
    def __init__(self, seed):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.src, self.dst = [], []
        self.n = 0

    def nodes(self, k):
        ids = np.arange(self.n, self.n + k)
        self.n += k
        return ids

    def edge(self, a, b):
        self.src.append(int(a))
        self.dst.append(int(b))

    def star(self, centre, leaves):
        for v in leaves:
            self.edge(centre, v)

    def edges_of(self, ei, offset):
        """Another graph's edges, its node i as node offset + i."""
        keep = ei[0] < ei[1]
        self.src += (ei[0][keep] + offset).tolist()
        self.dst += (ei[1][keep] + offset).tolist()

    def large_node(self, D, pool, extra, triangles):
        """A node with D neighbours: a clique of 6 and a few more triangles among them, second neighbours shared by 2, 3 and 40
        rows (adjacent rows and not), leaves, and `extra` random second neighbours per remaining row out of `pool`.  (The pools
        are wide and the shared second neighbours few: a neighbour of the node is a wave-class node, and every key it meets in
        two rows takes a slot of its exact table — with 70 shared rows and a pool of 300 some went to the retry list.)"""
        x = int(self.nodes(1)[0])
        nb = self.nodes(D)
        self.star(x, nb)
        for a in range(6):
            for b in range(a + 1, 6):
                self.edge(nb[a], nb[b])
        for a, b in ((6, 7), (8, 9), (10, 11), (11, 12)):
            self.edge(nb[a], nb[b])
        s = self.nodes(4)
        self.star(s[0], nb[[6, 7]])                       # two adjacent rows: the count goes to 0
        self.star(s[1], nb[[20, 21]])                     # two rows, not adjacent: it stays
        self.star(s[2], nb[[10, 11, 12]])                 # a path: the middle row loses both
        self.star(s[3], nb[0:40])                         # many rows, the clique among them
        for i in range(50, D):                            # (nb[40:50] stay leaves)
            self.star(nb[i], self.rng.choice(pool, size=int(self.rng.integers(extra[0], extra[1])), replace=False))
        for _ in range(triangles):
            a, b = self.rng.integers(50, D, size=2)
            self.edge(nb[a], nb[b])
        return x

    def twins(self, rows_x, rows_y):
        """Two nodes that are not adjacent: x with rows_x neighbours, y with the first rows_y of them — each a candidate key in
        rows_y rows of the other — and triangles at both, so that the candidates lose counts."""
        x, y = (int(v) for v in self.nodes(2))
        nb = self.nodes(rows_x)
        self.star(x, nb)
        self.star(y, nb[:rows_y])
        for i in range(20):
            self.edge(nb[2 * i], nb[2 * i + 1])
        return x, y, nb

    def edge_index(self):
        from dcr import synthetic
        return synthetic.coalesced_edge_index(np.array(self.src), np.array(self.dst), self.n), self.n


@pytest.fixture()
def h2graph(monkeypatch):
    monkeypatch.setenv('DCR_PASS', 'h2')
    from dcr.graph import DcrGraph
    return DcrGraph


def check(G, ei, n):
    """Every edge against the oracle, bit for bit; returns the pass's diagnostics and how it was launched."""
    from oracle import c_oracle
    eu, ev, cv = G.curvature_all('bfc')
    assert G.pass_engine() == 'two-hop'
    oc = c_oracle.CGraph(ei, n).curv_edges(eu, ev, 'bfc', nthreads=8)
    assert len(eu) == ei.shape[1] // 2
    bad = np.flatnonzero(cv.view(np.int64) != oc.view(np.int64))
    assert bad.size == 0, (bad.size, eu[bad[:5]], ev[bad[:5]], cv[bad[:5]], oc[bad[:5]])
    st, info = G.h2_stats(), G.h2_launch_info()
    print(st, info)
    return st, info


def joining_graph(seed, twin_rows=None):
    """Class-M nodes at both ends of the register path and beyond it, and a split hub of three or more partitions; no candidate
    key in more than JOIN_MAXM rows.  twin_rows: also a pair of twins sharing that many neighbours."""
    b = Builder(seed)
    pool = b.nodes(900)
    mids = [b.large_node(D, pool, (2, 9), D // 8) for D in (65, FAST_ROWS, 280)]
    rest = b.nodes(1600)                      # a sparse background: the second neighbours have neighbours of their own
    for v in pool:
        b.star(v, b.rng.choice(rest, size=2, replace=False))
    for v in rest[::2]:
        b.edge(v, b.rng.choice(rest))
    hub = b.large_node(1000, b.nodes(12000), (24, 34), 600)
    tw = b.twins(300, twin_rows) if twin_rows else None
    ei, n = b.edge_index()
    deg, S = degrees(ei, n)
    adj = adjacency(ei)
    for x in mids:
        assert classify(int(deg[x]), int(S[x])) == (3, 1), (deg[x], S[x])
    assert [int(deg[x]) for x in mids] == [65, FAST_ROWS, 280]
    cls, nparts = classify(int(deg[hub]), int(S[hub]))
    assert cls == 4 and nparts >= 3, (deg[hub], S[hub], nparts)
    big = [u for u in range(n) if classify(int(deg[u]), int(S[u]))[0] >= 3]
    assert max(most_rows_of_a_key(adj, u) for u in big) <= JOIN_MAXM
    if tw:
        x, y, _ = tw
        assert classify(int(deg[x]), int(S[x])) == (3, 1) and classify(int(deg[y]), int(S[y])) == (3, 1)
        assert most_rows_of_a_key(adj, x) == twin_rows and most_rows_of_a_key(adj, y) == twin_rows
    return ei, n, tw


def test_no_fallback_no_stage(h2graph):
    ei, n, _ = joining_graph(seed=1)
    assert n < 17000
    G = h2graph(ei, n)
    for _ in range(2):
        st, info = check(G, ei, n)
        assert st['fallback'] == 0 and st['ncand'] == (0, 0) and st['units_m'] >= 3 and st['units_split'] >= 3, st
        assert info == {'launches': 1, 'retry_stage': False, 'triangle_stage': False}, info


def fallback_on_the_first_pass(h2graph, ei, n):
    G = h2graph(ei, n)
    st, info = check(G, ei, n)
    assert st['fallback'] > 0, st
    assert info['launches'] == 2 and info['triangle_stage'], info
    st, info = check(G, ei, n)
    assert st['fallback'] > 0, st
    assert info['launches'] == 1 and info['triangle_stage'], info


def test_key_in_more_rows_than_the_join_takes_brings_the_stage(h2graph):
    b = Builder(5)
    x, y, nb = b.twins(300, 300)
    z = int(b.nodes(1)[0])
    b.star(z, nb[:100])
    ei, n = b.edge_index()
    deg, S = degrees(ei, n)
    adj = adjacency(ei)
    for v in (x, y):
        assert classify(int(deg[v]), int(S[v])) == (3, 1) and most_rows_of_a_key(adj, v) == 300 > JOIN_MAXM
    fallback_on_the_first_pass(h2graph, ei, n)


def test_overflowed_item_list_brings_the_stage(h2graph):
    """A hub whose neighbours are joined among themselves: every wave meets more members of N(u) in its rows than its item list
    holds.  The neighbours stay class-M nodes with a few hundred keys and the other second neighbours have one row each, so that no
    table fills: the triangle stage is the only one the first launch lacks."""
    b = Builder(4)
    pool = b.nodes(3000)
    D = 800
    x = int(b.nodes(1)[0])
    nb = b.nodes(D)
    b.star(x, nb)
    up = np.triu(b.rng.random((D, D)) < 0.1025, 1)
    for a, c in zip(*np.nonzero(up)):
        b.edge(nb[a], nb[c])
    for v in nb:
        b.star(v, b.rng.choice(pool, size=3, replace=False))
    ei, n = b.edge_index()
    deg, S = degrees(ei, n)
    assert classify(int(deg[x]), int(S[x]))[0] == 4
    assert np.median([classify(int(deg[v]), int(S[v]))[0] for v in nb]) == 3
    assert (int(S[x]) - 4 * D) // 16 > 2 * H2_ITEMS   # members of N(x) in the rows of one wave of the 16
    fallback_on_the_first_pass(h2graph, ei, n)


def test_an_edit_flips_the_expectation(h2graph):
    """Twins at exactly JOIN_MAXM common rows join; one edge added through the graph's edit call (journaled, applied to the edge
    set by k_h2_eset_apply in the launch that is then refused) makes it JOIN_MAXM + 1."""
    from dcr import synthetic
    ei, n, (x, y, nb) = joining_graph(seed=1, twin_rows=JOIN_MAXM)
    G = h2graph(ei, n)
    st, info = check(G, ei, n)
    assert st['fallback'] == 0, st
    # (the neighbours the twins share are class-0 nodes that meet JOIN_MAXM keys twice, more than their table holds: this graph
    #  needs the retry stage from its first pass on, whatever the triangle stage does)
    assert st['retry'] > 0 and info['retry_stage'] and not info['triangle_stage'], info
    st, info = check(G, ei, n)
    assert info == {'launches': 1, 'retry_stage': True, 'triangle_stage': False}, info
    G.add_edge(int(y), int(nb[JOIN_MAXM]))
    ei2 = synthetic.coalesced_edge_index(np.r_[ei[0], int(y)], np.r_[ei[1], int(nb[JOIN_MAXM])], n)
    assert ei2.shape[1] == ei.shape[1] + 2
    adj = adjacency(ei2)
    assert most_rows_of_a_key(adj, x) == JOIN_MAXM + 1 and most_rows_of_a_key(adj, y) == JOIN_MAXM + 1
    st, info = check(G, ei2, n)
    assert st['fallback'] >= 2, st
    assert info['launches'] == 2 and info['triangle_stage'], info
    st, info = check(G, ei2, n)
    assert info['launches'] == 1 and info['triangle_stage'], info


def test_both_stages_missing_at_once(h2graph):
    """A fresh graph that needs the retry list and has a unit on the probe path.  The retry list: a class-0 node (weight at most
    1,024) with more keys than its exact table has slots — its 40 neighbours and 150 second neighbours in two rows each — beside
    the dense power-law graph of tests/test_h2_engine_gpu.py whose wave classes' tables fill.  The probe path: twins sharing 300
    neighbours."""
    from dcr import synthetic
    b = Builder(7)
    u = int(b.nodes(1)[0])
    nb = b.nodes(40)
    b.star(u, nb)
    second = b.nodes(150)
    for j, w in enumerate(second):
        b.star(w, nb[[(3 * j) % 40, (3 * j + 7) % 40]])
    x, y, _ = b.twins(300, 300)
    ei_pl, n_pl = synthetic.powerlaw_graph(2500, 10, seed=11)
    b.edges_of(ei_pl, int(b.nodes(n_pl)[0]))
    ei, n = b.edge_index()
    assert n < 10000
    deg, S = degrees(ei, n)
    adj = adjacency(ei)
    assert classify(int(deg[u]), int(S[u])) == (0, 1), (deg[u], S[u])
    twice = {}
    for k in adj[u]:
        for w in adj[k]:
            if w != u:
                twice[w] = twice.get(w, 0) + 1
    assert len(adj[u]) + sum(1 for c in twice.values() if c >= 2) > EXS0
    assert classify(int(deg[x]), int(S[x])) == (3, 1) and most_rows_of_a_key(adj, x) > JOIN_MAXM
    G = h2graph(ei, n)
    st, info = check(G, ei, n)
    assert st['retry'] > 0 and st['fallback'] > 0, st
    assert info['retry_stage'] and info['triangle_stage'] and 2 <= info['launches'] <= 1 + HOST_LOOP, info
    st, info = check(G, ei, n)
    assert info == {'launches': 1, 'retry_stage': True, 'triangle_stage': True}, info


def test_every_layout_slot(h2graph):
    """The smallest power-law graph of the generator's (10 edges per new node) with units in all five classes: a kernel that the
    stream layout forks or joins wrongly leaves records missing."""
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(2000, 10, seed=3)
    deg, S = degrees(ei, n)
    per_class = np.bincount([classify(int(d), int(s))[0] for d, s in zip(deg, S) if d > 0], minlength=5)
    assert np.all(per_class > 0), per_class
    st, info = check(h2graph(ei, n), ei, n)
    assert st['units_m'] > 0 and st['units_split'] > 0, (st, per_class)
