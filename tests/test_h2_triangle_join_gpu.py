"""The block classes of the two-hop pass count the triangle term of their candidates themselves (csrc/dcr_bfc_h2.hip:
h2_join_prepare, h2_batch_join): for the occurrence of w in row r of node u,

    c(w) = M_u(w) - 1 - |{ j in rows(w), j != r : v_j adjacent to v_r }|

from the unit's own list of exact-path items, instead of listing (candidate, partner) pairs for k_h2_triangles.  Units whose
item list overflowed keep the probe path and are counted.  Every graph is built here with numpy so that the large node reaches
the class it is meant for (checked on the CPU against a restatement of h2_classify); every edge's curvature is compared bit for
bit with the C oracle (curvature/bfc_naive.py:7-40)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the limits of h2_classify / h2_parts_for (csrc/dcr_bfc_h2.hip)
SMALL_DEG, MAXW2, MAXW3, KEYCAP3, KEYCAP4, L1_SPLIT = 64, 4096, 8192, 2800, 5500, 17
FAST_ROWS = 256          # h2_node_fast: at most 64 rows per wave, 4 waves
SPLIT_BATCH = 64 * 16    # rows of a split unit per batch of 64 rows per wave
H2_ITEMS = 2048
JOIN_MAXM = 256          # rows one key may occur in for a unit to join its triangle term itself


def classify(d, S):
    """(class, partitions) of a node with d neighbours whose degrees sum to S."""
    if d <= SMALL_DEG and S <= MAXW2:
        return (0 if S <= 1024 else 1 if S <= 2048 else 2), 1
    if S <= MAXW3 and d + S // 4 <= KEYCAP3:
        return 3, 1
    room = KEYCAP4 - d
    if room <= 0:
        return 4, 65536
    keys = S // 3 + 64
    per = (1 << L1_SPLIT) // 8
    return 4, max(1, -(-keys // room), -(-S // per))


def part_of(key, nparts):
    return ((((key * 0xC2B2AE35) & 0xFFFFFFFF) >> 16) * nparts) >> 16


def degrees(ei, n):
    deg = np.bincount(ei[0], minlength=n)
    S = np.bincount(ei[0], weights=deg[ei[1]], minlength=n).astype(np.int64)
    return deg, S


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

    def large_node(self, D, pool, extra):
        """A node with exactly D neighbours: a clique of 6 among them, planted triangles, common second neighbours shared by 2, 3
        and up to 70 rows (adjacent rows: the correction takes the count to exactly 0; non-adjacent: it stays), neighbours of
        degree 1 (nb[42:50]), an isolated triangle {x, nb[40], nb[41]} (leaf_rows_present checks both on the finished graph),
        and `extra` random second neighbours per remaining row out of `pool`."""
        x = int(self.nodes(1)[0])
        nb = self.nodes(D)
        self.star(x, nb)
        for a in range(6):
            for b in range(a + 1, 6):
                self.edge(nb[a], nb[b])
        for a, b in ((6, 7), (8, 9), (10, 11), (11, 12)):
            self.edge(nb[a], nb[b])
        s = self.nodes(8)
        self.star(s[0], nb[[6, 7]])            # two adjacent rows: 2 - 1 - 1 = 0
        self.star(s[1], nb[[20, 21]])          # two rows, not adjacent: stays 1
        self.star(s[2], nb[[0, 1, 30]])        # three rows, two of them adjacent
        self.star(s[3], nb[[10, 11, 12]])      # a path: the middle row loses both
        wide = np.r_[0:40, 50:min(80, D)]      # (not the rows that stay leaves and the isolated triangle)
        self.star(s[4], nb[wide])              # 64+ rows where the node has them, the clique among them
        self.star(s[5], nb[[8, 9]])
        self.star(s[6], nb[[8, 9]])            # two candidates of one edge, both driven to 0
        self.star(s[7], nb[[0, 6, 8, 20]])
        self.edge(nb[40], nb[41])              # an isolated triangle {x, nb40, nb41}; nb[42:50]: degree 1
        for i in range(50, D):
            self.star(nb[i], self.rng.choice(pool, size=int(self.rng.integers(extra[0], extra[1])), replace=False))
        for _ in range(D // 8):                # more triangles at x, anywhere among the filled rows
            a, b = self.rng.integers(50, D, size=2)
            self.edge(nb[a], nb[b])
        return x, nb

    def edge_index(self):
        from dcr import synthetic
        return synthetic.coalesced_edge_index(np.array(self.src), np.array(self.dst), self.n), self.n


@pytest.fixture()
def h2graph(monkeypatch):
    monkeypatch.setenv('DCR_PASS', 'h2')
    from dcr.graph import DcrGraph
    return DcrGraph


def check(G, ei, n):
    """Every edge against the oracle, bit for bit; returns the pass's diagnostics."""
    from oracle import c_oracle
    eu, ev, cv = G.curvature_all('bfc')
    assert G.pass_engine() == 'two-hop'
    oc = c_oracle.CGraph(ei, n).curv_edges(eu, ev, 'bfc', nthreads=8)
    assert len(eu) == ei.shape[1] // 2
    bad = np.flatnonzero(cv.view(np.int64) != oc.view(np.int64))
    assert bad.size == 0, (bad.size, eu[bad[:5]], ev[bad[:5]], cv[bad[:5]], oc[bad[:5]])
    return G.h2_stats()


def edited(ei, n, add, remove):
    from dcr import synthetic
    key = ei[0] * n + ei[1]
    drop = {a * n + b for a, b in remove} | {b * n + a for a, b in remove}
    keep = np.array([k not in drop for k in key.tolist()])
    src = np.concatenate([ei[0][keep], [a for a, _ in add]])
    dst = np.concatenate([ei[1][keep], [b for _, b in add]])
    return synthetic.coalesced_edge_index(src, dst, n)


def close_and_open_a_triangle(G, ei, n, nb):
    """Join two neighbours of the large node that were not adjacent, separate two that were; pass again."""
    G.add_edge(int(nb[20]), int(nb[21]))
    G.remove_edge(int(nb[6]), int(nb[7]))
    ei2 = edited(ei, n, [(int(nb[20]), int(nb[21]))], [(int(nb[6]), int(nb[7]))])
    return check(G, ei2, n), ei2


def leaf_rows_present(ei, n, x, nb):
    """Rows of one entry (neighbours of degree 1) and an isolated triangle at the large node (bfc_naive.py:18-19)."""
    deg, _ = degrees(ei, n)
    assert np.all(deg[nb[42:50]] == 1), deg[nb[42:50]]
    assert deg[nb[40]] == 2 and deg[nb[41]] == 2
    pair = set(zip(ei[0].tolist(), ei[1].tolist()))
    assert {(int(nb[40]), int(nb[41])), (int(x), int(nb[40])), (int(x), int(nb[41]))} <= pair


def idle(st):
    assert st['fallback'] == 0 and st['ncand'] == (0, 0), st


def class_m_graph(degs, seed):
    b = Builder(seed)
    pool = b.nodes(300)
    big = [b.large_node(D, pool, (2, 9)) for D in degs]
    rest = b.nodes(1600)                      # a sparse background: the second neighbours have neighbours of their own
    for v in pool:
        b.star(v, b.rng.choice(rest, size=2, replace=False))
    for v in rest[::2]:
        b.edge(v, b.rng.choice(rest))
    ei, n = b.edge_index()
    deg, S = degrees(ei, n)
    for (x, _), D in zip(big, degs):
        assert deg[x] == D and classify(int(deg[x]), int(S[x])) == (3, 1), (D, deg[x], S[x])
    for x, nb in big:
        leaf_rows_present(ei, n, x, nb)
    return ei, n, big


def test_class_m_register_path_both_ends_of_its_range(h2graph):
    """Degree 65 and degree 256: the ends of h2_node_fast's range, one batch of rows per wave."""
    ei, n, big = class_m_graph([65, FAST_ROWS], seed=1)
    assert 2000 <= n <= 3000
    G = h2graph(ei, n)
    st = check(G, ei, n)
    idle(st)
    assert st['units_m'] >= 2
    st, ei = close_and_open_a_triangle(G, ei, n, big[1][1])
    idle(st)
    st, ei = close_and_open_a_triangle(G, ei, n, big[0][1])
    idle(st)


def test_class_m_beyond_the_register_path(h2graph):
    """Degree 280: class M, but more than 64 rows per wave — the streaming route, two batches."""
    ei, n, big = class_m_graph([280], seed=2)
    assert big and FAST_ROWS < 280 <= 300
    idle(check(h2graph(ei, n), ei, n))


def split_graph(seed):
    b = Builder(seed)
    pool = b.nodes(8000)
    D = 1200
    x, nb = b.large_node(D, pool, (24, 34))
    for _ in range(600):                      # many more triangles at the hub
        a, c = b.rng.integers(50, D, size=2)  # (nb[40:50] stay the isolated triangle and the leaves)
        b.edge(nb[a], nb[c])
    far = int(b.nodes(1)[0])                  # a second neighbour shared by rows of both batches of 64 rows per wave,
    b.star(far, nb[[5, 4, 1100, 1101]])       # two of them adjacent (clique) and two not
    ei, n = b.edge_index()
    return ei, n, x, nb, far


def test_split_hub_three_partitions_two_batches(h2graph):
    ei, n, x, nb, far = split_graph(seed=3)
    deg, S = degrees(ei, n)
    cls, nparts = classify(int(deg[x]), int(S[x]))
    assert cls == 4 and nparts >= 3 and deg[x] >= 300 and S[x] > MAXW3, (deg[x], S[x], nparts)
    leaf_rows_present(ei, n, x, nb)
    # a triangle {x, a, c} and a candidate w of edge {x, a}, adjacent to c, whose key lies in another partition than c's; and a
    # second neighbour shared by rows of different batches (row = position in x's ascending adjacency list)
    adj = {}
    for a, c in zip(ei[0].tolist(), ei[1].tolist()):
        adj.setdefault(a, set()).add(c)
    nx = adj[x]
    cross = False
    for a in sorted(nx):
        for c in adj[a] & nx:
            if any(part_of(w, nparts) != part_of(c, nparts) for w in (adj[a] & adj[c]) - nx - {x}):
                cross = True
                break
        if cross:
            break
    assert cross
    rows = {v: i for i, v in enumerate(sorted(nx))}
    assert {rows[v] // SPLIT_BATCH for v in adj[far] & nx} == {0, 1} and len(adj[far] & adj[int(nb[5])] & nx) > 0
    G = h2graph(ei, n)
    st = check(G, ei, n)
    idle(st)
    assert st['units_split'] >= 3
    idle(close_and_open_a_triangle(G, ei, n, nb)[0])


def test_overflowed_item_list_takes_the_probe_path(h2graph):
    """A hub whose neighbours are densely joined among themselves: every wave meets thousands of members of N(u) in its rows,
    more exact-path items than its list holds — the unit streams its third sweep and lists for k_h2_triangles."""
    b = Builder(4)
    pool = b.nodes(500)
    D = 400
    x = int(b.nodes(1)[0])
    nb = b.nodes(D)
    b.star(x, nb)
    up = np.triu(b.rng.random((D, D)) < 0.5, 1)
    for a, c in zip(*np.nonzero(up)):
        b.edge(nb[a], nb[c])
    for v in nb:
        b.star(v, b.rng.choice(pool, size=3, replace=False))
    ei, n = b.edge_index()
    deg, S = degrees(ei, n)
    assert classify(int(deg[x]), int(S[x]))[0] == 4
    # members of N(x) met in the rows of one wave of the 16 (they are listed whatever their partition)
    assert (int(S[x]) - 4 * D) // 16 > 2 * H2_ITEMS
    st = check(h2graph(ei, n), ei, n)
    assert st['fallback'] > 0, st


def test_key_in_more_rows_than_the_join_takes(h2graph):
    """Two nodes with 300 common neighbours: each is a key in 300 rows of the other, M (M - 1) probes inside one unit — above
    JOIN_MAXM rows the unit keeps the probe path (T_r probes per candidate) and is counted."""
    b = Builder(5)
    x, y, z = (int(v) for v in b.nodes(3))
    nb = b.nodes(300)
    b.star(x, nb)
    b.star(y, nb)
    b.star(z, nb[:100])
    for i in range(20):
        b.edge(nb[2 * i], nb[2 * i + 1])        # triangles at x and at y: their candidates y, x and z lose a count each
    ei, n = b.edge_index()
    deg, S = degrees(ei, n)
    for v in (x, y):
        assert deg[v] == 300 > JOIN_MAXM and classify(int(deg[v]), int(S[v])) == (3, 1)
    st = check(h2graph(ei, n), ei, n)
    assert st['fallback'] >= 2, st
