"""Inputs for the improvement pipeline's tests (csrc/dcr_sdrf.hip: k_imp_insert, k_imp_rows_count, k_imp_bc, k_imp_emit) and a
host model of its bookkeeping, from the adjacency alone.  No GPU and no oracle in here: the builders say what they built, the
census says which of the pipeline's branches a set of edges reaches, and the tests assert both before they compare anything.

Names as in the kernels: for an edge (x, y), DX = N(x) - N(y) - {y}, DY = N(y) - N(x) - {x}; c1[i] = |N(i) & DY| for i in DX,
c2[j] = |N(j) & DX| for j in DY (the 4-cycles x - i - j - y); every counter set is summarised as (maximum, how many attain it,
largest value below it); gamma = max(max c1, max c2)."""
import numpy as np

KINDS = ('bfc', '1d', 'augmented', 'haantjes')

# the (dx, dy, big) of tests 1: each of dx + 1 and dy + 1 on both sides of 32, 256 and 512 in one orientation or the other, a
# bitmap whose last word is full (dy + 1 = 32, 256, 33 * 32 ...) and one that is not, a row beyond one 4 * 256 stride
SHAPES = [(1, 1, 0), (1, 40, 0), (31, 255, 0), (30, 31, 0), (32, 32, 0), (255, 33, 0), (256, 32, 1030), (257, 256, 2049),
          (513, 512, 0), (40, 1100, 1500)]
LARGE_SHAPES = [(513, 512, 0), (40, 1100, 1500)]   # bfc and augmented only
STRIDE = 4 * 256                                      # entries of a neighbour's row per round of k_imp_rows_count / k_imp_bc


def shape_args(dx, dy, big, seed=0):
    """The arguments of ``shaped`` the tests use for a (dx, dy, big)."""
    return dict(dx=dx, dy=dy, big=big, n_tri=5 if min(dx, dy) > 5 else 0, n_sq=3 * max(dx, dy), seed=seed)


def undirected_edge_index(pairs):
    """int64 [2, 2E] from a list of undirected pairs, in THAT order: rows keep insertion order (first the pairs with
    dst <= src, which is what the graph is built from; the mirrored half makes the input symmetric)."""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    hi, lo = np.maximum(p[:, 0], p[:, 1]), np.minimum(p[:, 0], p[:, 1])
    return np.stack([np.concatenate([hi, lo]), np.concatenate([lo, hi])])


def shaped(dx, dy, big, n_tri, n_sq, seed):
    """An edge (x, y) with deg(x) = dx, deg(y) = dy, ``n_tri`` common neighbours, ``n_sq`` edges between the private
    neighbourhoods (4-cycles and inadmissible pairs) and, with ``big`` > 0, one private neighbour of x with ``big`` further
    neighbours of its own.  Node ids are a seeded permutation and the edges come in a seeded order, so no row is in id order;
    the big node's last min(4, .) private-neighbourhood edges (they count towards ``n_sq``) are appended at the very end, so
    they sit behind position ``big`` of its row.  Returns (edge_index, num_nodes, info); info: x, y, big_node (or -1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    px, py = dx - 1 - n_tri, dy - 1 - n_tri
    if px < 0 or py < 0 or (big > 0 and px < 1):
        raise ValueError('degrees too small for the triangles / the big neighbour')
    n = 2 + n_tri + px + py + big
    X, Y = 0, 1
    tri = list(range(2, 2 + n_tri))
    ax = list(range(2 + n_tri, 2 + n_tri + px))
    ay = list(range(2 + n_tri + px, 2 + n_tri + px + py))
    far = list(range(2 + n_tri + px + py, n))
    pairs = [(X, Y)] + [(X, t) for t in tri] + [(Y, t) for t in tri] + [(X, a) for a in ax] + [(Y, b) for b in ay]
    n_sq = min(n_sq, px * py)
    tail = []
    bign = ax[0] if big > 0 else -1
    if big > 0:
        pairs += [(bign, f) for f in far]
        tail = [(bign, int(b)) for b in rng.choice(ay, size=min(4, py, n_sq), replace=False)]
    if n_sq:
        taken = {0 * py + (b - ay[0]) for _, b in tail}
        free = np.setdiff1d(np.arange(px * py), np.fromiter(taken, dtype=np.int64, count=len(taken)))
        for c in rng.choice(free, size=n_sq - len(tail), replace=False).tolist():
            pairs.append((ax[c // py], ay[c % py]))
    order = rng.permutation(len(pairs))
    pairs = [pairs[k] for k in order] + tail
    perm = rng.permutation(n)
    pairs = [(int(perm[u]), int(perm[v])) for u, v in pairs]
    info = dict(x=int(perm[X]), y=int(perm[Y]), big_node=int(perm[bign]) if big > 0 else -1)
    return undirected_edge_index(pairs), n, info


def rows_of(ei, n):
    """Adjacency rows in insertion order (pairs with dst <= src, duplicates ignored), as the graph container keeps them."""
    rows = [[] for _ in range(n)]
    seen = set()
    for u, v in zip(ei[0].tolist(), ei[1].tolist()):
        if v > u or (u, v) in seen:
            continue
        seen.add((u, v))
        rows[u].append(v)
        rows[v].append(u)
    return rows


def check_shaped(ei, n, info, dx, dy, big, n_tri):
    """What the host can say about a shaped graph: the degrees, the triangles, the long row and — beyond the first stride of
    that row — neighbours of y, so that the second round of the row's sweep has something to find.  Returns the rows."""
    rows = rows_of(ei, n)
    x, y = info['x'], info['y']
    assert len(set(zip(ei[0].tolist(), ei[1].tolist()))) == ei.shape[1], 'duplicate pairs'
    assert len(rows[x]) == dx and len(rows[y]) == dy, (len(rows[x]), len(rows[y]))
    assert y in rows[x] and x in rows[y]
    assert len(set(rows[x]) & set(rows[y])) == n_tri
    assert rows[x] != sorted(rows[x]) or dx < 3, 'row x is in id order'
    if big > 0:
        b = info['big_node']
        assert b in rows[x] and b not in rows[y]
        assert len(rows[b]) > big and len(rows[b]) > STRIDE, len(rows[b])
        late = [w for w in rows[b][STRIDE:] if w in set(rows[y])]
        assert late, 'no neighbour of y behind the first stride of the long row'
    return rows


def disjoint_union(ei_a, n_a, ei_b, n_b):
    return np.concatenate([ei_a, ei_b + n_a], axis=1), n_a + n_b


def star_with_leaf_edge(leaves):
    """Centre 0, leaves 1 .. leaves, and the leaf-leaf edge (1, 2)."""
    pairs = [(0, k) for k in range(1, leaves + 1)] + [(1, 2)]
    return undirected_edge_index(pairs), leaves + 1


def ranked_edges(eu, ev, deg, heavy=6, median=3, light=3):
    """(x, y) of the heaviest, median and lightest edges by deg * deg (stable order among equals)."""
    w = deg[eu].astype(np.int64) * deg[ev].astype(np.int64)
    order = np.argsort(-w, kind='stable')
    mid = len(order) // 2
    pick = order[:heavy].tolist() + order[mid:mid + median].tolist() + order[len(order) - light:].tolist()
    return [(int(eu[e]), int(ev[e])) for e in dict.fromkeys(pick)]


# ---- the many small graphs of test 2 -------------------------------------------------------------------------------------
CENSUS_SEED = 7
CENSUS_GRAPHS = 120
CENSUS_CAP = 20
BRANCHES = ('sec_B', 'sec_C', 'dec_B', 'dec_C', 'gamma_raised', 'deg1_edges', 'empty_edges')


def small_graphs(count=CENSUS_GRAPHS, seed=CENSUS_SEED):
    """Seeded Erdős–Rényi graphs, n in [4, 14], p in [0.15, 0.7]; graphs without an edge are skipped (and not counted).
    Yields (edge_index, n, oriented edges): every edge once, (u, v) and (v, u) alternating along G.edges order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    made = 0
    while made < count:
        n = int(rng.integers(4, 15))
        p = float(rng.uniform(0.15, 0.7))
        iu, ju = np.triu_indices(n, k=1)
        keep = rng.random(iu.shape[0]) < p
        if not keep.any():
            continue
        ei = undirected_edge_index(np.stack([iu[keep], ju[keep]], 1))
        rows = rows_of(ei, n)
        edges = [(u, v) for u in range(n) for v in rows[u] if v > u]
        yield ei, n, [(u, v) if (made + k) % 2 == 0 else (v, u) for k, (u, v) in enumerate(edges)]
        made += 1


def _mx(values):
    """(maximum, multiplicity, runner-up) of a counter set; (0, 0, 0) when it is empty; runner-up 0 when there is none."""
    if not values:
        return 0, 0, 0
    m = max(values)
    below = [v for v in values if v < m]
    return m, sum(v == m for v in values), max(below) if below else 0


def edge_model(adj, x, y):
    """The pipeline's view of the edge (x, y) on adjacency sets ``adj``: counters, their summaries, and how many candidates
    reach each branch.  A branch counts only where it decides the value: both degrees at least 2 after the add (else the
    curvature is 0 whatever the counters say), both 4-cycle sets non-empty after it (else gamma is not read), and gamma not
    what the branch's alternative would have given."""
    nx, ny = adj[x], adj[y]
    DX = sorted(nx - ny - {y})
    DY = sorted(ny - nx - {x})
    sDX, sDY = set(DX), set(DY)
    c1 = {i: len(adj[i] & sDY) for i in DX}
    c2 = {j: len(adj[j] & sDX) for j in DY}
    max1, cnt1, sec1 = _mx(list(c1.values()))
    max2, cnt2, sec2 = _mx(list(c2.values()))
    s1 = sum(v > 0 for v in c1.values())
    s2 = sum(v > 0 for v in c2.values())
    gamma = max(max1, max2)
    dx, dy = len(nx), len(ny)
    out = dict.fromkeys(BRANCHES, 0)
    out.update(reach_sec_B=0, reach_sec_C=0, reach_dec_B=0, reach_dec_C=0, reach_gamma_raised=0)

    def side(tag, nodes, c_own, mx_own, c_other, mx_other, s_own, s_other, d_other_min):
        # class B (tag 'B'): i == x, j in DY leaves DY (own = c2), and every c1[k] with k ~ j loses one (other = c1)
        (m_own, n_own, r_own), (m_oth, n_oth, _) = mx_own, mx_other
        for j in nodes:
            sec = m_own > 0 and c_own[j] == m_own and n_own == 1
            hit = [k for k, v in c_other.items() if k in adj[j]]
            dec = m_oth > 0 and sum(c_other[k] == m_oth for k in hit) == n_oth
            new_own = r_own if sec else m_own
            new_oth = m_oth - 1 if dec else m_oth
            s_own_after = s_own - (c_own[j] > 0)
            s_oth_after = s_other - sum(c_other[k] == 1 for k in hit)
            # the literal recount agrees with the summaries (this is the model, checked here on every candidate)
            assert new_own == max([v for k, v in c_own.items() if k != j], default=0)
            assert new_oth == max([v - (k in adj[j]) for k, v in c_other.items()], default=0)
            live = d_other_min >= 2 and s_own_after > 0 and s_oth_after > 0
            g_true = max(new_own, new_oth)
            out['reach_sec_' + tag] += sec
            out['reach_dec_' + tag] += dec
            out['sec_' + tag] += bool(sec and live and max(m_own, new_oth) != g_true)
            out['dec_' + tag] += bool(dec and live and max(new_own, m_oth) != g_true)

    side('B', DY, c2, (max2, cnt2, sec2), c1, (max1, cnt1, sec1), s2, s1, dy)
    side('C', DX, c1, (max1, cnt1, sec1), c2, (max2, cnt2, sec2), s1, s2, dx)
    for i in DX:
        for j in DY:
            if j not in adj[i] and max(c1[i], c2[j]) + 1 > gamma:
                out['reach_gamma_raised'] += 1
                out['gamma_raised'] += min(dx, dy) >= 2
    cand = sum(1 for i in list(nx) + [x] for j in list(ny) + [y] if i != j and j not in adj[i])
    out['deg1_edges'] = int(min(dx, dy) == 1)
    out['empty_edges'] = int(cand == 0)
    out.update(dx=dx, dy=dy, T=len(nx & ny), s1=s1, s2=s2, gamma=gamma, mx1=(max1, cnt1, sec1), mx2=(max2, cnt2, sec2),
               candidates=cand)
    return out


def branch_census(ei, n, edges=None):
    """Sum of ``edge_model`` over ``edges`` (default: every edge, (u, v) with u < v) of the graph: how many candidates reach
    the ``sec`` and ``max - 1`` branches of classes B and C and the gamma-raised branch of the general class where they
    decide the value (``reach_*``: where they are taken at all), and how many edges have a degree-1 endpoint / no
    candidate.  Also ``per_edge``: the models themselves."""
    rows = rows_of(ei, n)
    adj = [set(r) for r in rows]
    if edges is None:
        edges = [(u, v) for u in range(n) for v in rows[u] if v > u]
    per_edge = [edge_model(adj, x, y) for x, y in edges]
    total = {k: sum(m[k] for m in per_edge) for k in BRANCHES + tuple('reach_' + b for b in BRANCHES[:5])}
    total['edges'] = len(per_edge)
    total['per_edge'] = per_edge
    return total


def census_of(graphs):
    """Totals over an iterable of (edge_index, n, oriented edges)."""
    tot = {}
    n_graphs = 0
    for ei, n, edges in graphs:
        c = branch_census(ei, n, edges)
        for k, v in c.items():
            if k != 'per_edge':
                tot[k] = tot.get(k, 0) + v
        n_graphs += 1
    tot['graphs'] = n_graphs
    return tot
