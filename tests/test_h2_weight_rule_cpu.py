"""The update rule by which the edit kernels keep the two-hop pass's node weights W(u) = sum of deg(k) over k in N(u) current
(csrc/dcr_graph.hip: dev_weight_edit), restated in numpy and checked against a recomputation from scratch over random edit
sequences.  Plain integer arithmetic, no GPU: an add of {u,v} with old degrees du, dv gives W[u] += dv + 1, W[v] += du + 1 and
W[w] += 1 for every other member w of the old N(u) and of the old N(v) (a common neighbour gets both); a removal is the mirror
image; an add of an existing edge and a removal of an absent one change nothing."""
import numpy as np
import pytest


def weights_from_scratch(adj):
    deg = np.array([len(a) for a in adj], dtype=np.int64)
    return np.array([int(deg[list(a)].sum()) if a else 0 for a in adj], dtype=np.int64)


def apply_add(adj, W, u, v):
    """The rule as the kernels apply it: the edit first, then the rows as they stand behind it."""
    if u == v or v in adj[u]:
        return False
    adj[u].add(v)
    adj[v].add(u)
    for w in adj[u]:
        if w != v:
            W[w] += 1
    for w in adj[v]:
        if w != u:
            W[w] += 1
    W[u] += len(adj[v])      # dv + 1: v's degree with the edge in place
    W[v] += len(adj[u])
    return True


def apply_remove(adj, W, u, v):
    if u == v or v not in adj[u]:
        return False
    adj[u].discard(v)
    adj[v].discard(u)
    for w in adj[u]:
        W[w] -= 1
    for w in adj[v]:
        W[w] -= 1
    W[u] -= len(adj[v]) + 1  # v's degree while the edge was there
    W[v] -= len(adj[u]) + 1
    return True


def random_graph(rng, n, m):
    adj = [set() for _ in range(n)]
    for _ in range(m):
        a, b = (int(t) for t in rng.integers(0, n, 2))
        if a != b:
            adj[a].add(b)
            adj[b].add(a)
    return adj


@pytest.mark.parametrize('n,m,seed', [(8, 10, 0), (40, 60, 1), (40, 400, 2), (200, 300, 3)])
def test_random_edit_sequences_keep_the_weights_exact(n, m, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    adj = random_graph(rng, n, m)
    W = weights_from_scratch(adj)
    done = {'add': 0, 'remove': 0, 'noop': 0}
    for step in range(600):
        a, b = (int(t) for t in rng.integers(0, n, 2))
        if rng.random() < 0.5:
            changed = apply_add(adj, W, a, b)
            done['add' if changed else 'noop'] += 1
        else:
            if rng.random() < 0.7 and adj[a]:          # mostly edges that exist
                b = int(rng.choice(sorted(adj[a])))
            changed = apply_remove(adj, W, a, b)
            done['remove' if changed else 'noop'] += 1
        assert np.array_equal(W, weights_from_scratch(adj)), (step, a, b)
    assert min(done.values()) > 20, done


def test_common_neighbour_gets_both_increments_and_leaves_reach_zero():
    # 0 and 1 share the neighbours 2 and 3; 4 hangs on 0, 5 on 1
    adj = [set() for _ in range(7)]
    for a, b in ((0, 2), (0, 3), (1, 2), (1, 3), (0, 4), (1, 5)):
        adj[a].add(b)
        adj[b].add(a)
    W = weights_from_scratch(adj)
    before = W.copy()
    assert apply_add(adj, W, 0, 1)
    assert (W - before).tolist() == [4, 4, 2, 2, 1, 1, 0]    # endpoints: the other's new degree; 2 and 3: +2; 4 and 5: +1
    assert apply_remove(adj, W, 0, 1)
    assert np.array_equal(W, before)
    assert not apply_add(adj, W, 0, 2) and not apply_remove(adj, W, 4, 5) and np.array_equal(W, before)
    assert apply_remove(adj, W, 0, 4)                        # 4 is left with degree 0: its weight is 0, 0 lost a leaf
    assert W[4] == 0 and np.array_equal(W, weights_from_scratch(adj))
    assert apply_add(adj, W, 6, 4)                           # an add between two isolated nodes
    assert W[4] == 1 and W[6] == 1 and np.array_equal(W, weights_from_scratch(adj))


def test_the_retry_mark_survives_the_arithmetic():
    """Bit 31 of a kept weight is the retry mark of the last pass; the updates are 32-bit wrapping adds of small numbers on a
    value whose low 31 bits stay in [0, 2^31): no carry or borrow reaches the mark."""
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(2000):
        w = int(rng.integers(0, 1 << 20))
        d = int(rng.integers(-w, 1 << 12))
        marked = np.array([w | 0x80000000], dtype=np.uint32)
        marked += np.uint32(d & 0xFFFFFFFF)
        assert int(marked[0]) & 0x7FFFFFFF == w + d and int(marked[0]) >> 31 == 1
