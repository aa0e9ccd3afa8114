"""What tests/test_improvements_gpu.py takes for granted about its inputs, checked without a GPU: the shaped graphs have the
degrees and the long row they were asked for, the small graphs reach every branch of the maximum bookkeeping often enough,
and the host model that says so agrees with the C oracle's ingredients."""
import numpy as np
import pytest

import improvements_ref as R


@pytest.fixture(scope='module')
def oracle():
    from oracle import c_oracle
    return c_oracle


@pytest.mark.parametrize('dx,dy,big', R.SHAPES)
def test_shaped_graphs_are_what_was_asked_for(oracle, dx, dy, big):
    a = R.shape_args(dx, dy, big)
    ei, n, info = R.shaped(**a)
    rows = R.check_shaped(ei, n, info, dx, dy, big, a['n_tri'])
    C = oracle.CGraph(ei, n)
    x, y = info['x'], info['y']
    assert (C.degree(x), C.degree(y)) == (dx, dy) and C.num_edges() == ei.shape[1] // 2
    q = C.ingredients(x, y)
    assert q[2] == a['n_tri']
    px, py = dx - 1 - a['n_tri'], dy - 1 - a['n_tri']
    if px * py >= 4:
        assert q[3] > 0 and q[4] > 0 and q[5] > 1    # 4-cycles on both sides, some counter above one
    # the candidate list walks the rows in their stored order
    oi, oj = C.candidates(x, y)
    first = next((i, j) for i in rows[x] + [x] for j in rows[y] + [y] if i != j and j not in rows[i]) if len(oi) else None
    assert first is None or (int(oi[0]), int(oj[0])) == (min(first), max(first))
    ei2, _, info2 = R.shaped(**a)
    assert np.array_equal(ei, ei2) and info == info2


def test_shapes_cross_every_stride_in_one_orientation_or_the_other():
    # both orientations are run, so either degree is dx (rows of the scan) and dy (positions placed, bits of a bitmap row)
    rows = {d + 1 for dx, dy, _ in R.SHAPES for d in (dx, dy)}
    assert {32, 33, 256, 257} <= rows, sorted(rows)                 # a last bitmap word / a last round exactly full, and one more
    assert {1, 2, 3, 5} <= {-(-r // 256) for r in rows}, sorted(rows)  # one, two, three and more rounds of 256 with a carry
    assert any(r % 32 == 0 and r > 32 for r in rows) and any(r % 32 for r in rows)
    assert any(big > R.STRIDE for _, _, big in R.SHAPES) and any(big > 2 * R.STRIDE for _, _, big in R.SHAPES)
    assert all(s in R.SHAPES for s in R.LARGE_SHAPES)


def test_small_graphs_reach_every_branch():
    census = R.census_of(R.small_graphs())
    print({k: v for k, v in census.items()})
    assert census['graphs'] == R.CENSUS_GRAPHS
    for b in R.BRANCHES:
        assert census[b] >= R.CENSUS_CAP, (b, census[b])
    for b in R.BRANCHES[:5]:
        assert census['reach_' + b] >= census[b]


def test_host_model_agrees_with_the_oracle_ingredients(oracle):
    checked = 0
    for g, (ei, n, edges) in enumerate(R.small_graphs(12)):
        C = oracle.CGraph(ei, n)
        models = R.branch_census(ei, n, edges)['per_edge']
        for (x, y), m in zip(edges, models):
            q = C.ingredients(x, y).tolist()
            assert q == [m['dx'], m['dy'], m['T'], m['s1'], m['s2'], max(m['mx1'][0], m['mx2'][0])], (g, x, y)
            assert m['candidates'] == len(C.candidates(x, y)[0])
            checked += 1
    assert checked > 100


def test_host_model_branches_are_the_oracle_values(oracle):
    """Around edges whose class-B candidates take the ``sec`` or the ``max - 1`` branch: the model recomputed on the graph with
    the candidate literally added gives the oracle's 4-cycle ingredients there (``edge_model`` itself asserts, candidate by
    candidate, that each branch's outcome is that recount)."""
    seen = dict(sec=0, dec=0)
    for ei, n, edges in R.small_graphs(30):
        C = oracle.CGraph(ei, n)
        adj = [set(r) for r in R.rows_of(ei, n)]
        for x, y in edges:
            m = R.edge_model(adj, x, y)
            if not (m['sec_B'] or m['dec_B']):
                continue
            for j in sorted(adj[y] - adj[x] - {x}):
                assert C.add_edge(x, j) == 0
                adj[x].add(j), adj[j].add(x)
                after = R.edge_model(adj, x, y)
                assert C.ingredients(x, y).tolist()[3:] == [after['s1'], after['s2'], after['gamma']]
                seen['sec'] += m['sec_B'] > 0
                seen['dec'] += m['dec_B'] > 0
                assert C.remove_edge(x, j) == 0
                adj[x].discard(j), adj[j].discard(x)
    assert seen['sec'] > 20 and seen['dec'] > 20, seen
