"""tests/tri_ref.py (the numpy restatement of the 'augmented' and 'haantjes' curvatures) against the reference's own recorded
values and against the C oracle, with ==: the reference behind tests/test_tri_incremental_gpu.py must not be wrong in the way
the code it checks is.  No GPU."""
import numpy as np
import pytest

import tri_ref
from conftest import load_golden


@pytest.mark.parametrize('fname', ['fullpass_small.json', 'fullpass_sampled.json'])
def test_recorded_values_of_the_reference(fname):
    graphs = load_golden(fname)['graphs']
    assert graphs
    for name, rec in graphs.items():
        ei, n = np.array(rec['edge_index']), rec['num_nodes']
        for kind in tri_ref.KINDS:
            eu, ev, cv = tri_ref.curv_all(ei, n, kind)
            assert cv.dtype == np.float64 and np.array_equal(cv, np.rint(cv))
            if not rec['sampled']:
                assert np.stack([eu, ev], 1).tolist() == rec['edges'], (name, 'edge order')
                assert cv.tolist() == [float(w) for w in rec[kind]], (name, kind)
            got = {(u, v): c for u, v, c in zip(eu.tolist(), ev.tolist(), cv.tolist())}
            assert len(rec['edges']) == len(rec[kind]) > 0
            for (u, v), w in zip(rec['edges'], rec[kind]):
                assert got[(u, v)] == float(w), (name, kind, u, v)


def test_both_counts_of_common_neighbours_agree():
    """The sorted-adjacency count against (A @ A) masked by A and against Python sets, on a graph with triangles, one with a
    hub and degree-1 leaves, and one with isolated nodes at both ends of the id range."""
    import scipy.sparse  # noqa: F401  (tests/spectral_ref.py and others need it too)
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(300, 6, seed=2)
    star = np.array([[k for k in range(2, 80)] + [3, 5], [1] * 78 + [2, 4]])      # hub 1, one triangle (1, 2, 3); 0, 80, 81 isolated
    for ei_, n_ in ((ei, n), (star, 82), (np.array([[2], [1]]), 4)):
        eu, ev = tri_ref.edges_of_input(ei_, n_)
        got = tri_ref.common_neighbours(eu, ev, n_)
        assert np.array_equal(got, tri_ref.common_neighbours_scipy(eu, ev, n_))
        nbr = [set() for _ in range(n_)]
        for u, v in zip(eu.tolist(), ev.tolist()):
            nbr[u].add(v)
            nbr[v].add(u)
        assert got.tolist() == [len(nbr[u] & nbr[v]) for u, v in zip(eu.tolist(), ev.tolist())]
    assert tri_ref.common_neighbours(*tri_ref.edges_of_input(ei, n), n).sum() > 0


@pytest.mark.parametrize('n,m,seed', [(500, 6, 31), (900, 3, 32)])
def test_c_oracle_on_random_graphs_and_behind_edits(n, m, seed):
    """oracle.c_oracle.CGraph.curv_all on two random graphs: as created (edges_of_input), and after random additions and
    removals from the export of its rows (edges_of_rows) — the form the GPU tests hand over."""
    from dcr import synthetic
    from oracle import c_oracle
    ei, nn = synthetic.powerlaw_graph(n, m, seed=seed)
    C = c_oracle.CGraph(ei, nn)
    rng = np.random.Generator(np.random.PCG64(seed))
    for edited in (False, True):
        if edited:
            for _ in range(60):
                u, v = (int(t) for t in rng.integers(0, nn, 2))
                if u != v:
                    C.remove_edge(u, v) if C.has_edge(u, v) else C.add_edge(u, v)
        for kind in tri_ref.KINDS:
            ou, ov, oc = C.curv_all(kind, nthreads=2)
            eu, ev, cv = tri_ref.curv_all(C.to_edge_index(), nn, kind, rows=True)
            assert np.array_equal(eu, ou) and np.array_equal(ev, ov), (kind, edited)
            assert np.array_equal(cv.view(np.int64), oc.view(np.int64)), (kind, edited)
            if not edited:
                iu, iv, ic = tri_ref.curv_all(ei, nn, kind)
                assert np.array_equal(iu, ou) and np.array_equal(iv, ov) and np.array_equal(ic, oc), kind
        assert (C.curv_all('haantjes')[2] > 0).sum() > 10      # there are triangles to count
