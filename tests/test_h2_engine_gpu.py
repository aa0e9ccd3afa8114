"""The two-hop curvature-pass engine (csrc/dcr_bfc_h2.hip; the default for full Balanced Forman passes of graphs whose 2-hop
neighbourhoods are a small part of the graph, forced here with DCR_PASS=h2 when the graph is created): row u of A.A from
Bloom bitmaps and an exact table of the repeated keys instead of per-edge neighbourhood streaming.  Same bits as the
node-centric engine, the CPU oracle and the reference's fixtures (curvature/bfc_naive.py:7-40)."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture()
def h2graph(monkeypatch):
    monkeypatch.setenv('DCR_PASS', 'h2')
    from dcr.graph import DcrGraph

    def make(ei, n):
        G = DcrGraph(ei, n)
        return G
    return make


def _check_against_oracle(G, ei, n, nthreads=8):
    from oracle import c_oracle
    eu, ev, cv = G.curvature_all('bfc')
    assert G.pass_engine() == 'two-hop'
    C = c_oracle.CGraph(ei, n)
    ou, ov, oc = C.curv_all('bfc', nthreads=nthreads)
    assert np.array_equal(eu, ou) and np.array_equal(ev, ov)
    bad = np.flatnonzero(cv != oc)
    assert bad.size == 0, (bad[:5], eu[bad[:5]], ev[bad[:5]], cv[bad[:5]], oc[bad[:5]])


def test_reference_fixtures(h2graph):
    for fname in ('fullpass_small.json', 'fullpass_sampled.json'):
        for name, rec in load_golden(fname)['graphs'].items():
            G = h2graph(np.array(rec['edge_index']), rec['num_nodes'])
            eu, ev, cv = G.curvature_all('bfc')
            assert G.pass_engine() == 'two-hop'
            got = {(u, v): c for u, v, c in zip(eu.tolist(), ev.tolist(), cv.tolist())}
            for (u, v), h in zip(rec['edges'], rec['bfc']):
                assert got[(u, v)] == float.fromhex(h), (name, u, v)


@pytest.mark.parametrize('n,m,seed', [(3000, 4, 1), (1500, 12, 2), (400, 40, 3), (20000, 10, 4)])
def test_power_law_graphs(h2graph, n, m, seed):
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(n, m, seed=seed)
    _check_against_oracle(h2graph(ei, n), ei, n)


@pytest.mark.parametrize('n,p,seed', [(300, 0.5, 0), (600, 0.15, 1), (1200, 0.05, 2)])
def test_dense_random_graphs_many_triangles(h2graph, n, p, seed):
    """Nearly every 2-hop key repeats and every edge has triangle partners: overflow table, queue and step C all busy."""
    from dcr import synthetic
    ei, n = synthetic.erdos_renyi_graph(n, p, seed=seed)
    _check_against_oracle(h2graph(ei, n), ei, n)


def test_hubs_split_into_key_partitions(h2graph):
    """Hubs whose 2-hop neighbourhoods exceed the largest table: their keys are split over several units."""
    rng = np.random.Generator(np.random.PCG64(9))
    n = 30000
    src, dst = [], []
    hubs = [0, 1, 2]
    for h in hubs:                       # three adjacent hubs with ~4,000 neighbours each, overlapping
        nb = rng.choice(np.arange(3, n), size=4000, replace=False)
        src += [h] * len(nb)
        dst += nb.tolist()
    src += [0, 0, 1]
    dst += [1, 2, 2]
    a = rng.integers(3, n, size=60000)   # background edges: the hubs' neighbours have neighbours of their own
    b = rng.integers(3, n, size=60000)
    src += a.tolist()
    dst += b.tolist()
    from dcr import synthetic
    ei = synthetic.coalesced_edge_index(np.array(src), np.array(dst), n)
    _check_against_oracle(h2graph(ei, n), ei, n, nthreads=16)


def test_engines_agree_on_the_bench_graph_and_after_edits(h2graph, monkeypatch):
    from dcr import synthetic
    from dcr.graph import DcrGraph
    ei, n = synthetic.powerlaw_graph(100000, 10, seed=12345)
    H = h2graph(ei, n)
    monkeypatch.setenv('DCR_PASS', 'nc')
    D = DcrGraph(ei, n)
    monkeypatch.delenv('DCR_PASS')
    rng = np.random.Generator(np.random.PCG64(3))
    for rnd in range(3):
        hu, hv, hc = H.curvature_all('bfc')
        du, dv, dc = D.curvature_all('bfc')
        assert H.pass_engine() == 'two-hop' and D.pass_engine() == 'node-centric'
        assert np.array_equal(hu, du) and np.array_equal(hv, dv) and np.array_equal(hc, dc), rnd
        for _ in range(20):              # edits at hubs and elsewhere, the same on both
            a, b = int(rng.integers(0, 200)), int(rng.integers(0, n))
            if a != b and not D.has_edge(a, b):
                H.add_edge(a, b)
                D.add_edge(a, b)
        eu, ev = D.edges()
        for j in rng.integers(0, len(eu), size=20):
            a, b = int(eu[j]), int(ev[j])
            if D.has_edge(a, b):
                H.remove_edge(a, b)
                D.remove_edge(a, b)


def test_edge_set_is_patched_not_rebuilt_between_passes(h2graph, monkeypatch):
    """Round 4: the edge set of the triangle step is kept across passes and brought up to date from the journal of device-side
    edits (insertions, tombstones, re-insertions over tombstones; more than eight edits between two passes: rebuilt).  A
    handful of edits per round among hubs and their neighbours — where the triangle step probes — then a pass, against the
    node-centric engine on a twin graph, for 40 rounds; one round has too many edits for the journal."""
    from dcr import synthetic
    from dcr.graph import DcrGraph
    ei, n = synthetic.powerlaw_graph(30000, 8, seed=77)
    H = h2graph(ei, n)
    monkeypatch.setenv('DCR_PASS', 'nc')
    D = DcrGraph(ei, n)
    monkeypatch.delenv('DCR_PASS')
    rng = np.random.Generator(np.random.PCG64(5))
    removed, added = [], []
    for rnd in range(40):
        hu, hv, hc = H.curvature_all('bfc')
        du, dv, dc = D.curvature_all('bfc')
        assert H.pass_engine() == 'two-hop' and D.pass_engine() == 'node-centric'
        assert np.array_equal(hu, du) and np.array_equal(hv, dv)
        bad = np.flatnonzero(hc.view(np.int64) != dc.view(np.int64))
        assert bad.size == 0, (rnd, bad[:5], hu[bad[:5]], hv[bad[:5]])
        edits = 30 if rnd == 17 else int(rng.integers(1, 5))
        for _ in range(edits):
            kind = int(rng.integers(0, 4))
            if kind == 0 and removed:                      # put a removed edge back (a key over its own tombstone)
                a, b = removed.pop(int(rng.integers(0, len(removed))))
                if not D.has_edge(a, b):
                    H.add_edge(a, b), D.add_edge(a, b)
            elif kind == 1 and added:                      # take an added edge out again
                a, b = added.pop(int(rng.integers(0, len(added))))
                if D.has_edge(a, b):
                    H.remove_edge(a, b), D.remove_edge(a, b)
                    removed.append((a, b))
            elif kind == 2:                                # remove an edge at a hub
                hub = int(rng.integers(0, 40))
                nb = D.neighbors(hub)
                if len(nb) > 3:
                    b = int(nb[int(rng.integers(0, len(nb)))])
                    H.remove_edge(hub, b), D.remove_edge(hub, b)
                    removed.append((hub, b))
            else:                                          # join two neighbours of a hub (a new triangle at the hub) or two hubs
                hub = int(rng.integers(0, 40))
                nb = D.neighbors(hub)
                a, b = (int(nb[int(rng.integers(0, len(nb)))]), int(nb[int(rng.integers(0, len(nb)))])) if rng.random() < 0.7 \
                    else (int(rng.integers(0, 40)), int(rng.integers(0, 40)))
                if a != b and not D.has_edge(a, b):
                    H.add_edge(a, b), D.add_edge(a, b)
                    added.append((a, b))


def test_automatic_engine_choice(monkeypatch):
    """Without DCR_PASS the two-hop kernels take the full Balanced Forman passes of sparse graphs, the node-centric ones
    small dense graphs (where nearly every 2-hop key repeats), every incremental pass and the classical curvatures."""
    from dcr import synthetic
    from dcr.graph import DcrGraph
    monkeypatch.delenv('DCR_PASS', raising=False)
    ei, n = synthetic.powerlaw_graph(20000, 4, seed=5)
    G = DcrGraph(ei, n)
    G.curvature_pass('bfc')
    assert G.pass_engine() == 'two-hop'
    G.curvature_pass('augmented')
    assert G.pass_engine() == 'node-centric'
    ei, n = synthetic.powerlaw_graph(1500, 12, seed=2)
    G = DcrGraph(ei, n)
    G.curvature_pass('bfc')
    assert G.pass_engine() == 'node-centric'


def test_edge_by_edge_switch_is_read_per_pass(monkeypatch):
    """The automatic choice is three-way and its switches are read with every pass: 12 k edges go edge by edge (reported as
    node-centric: its estimate is below the two-hop one); with DCR_NC_FINE=0 set later in the same process a second graph of
    the same edges goes to the two-hop kernels.  (Read once per process, the second answer depended on which test had
    created the first graph.)  Same bits as the C oracle either way."""
    from dcr import synthetic
    from dcr.graph import DcrGraph
    from oracle import c_oracle
    monkeypatch.delenv('DCR_PASS', raising=False)
    monkeypatch.delenv('DCR_NC_FINE', raising=False)
    monkeypatch.delenv('DCR_NC_FINE_FULL', raising=False)
    ei, n = synthetic.powerlaw_graph(6000, 2, seed=4)
    ou, ov, oc = c_oracle.CGraph(ei, n).curv_all('bfc', nthreads=8)
    for fine, engine in ((None, 'node-centric'), ('0', 'two-hop')):
        if fine is not None:
            monkeypatch.setenv('DCR_NC_FINE', fine)
        G = DcrGraph(ei, n)
        eu, ev, cv = G.curvature_all('bfc')
        assert G.pass_engine() == engine
        assert np.array_equal(eu, ou) and np.array_equal(ev, ov)
        assert np.array_equal(cv.view(np.int64), oc.view(np.int64)), fine
        G.close()


def test_dense_neighbourhoods_are_redone_one_class_up(h2graph):
    """Small dense graph under the forced engine: the wave classes' tables fill up, the nodes go to the retry list and are
    redone by the largest class with worst-case partitions; the pools of the triangle step grow on demand."""
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(2500, 10, seed=11)
    _check_against_oracle(h2graph(ei, n), ei, n)


def test_pools_grown_to_their_limit_lose_no_corrections(h2graph):
    """Round 5 (found by tests/fuzz_parity.py, one pass in ~1,500): on this graph the two-hop pass outgrows its triangle-step pools,
    is run again with pools grown to what it had counted, then once more with its retry stage — and the candidate counter,
    which advances by whole chunks, ends within a few chunks of the grown pool's size, above it in one fresh pass in forty
    although every reservation fitted.  k_h2_triangles took that for a failed pass and returned; no status was raised, the pass
    was not run again, and a third of the edges lost their corrections.  120 fresh graphs (98 % to meet the case before the fix),
    every pass against the C oracle (bfc_naive.py:25-40)."""
    from dcr import synthetic
    from oracle import c_oracle
    ei, n = synthetic.powerlaw_graph(2997, 11, seed=210271642)
    oc = c_oracle.CGraph(ei, n).curv_all('bfc', nthreads=8)[2]
    for rep in range(120):
        G = h2graph(ei, n)
        cv = G.curvature_all('bfc')[2]
        assert G.pass_engine() == 'two-hop'
        bad = np.flatnonzero(cv != oc)
        assert bad.size == 0, (rep, bad.size, bad[:5])
        G.close()
