"""Monte-Carlo Cheeger estimate on the GPU against tests/cheeger_ref.py (itself pinned to the reference's recorded outputs by
tests/test_cheeger_cpu.py) and against tests/golden/cheeger_reference.json.  Every comparison is exact: == on int64 counts,
float.hex on ratios."""
import random

import numpy as np
import pytest

import cheeger_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

SHAPES = ['sliced', 'lane']


def fh(s):
    return float.fromhex(s)


def hexes(vals):
    return [float(v).hex() for v in vals]


def case_edge_index(case):
    from dcr import synthetic
    if case['generator'] is not None:
        return synthetic.powerlaw_graph(*case['generator']['powerlaw_graph'])[0]
    return np.asarray(case['edge_index'], dtype=np.int64).reshape(2, -1)


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


@pytest.fixture(scope='module')
def s100k():
    from dcr import synthetic
    return synthetic.powerlaw_graph(100000, 10, seed=12345)


def random_members(B, n, seed):
    """bool [B, n] with the all-members and the no-members subsets in front and a range of densities behind them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = rng.random((B, n)) < rng.random((B, 1))
    m[0] = True
    if B > 1:
        m[1] = False
    return m


def check_counts(G, ei, members):
    got = G.cheeger_counts(members)
    want = cheeger_ref.counts(ei, members)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:10]


@pytest.mark.parametrize('shape', SHAPES)
def test_hand_graphs_and_explicit_subsets_of_the_fixture(dcr, monkeypatch, shape):
    from experiment.compute_cheeger import values_from_counts
    monkeypatch.setenv('DCR_CHEEGER', shape)
    fx = load_golden('cheeger_reference.json')
    by_name = {c['name']: c for c in fx['estimate']}
    for rec in fx['cheeger_S']:
        case = by_name[rec['name']]
        ei, n = case_edge_index(case), case['num_nodes']
        members = np.zeros((len(rec['subsets']), n), dtype=np.bool_)
        for j, S in enumerate(rec['subsets']):
            members[j, S] = True
        G = dcr(ei, n)
        check_counts(G, ei, members)
        assert hexes(values_from_counts(G.cheeger_counts(members))) == [fh(h).hex() for h in rec['values']], rec['name']


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('n,m,gseed,B', [(400, 4, 3, 64), (400, 4, 3, 100), (400, 4, 3, 192), (400, 4, 3, 1), (20000, 2, 4, 1024),
                                         (20000, 2, 4, 130), (2485, 2, 0, 512 - 7)])
def test_counts_on_powerlaw_graphs(dcr, monkeypatch, shape, n, m, gseed, B):
    """W = 1, 2, 3, 16, 8 and subset counts that are not multiples of 64."""
    from dcr import synthetic
    monkeypatch.setenv('DCR_CHEEGER', shape)
    ei, n = synthetic.powerlaw_graph(n, m, seed=gseed)
    check_counts(dcr(ei, n), ei, random_members(B, n, seed=B))


@pytest.mark.parametrize('shape', SHAPES)
def test_counts_at_s100k(dcr, s100k, monkeypatch, shape):
    monkeypatch.setenv('DCR_CHEEGER', shape)
    ei, n = s100k
    check_counts(dcr(ei, n), ei, random_members(70, n, seed=11))


def test_packed_words_are_accepted_as_they_are(dcr):
    from dcr import synthetic
    from dcr.graph import pack_members
    ei, n = synthetic.powerlaw_graph(400, 4, seed=3)
    members = random_members(128, n, seed=5)
    words, _ = pack_members(members, n)
    G = dcr(ei, n)
    assert np.array_equal(G.cheeger_counts(words), cheeger_ref.counts(ei, members))


@pytest.mark.parametrize('shape', SHAPES)
def test_planted_hub_and_isolated_nodes(dcr, monkeypatch, shape):
    """One node of degree 6,000 (beyond the LDS tables of the curvature engines), and 300 nodes without any edge."""
    from dcr import synthetic
    monkeypatch.setenv('DCR_CHEEGER', shape)
    ei, n0 = synthetic.powerlaw_graph(8000, 3, seed=9)
    hub = 4321
    others = np.setdiff1d(np.arange(n0), [hub])[:6000]
    ei = synthetic.coalesced_edge_index(np.concatenate([ei[0], np.full(6000, hub)]), np.concatenate([ei[1], others]), n0 + 300)
    n = n0 + 300
    G = dcr(ei, n)
    assert G.degree(hub) >= 6000 and G.degree(n - 1) == 0
    check_counts(G, ei, random_members(200, n, seed=2))


@pytest.mark.parametrize('batch', [7, 64, 'iterations', 5000])
def test_estimate_cheeger_equals_the_reference(batch):
    import torch
    from dcr.data import Data
    from experiment.compute_cheeger import estimate_cheeger
    for case in load_golden('cheeger_reference.json')['estimate']:
        if batch == 7 and case['num_nodes'] > 1000:
            continue   # (the same code path as on the other graphs, 29 launches of it)
        data = Data(edge_index=torch.from_numpy(case_edge_index(case)), num_nodes=case['num_nodes'])
        random.seed(case['seed'])
        b = case['iterations'] if batch == 'iterations' else batch
        result, all_results = estimate_cheeger(data, case['iterations'], batch=b)
        assert isinstance(all_results, list) and all(type(v) is float for v in all_results)
        assert hexes(all_results) == [fh(h).hex() for h in case['all_results']], case['name']
        assert float(result).hex() == fh(case['result']).hex(), case['name']
        assert random.random().hex() == case['next_random'], case['name']


def test_estimate_cheeger_takes_a_live_graph_and_zero_iterations(dcr):
    from dcr import synthetic
    from experiment.compute_cheeger import estimate_cheeger
    ei, n = synthetic.powerlaw_graph(400, 4, seed=3)
    G = dcr(ei, n)
    state = random.getstate()
    assert estimate_cheeger(G, 0) == (float('inf'), [])
    assert random.getstate() == state
    random.seed(3)
    want = cheeger_ref.estimate(ei, n, 30)
    random.seed(3)
    got = estimate_cheeger(G, 30, batch=16)
    assert got[0].hex() == want[0].hex() and hexes(got[1]) == hexes(want[1])


def test_conductance_is_networkx_conductance(dcr):
    import networkx as nx
    from dcr import synthetic
    from experiment.compute_cheeger import estimate_cheeger, values_from_counts
    ei, n = synthetic.powerlaw_graph(400, 4, seed=3)
    G, H = dcr(ei, n), cheeger_ref.to_graph(ei, n)
    members = random_members(160, n, seed=8)[2:]
    got = values_from_counts(G.cheeger_counts(members), 'conductance')
    checked = 0
    for j in range(members.shape[0]):
        S = np.flatnonzero(members[j]).tolist()
        if 0 < len(S) < n and nx.volume(H, S) > 0 and nx.volume(H, set(range(n)) - set(S)) > 0:
            assert got[j].hex() == float(nx.conductance(H, S)).hex(), j
            checked += 1
    assert checked >= 100
    random.seed(21)
    want = cheeger_ref.estimate(ei, n, 50, 'conductance')
    random.seed(21)
    res = estimate_cheeger(G, 50, definition='conductance')
    assert res[0].hex() == want[0].hex() and hexes(res[1]) == hexes(want[1])


@pytest.mark.parametrize('shape', SHAPES)
def test_philox_subsets_are_the_documented_family(dcr, monkeypatch, shape):
    from dcr import synthetic
    monkeypatch.setenv('DCR_CHEEGER', shape)
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    G = dcr(ei, n)
    seed = 0xC0FFEE_0000_0007
    for first, count in ((0, 64), (64, 200), (1024, 1000), (128, 1)):
        members = cheeger_ref.philox_members(seed, first, count, n)
        W = (count + 63) // 64
        assert np.array_equal(cheeger_ref.unpack(G.cheeger_philox_members(seed, first, W), count), members)
        want = cheeger_ref.counts(ei, members)
        assert np.array_equal(G.cheeger_philox_counts(seed, first, count), want)
        for definition in ('reference', 'conductance'):
            assert hexes(G.cheeger_philox_values(seed, first, count, definition)) == hexes(cheeger_ref.values(want, definition))


def test_philox_estimate_does_not_depend_on_the_batch(dcr):
    from dcr import synthetic
    from experiment.compute_cheeger import estimate_cheeger
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    G = dcr(ei, n)
    state = random.getstate()
    a = estimate_cheeger(G, 5000, rng='philox', seed=17, batch=64)
    b = estimate_cheeger(G, 5000, rng='philox', seed=17, batch=4096)
    c = estimate_cheeger(G, 5000, rng='philox', seed=17, batch=100)
    assert random.getstate() == state   # Python's stream is not involved
    assert len(a[1]) == 5000 and hexes(a[1]) == hexes(b[1]) == hexes(c[1]) and a[0].hex() == b[0].hex() == c[0].hex()
    assert a[0] == min(a[1])
    want = cheeger_ref.values(cheeger_ref.counts(ei, cheeger_ref.philox_members(17, 0, 300, n)))
    assert hexes(a[1][:300]) == hexes(want)
    assert hexes(estimate_cheeger(G, 300, rng='philox', seed=18)[1]) != hexes(a[1][:300])


def test_philox_member_share(dcr, s100k):
    """64 x 100,000 bits: share within 0.5 +- 0.001 (sigma = 0.5 / sqrt(6.4e6) ~ 0.0002, so 5 sigma)."""
    ei, n = s100k
    words = dcr(ei, n).cheeger_philox_members(2024, 0, 1)
    assert words.shape == (n, 1)
    ones = int(np.unpackbits(words.view(np.uint8)).sum())
    share = ones / (64 * n)
    print('member share', share)
    assert abs(share - 0.5) <= 0.001


def test_counts_follow_edits_and_sdrf_iterations(dcr):
    import torch
    from dcr import synthetic
    from dcr.data import Data
    from rewiring.sdrf_no_cuda import SdrfRun
    ei, n = synthetic.powerlaw_graph(400, 4, seed=3)
    G = dcr(ei, n)
    members = random_members(100, n, seed=4)
    check_counts(G, ei, members)
    rng = np.random.Generator(np.random.PCG64(6))
    for _ in range(40):   # enough appends at one node to outgrow its row's slack (the rows are laid out again)
        v = int(rng.integers(1, n))
        if not G.has_edge(0, v):
            G.add_edge(0, v)
    eu, ev = G.edges()
    for k in range(0, 60, 3):
        G.remove_edge(int(eu[k]), int(ev[k]))
    check_counts(G, G.to_edge_index(), members)
    np.random.seed(0)
    run = SdrfRun(Data(edge_index=torch.from_numpy(ei), num_nodes=n), 'bfc', True, 0.5, 50)
    for i in range(50):
        assert run.step(more=i + 1 < 50)
    now = run.G.to_edge_index()
    assert not np.array_equal(now, ei)
    check_counts(run.G, now, members)


def test_cheeger_calls_leave_the_curvature_buffer_alone(dcr):
    from dcr import synthetic
    from experiment.compute_cheeger import estimate_cheeger
    ei, n = synthetic.powerlaw_graph(20000, 2, seed=4)
    G = dcr(ei, n)
    G.curvature_pass('bfc')
    before = [a.tobytes() for a in G.curvature_read()]
    random.seed(1)
    estimate_cheeger(G, 100, batch=64)
    estimate_cheeger(G, 100, rng='philox', seed=3)
    G.cheeger_counts(random_members(10, n, seed=1))
    assert [a.tobytes() for a in G.curvature_read()] == before   # no pass in between: curv_valid still set, same bytes
    assert G.argext(False)[:2] == G.argext(False)[:2]


@pytest.mark.parametrize('incremental', ['0', '1'])
def test_sdrf_replay_with_cheeger_calls_in_between(monkeypatch, incremental):
    """tests/golden/sdrf_traces_small.json replayed with an estimate between the iterations, traced (host draw) and untraced
    (device draw, the next pass enqueued behind the edit): same iterations, same final edge list."""
    import torch
    from dcr.data import Data
    from experiment.compute_cheeger import estimate_cheeger
    from rewiring.sdrf_no_cuda import SdrfRun
    monkeypatch.setenv('DCR_INCREMENTAL', incremental)
    for case in load_golden('sdrf_traces_small.json')['cases']:
        if case['error']:
            continue
        tau = float('inf') if case['tau'] == 'inf' else case['tau']
        label = (case['graph'], case['curv_type'], case['loops'], case['tau'], case['seed'])
        for traced in (True, False):
            data = Data(edge_index=torch.tensor(case['edge_index']), num_nodes=case['num_nodes'])
            trace = [] if traced else None
            np.random.seed(case['seed'])
            random.seed(0)
            run = SdrfRun(data, case['curv_type'], case.get('remove_edges', True), case['removal_bound'], tau, trace=trace)
            assert run.incremental == (incremental == '1')
            for i in range(case['loops']):
                estimate_cheeger(run.G, 70, batch=64)
                more = run.step(more=i + 1 < case['loops'])
                estimate_cheeger(run.G, 10, rng='philox', seed=i)
                if not more:
                    break
            if traced:
                ref = case['iterations']
                assert len(trace) == len(ref), label
                for it, (a, b) in enumerate(zip(trace, ref)):
                    assert b['argmin'] is None or a['argmin'] == b['argmin'], (label, it)
                    assert a['candidates'] == b['candidates'], (label, it)
                    assert hexes(a['improvements']) == [fh(h).hex() for h in b['improvements']], (label, it)
                    assert (a['choice'], a['added'], a['removed']) == (b['choice'], b['added'], b['removed']), (label, it)
            assert run.result().edge_index.tolist() == case['final_edge_index'], (label, traced)
