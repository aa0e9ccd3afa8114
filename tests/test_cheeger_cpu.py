"""Monte-Carlo Cheeger estimate, the parts that need no GPU: the tests' own restatement (tests/cheeger_ref.py) against the
recorded outputs of the reference, the bulk Mersenne-Twister subset generator against a plain ``randint`` loop, the Philox
mapping's restatement, argument checks, and the build of the new kernels."""
import os
import random
import re
import subprocess
import tempfile

import numpy as np
import pytest

import cheeger_ref
from conftest import PKG, REPO, load_golden


def fh(s):
    return float.fromhex(s)


def case_edge_index(case):
    from dcr import synthetic
    if case['generator'] is not None:
        return synthetic.powerlaw_graph(*case['generator']['powerlaw_graph'])[0]
    return np.asarray(case['edge_index'], dtype=np.int64).reshape(2, -1)


def test_fixture_has_the_cases_the_feature_is_judged_on():
    fx = load_golden('cheeger_reference.json')
    by_name = {c['name']: c for c in fx['estimate']}
    for name in ('powerlaw400m4', 'powerlaw2485m2'):
        assert by_name[name]['iterations'] >= 200
    assert {'karate', 'grid5x5', 'karate_rewired', 'two_nodes', 'star6', 'edgeless5'} <= set(by_name)
    for name in ('two_nodes', 'star6', 'edgeless5'):
        assert fh(by_name[name]['result']) == float('inf')
    assert all(c['sec_per_draw'] > 0 for c in fx['estimate'])


def test_restatement_reproduces_the_reference_bit_for_bit():
    fx = load_golden('cheeger_reference.json')
    for case in fx['estimate']:
        ei = case_edge_index(case)
        random.seed(case['seed'])
        result, all_results = cheeger_ref.estimate(ei, case['num_nodes'], case['iterations'])
        assert [v.hex() for v in all_results] == [fh(h).hex() for h in case['all_results']], case['name']
        assert result.hex() == fh(case['result']).hex(), case['name']
        assert random.random().hex() == case['next_random'], case['name']
    by_name = {c['name']: c for c in fx['estimate']}
    for rec in fx['cheeger_S']:
        case = by_name[rec['name']]
        ei, n = case_edge_index(case), case['num_nodes']
        members = np.zeros((len(rec['subsets']), n), dtype=np.bool_)
        for j, S in enumerate(rec['subsets']):
            members[j, S] = True
        got = cheeger_ref.values(cheeger_ref.counts(ei, members))
        assert [v.hex() for v in got] == [fh(h).hex() for h in rec['values']], rec['name']


def test_conductance_restatement_is_networkx_conductance():
    import networkx as nx
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(300, 3, seed=2)
    G = cheeger_ref.to_graph(ei, n)
    rng = np.random.Generator(np.random.PCG64(1))
    members = rng.random((40, n)) < 0.5
    cnt = cheeger_ref.counts(ei, members)
    assert (cnt.sum(axis=1) == G.number_of_edges()).all()
    for j, v in enumerate(cheeger_ref.values(cnt, 'conductance')):
        assert v == nx.conductance(G, np.flatnonzero(members[j]).tolist())


@pytest.mark.parametrize('prime', ['fresh_seed', 'mid_block', 'block_edge'])
@pytest.mark.parametrize('count,n', [(1, 1), (3, 7), (50, 100), (5, 1000), (2, 20000), (0, 10), (4, 0)])
def test_bulk_subset_generator_is_the_randint_loop(prime, count, n):
    from experiment.compute_cheeger import mt_members
    random.seed(1234)
    if prime == 'mid_block':
        for _ in range(301):
            random.getrandbits(32)
    elif prime == 'block_edge':
        for _ in range(623):
            random.getrandbits(32)
    start = random.getstate()
    want = cheeger_ref.randint_members(count, n)
    want_state = random.getstate()
    random.setstate(start)
    got = mt_members(count, n)
    assert got.shape == (count, n) and got.dtype == np.bool_
    assert np.array_equal(got, want)
    assert random.getstate() == want_state
    assert random.random() == (random.setstate(want_state) or random.random())


def test_bulk_subset_generator_keeps_a_pending_gauss_value():
    from experiment.compute_cheeger import mt_members
    random.seed(5)
    random.gauss(0.0, 1.0)   # leaves the second normal deviate in the state
    start = random.getstate()
    want = cheeger_ref.randint_members(3, 50)
    want_state = random.getstate()
    random.setstate(start)
    assert np.array_equal(mt_members(3, 50), want)
    assert random.getstate() == want_state


def test_random_subset_and_host_helpers_keep_the_references_meaning():
    import networkx as nx
    from experiment import compute_cheeger as cc
    random.seed(9)
    want = {v for v in range(40) if random.randint(0, 1) == 0}
    random.seed(9)
    assert cc.random_subset(range(40)) == want
    G = nx.karate_club_graph()
    S = G.subgraph(sorted(want & set(G.nodes)))
    ei = np.array([[u for u, v in G.edges] + [v for u, v in G.edges], [v for u, v in G.edges] + [u for u, v in G.edges]])
    members = np.zeros((1, G.number_of_nodes()), dtype=np.bool_)
    members[0, list(S.nodes)] = True
    c = cheeger_ref.counts(ei, members)[0]
    assert cc.vol(S) == 2 * c[0]
    assert cc.boundary_size(G, S) == c[1]
    assert cc.cheeger_S(G, S) == cheeger_ref.value(*c)
    assert cc.cheeger_S(G, G.subgraph([])) == float('inf')
    assert cc.values_from_counts(c[None, :]).tolist() == [cheeger_ref.value(*c)]
    assert cc.values_from_counts(c[None, :], 'conductance').tolist() == [cheeger_ref.value(*c, definition='conductance')]


def test_philox_restatement_is_consistent_across_batch_splits():
    seed, n = 0x1234_5678_9ABC_DEF0, 300
    whole = cheeger_ref.philox_members(seed, 0, 400, n)
    for first, count in ((0, 64), (64, 64), (128, 200), (320, 80), (0, 1), (192, 129)):
        assert np.array_equal(cheeger_ref.philox_members(seed, first, count, n), whole[first:first + count])
    assert not np.array_equal(whole, cheeger_ref.philox_members(seed + 1, 0, 400, n))
    assert abs(whole.mean() - 0.5) < 5 * 0.5 / np.sqrt(whole.size)
    # known answer of Philox-4x32-10 (Random123 kat_vectors: zero counter and key)
    out = cheeger_ref.philox4x32_10(np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1), 0, 0)
    assert [int(w[0]) for w in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_pack_members_layout():
    from dcr.graph import pack_members
    rng = np.random.Generator(np.random.PCG64(3))
    for B, n in ((1, 5), (64, 9), (65, 4), (200, 33)):
        m = rng.random((B, n)) < 0.5
        words, count = pack_members(m, n)
        assert count == B and words.shape == (n, (B + 63) // 64) and words.dtype == np.uint64
        assert np.array_equal(cheeger_ref.unpack(words, B), m)
        assert not cheeger_ref.unpack(words, 64 * words.shape[1])[B:].any()
    with pytest.raises(ValueError):
        pack_members(np.zeros((3, 4), dtype=np.bool_), 5)
    with pytest.raises(ValueError):
        pack_members(np.zeros((3, 4), dtype=np.int32), 4)


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    import torch
    from dcr.data import Data
    from experiment.compute_cheeger import estimate_cheeger
    data = Data(edge_index=torch.tensor([[0, 1], [1, 0]]), num_nodes=2)
    state = random.getstate()
    for kw in ({'rng': 'numpy'}, {'definition': 'expansion'}, {'batch': 0}, {'batch': -4}, {'rng': 'philox'}):
        with pytest.raises(ValueError):
            estimate_cheeger(data, 10, **kw)
    with pytest.raises(ValueError):
        estimate_cheeger(data, -1)
    with pytest.raises(TypeError):
        estimate_cheeger(data, 10, 'python')   # the extras are keyword-only
    assert random.getstate() == state
    # the C entry points: -1 before any device call (no GPU is needed to see it)
    from dcr import _lib
    L = _lib.lib()
    buf = np.zeros(8, dtype=np.int64)
    p = buf.ctypes.data_as(_lib._i64p)
    assert L.dcr_cheeger_counts(None, buf.ctypes.data, 1, p) == -1                 # closed handle
    assert L.dcr_cheeger_philox_counts(None, 1, 0, 64, p) == -1
    assert L.dcr_cheeger_philox_values(None, 1, 0, 64, 0, buf.ctypes.data_as(_lib._f64p)) == -1
    assert L.dcr_cheeger_philox_members(None, 1, 0, 1, buf.ctypes.data) == -1
    assert b'null' in L.dcr_last_error()


def test_new_kernels_compile_without_warnings_and_without_scratch():
    """The flags of csrc/build.sh; the code object's resource notes, per kernel, must show no scratch memory."""
    csrc = os.path.join(PKG, 'csrc')
    flags = re.search(r'^FLAGS="(.*)"$', open(os.path.join(csrc, 'build.sh')).read(), re.M).group(1).split()
    assert 'dcr_cheeger' in open(os.path.join(csrc, 'build.sh')).read()
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), *flags, '-Rpass-analysis=kernel-resource-usage', '-c',
                            'dcr_cheeger.hip', '-o', os.path.join(tmp, 'dcr_cheeger.o')], cwd=csrc, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'warning:' not in r.stderr, r.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stderr)
    scratch = [int(x) for x in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stderr)]
    assert len(names) == len(scratch) >= 4 and any('k_cheeger_lane' in x for x in names) and \
        any('k_cheeger_sliced' in x for x in names) and any('k_cheeger_draw' in x for x in names)
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
    assert REPO
