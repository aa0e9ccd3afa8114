"""Hop distances on the device (csrc/dcr_hops.hip) against tests/hops_ref.py, every value by ==: the results are integers and the
reference is exact (tests/test_hops_cpu.py holds it against scipy on every graph used here), so nothing is skipped, filtered or
given a tolerance.  Shapes are the smallest at which each piece can go wrong: degenerate and disconnected graphs, more levels
than an 8-bit counter holds, every row class at its workgroup, wave and turn boundaries, every batch width and the source counts
either side of them, the hop limit, a graph edited between queries.  The last section runs the sizes of tests/scale_ref.py, where
the level kernel has thousands of workgroups and the count kernel's capped grid takes a second trip."""
import ctypes
import time

import numpy as np
import pytest

import hops_ref
import spectral_ref

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name, ei, n):
    """The reference over ALL sources of a named graph, computed once and never written to."""
    if name not in _REF:
        out = hops_ref.hops(ei, n)
        for a in out:
            a.setflags(write=False)
        _REF[name] = out
    return _REF[name]


def graph(ei, n):
    from dcr.graph import DcrGraph
    return DcrGraph(ei, n)


def plan_graph(name):
    return next((ei, n) for nm, ei, n in spectral_ref.plan_family() if nm == name)


def check(G, name, ei, n, sources=None, max_hops=None):
    """hop_distances and hop_summary of one call against the reference rows of the same sources."""
    if max_hops is None:
        dist, ecc, reached, total = (a if sources is None else a[np.asarray(sources, dtype=np.int64)] for a in reference(name, ei, n))
    else:
        dist, ecc, reached, total = hops_ref.hops(ei, n, sources, max_hops=max_hops)
    src = np.arange(n) if sources is None else sources
    got = G.hop_distances(src, max_hops=max_hops)
    assert got.dtype == np.int32 and got.shape == dist.shape and np.array_equal(got, dist), name
    e, r, t = G.hop_summary(sources, max_hops=max_hops)
    assert (e.dtype, r.dtype, t.dtype) == (np.int32, np.int64, np.int64)
    assert np.array_equal(e, ecc) and np.array_equal(r, reached) and np.array_equal(t, total), name
    return got, e, r, t


@pytest.mark.parametrize('name,ei,n', hops_ref.degenerate(), ids=[g[0] for g in hops_ref.degenerate()])
def test_degenerate_graphs(name, ei, n):
    got, e, r, t = check(graph(ei, n), name, ei, n)
    comps, labels = spectral_ref.components(ei, n)
    assert np.array_equal(got >= 0, labels[:, None] == labels[None, :])          # -1 exactly across components
    assert np.array_equal(r, np.bincount(labels, minlength=n)[labels])            # reached = the component's size
    isolated = np.bincount(np.asarray(ei[0], dtype=np.int64), minlength=n) == 0
    assert (e[isolated] == 0).all() and (r[isolated] == 1).all() and (t[isolated] == 0).all()
    if comps > 1:
        assert (got == -1).any() and (r < n).all()


def test_path_of_300_has_299_levels():
    ei, n = spectral_ref.path(300)
    got, e, r, t = check(graph(ei, n), 'path300', ei, n, np.array([0, 299, 150]))
    assert e.tolist() == [299, 299, 150] and r.tolist() == [300] * 3 and t.tolist() == [299 * 300 // 2, 299 * 300 // 2, 2 * (150 * 151 // 2) - 150]
    assert np.array_equal(got[0], np.arange(300)) and got.max() == 299            # past any 8-bit level counter


def test_cycle_of_257():
    ei, n = spectral_ref.cycle(257)
    _, e, r, t = check(graph(ei, n), 'cycle257', ei, n)
    assert (e == 128).all() and (r == 257).all() and (t == 128 * 129).all()


@pytest.mark.parametrize('name', spectral_ref.PLAN_NAMES)
def test_every_row_class_with_all_sources(name):
    ei, n = plan_graph(name)
    check(graph(ei, n), name, ei, n)


def test_star_with_a_long_hub_row():
    ei, n = hops_ref.hub_star(2100)
    G = graph(ei, n)
    assert G.degree(0) == 2100
    got, e, r, t = check(G, 'hub_star', ei, n, np.array([0, 1, 2100]))
    assert e.tolist() == [1, 2, 2] and r.tolist() == [2101] * 3 and t.tolist() == [2100, 1 + 2 * 2099, 1 + 2 * 2099]


def boundary_sources(P):
    """P sources of the 330-node graph with repeats among them, the isolated nodes 328 and 329 included where P allows."""
    src = np.random.Generator(np.random.PCG64(100 + P)).integers(0, 330, size=P)
    if P >= 63:
        src[[5, P - 1]] = 329, 328
        src[P // 2] = src[0]
    return src.astype(np.int32)


@pytest.mark.parametrize('P', [1, 63, 64, 65, 255, 256, 257, 321])
def test_batch_boundaries(P):
    ei, n = hops_ref.irregular330()
    src = boundary_sources(P)
    assert P < 63 or np.unique(src).size < P                                      # duplicated sources, each with a bit of its own
    check(graph(ei, n), 'irregular330', ei, n, src)


@pytest.mark.parametrize('words', ['1', '2', '4'])
def test_every_batch_width_gives_the_same_bits(words, monkeypatch):
    """DCR_HOPS_W fixes the words of a batch: 321 sources as 6 batches of 64, 3 of 128, 2 of 256, the last one partly filled."""
    ei, n = hops_ref.irregular330()
    monkeypatch.setenv('DCR_HOPS_W', words)
    check(graph(ei, n), 'irregular330', ei, n, boundary_sources(321))
    ei, n = plan_graph('long3_mid9_short63')
    check(graph(ei, n), 'long3_mid9_short63', ei, n, np.arange(0, n, 7, dtype=np.int32))


def test_placement_independence():
    ei, n = hops_ref.irregular330()
    G = graph(ei, n)
    rng = np.random.Generator(np.random.PCG64(5))
    s = 17
    alone = (G.hop_distances([s]), *G.hop_summary([s]))
    for P, at in ((64, 63), (65, 64), (200, 0), (300, 257), (321, 130)):
        src = rng.integers(0, n, size=P).astype(np.int32)
        src[at] = s
        dist = G.hop_distances(src)
        e, r, t = G.hop_summary(src)
        assert np.array_equal(dist[at], alone[0][0]) and (e[at], r[at], t[at]) == (alone[1][0], alone[2][0], alone[3][0])


def test_summary_equals_the_summaries_of_the_rows():
    for name, (ei, n) in (('irregular330', hops_ref.irregular330()), ('three_components', hops_ref.degenerate()[-1][1:])):
        G = graph(ei, n)
        dist = G.hop_distances(np.arange(n))
        e, r, t = G.hop_summary()
        we, wr, wt = hops_ref.summaries_of(dist)
        assert np.array_equal(e, we) and np.array_equal(r, wr) and np.array_equal(t, wt), name


@pytest.mark.parametrize('max_hops', [0, 1, 2, 1000])
def test_hop_limit(max_hops):
    from experiment.hop_metrics import ball_sizes
    for name, (ei, n) in (('irregular330', hops_ref.irregular330()), ('three_components', hops_ref.degenerate()[-1][1:]),
                          ('mid5_short9', plan_graph('mid5_short9'))):
        G = graph(ei, n)
        src = np.arange(0, n, 3, dtype=np.int32)
        _, e, r, t = check(G, name, ei, n, src, max_hops=max_hops)
        if max_hops == 0:
            assert (e == 0).all() and (r == 1).all() and (t == 0).all()
        if max_hops == 1000:
            assert np.array_equal(r, reference(name, ei, n)[2][src])
        want = hops_ref.hops(ei, n, None, max_hops=max_hops)[2]
        assert np.array_equal(ball_sizes(G, max_hops), want)
        assert np.array_equal(ball_sizes(G, max_hops, src), want[src])


def test_live_graph_after_edits():
    ei, n = spectral_ref.path(300)
    G = graph(ei, n)
    src = np.array([0, 299, 150, 10, 250, 100, 101], dtype=np.int32)
    check(G, 'path300', ei, n, src)
    G.add_edge(10, 250)                                                            # a chord across the path
    chord = hops_ref.with_edge(ei, n, 10, 250)
    _, e, _, _ = check(G, 'path300_chord', *chord, src)
    assert e[0] < 299
    G.remove_edge(100, 101)                                                        # on the cycle the chord closed: still connected
    cut = hops_ref.with_edge(*chord, 100, 101, remove=True)
    _, _, r, _ = check(G, 'path300_chord_cut', *cut, src)
    assert (r == 300).all()
    G.remove_edge(5, 6)                                                            # a bridge: nodes 0 .. 5 split off
    split = hops_ref.with_edge(*cut, 5, 6, remove=True)
    got, _, r, _ = check(G, 'path300_split', *split, src)
    assert r.tolist() == [6] + [294] * 6 and (got[0, 6:] == -1).all()
    check(G, 'path300_split', *split)                                              # and every node as a source


def test_live_graph_after_fosr():
    from experiment.hop_metrics import aggregate, hop_metrics
    ei, n = hops_ref.irregular330()
    G = graph(ei, n)
    before = hop_metrics(G)
    edges = G.fosr(10)
    assert edges.shape == (2, 10)
    after_ei = np.concatenate([ei, edges, edges[::-1]], axis=1)
    _, e, r, t = check(G, 'irregular330_fosr10', after_ei, n)
    after = hop_metrics(G)
    want = aggregate(e, r, t, spectral_ref.components(after_ei, n)[1])
    ref0 = reference('irregular330', ei, n)
    assert before['diameter'] == int(ref0[1].max()) and before['exact']
    for key in ('diameter', 'radius', 'average_path_length', 'largest_component', 'exact'):
        assert after[key] == want[key], key
    assert np.array_equal(after['eccentricity'], e)


def test_hop_metrics_takes_a_data_object_and_a_sample():
    import torch
    from dcr.data import Data
    from experiment.hop_metrics import aggregate, draw_sources, hop_metrics
    name, ei, n = hops_ref.degenerate()[-1]
    m = hop_metrics(Data(edge_index=torch.from_numpy(ei), num_nodes=n), sources=20, seed=2)
    src = draw_sources(n, 20, seed=2)
    ref = reference(name, ei, n)
    want = aggregate(ref[1][src], ref[2][src], ref[3][src], spectral_ref.components(ei, n)[1], src)
    assert not m['exact'] and m['num_sources'] == 20
    for key in ('diameter', 'radius', 'average_path_length', 'largest_component'):
        assert m[key] == want[key] or (m[key] != m[key] and want[key] != want[key]), key
    assert m['diameter'] <= int(ref[1].max())                                      # a sample's diameter is a lower bound


def test_two_identical_calls_return_identical_arrays():
    ei, n = hops_ref.irregular330()
    G = graph(ei, n)
    src = boundary_sources(321)
    a, b = G.hop_distances(src), G.hop_distances(src)
    assert a is not b and a.tobytes() == b.tobytes()
    for x, y in zip(G.hop_summary(src), G.hop_summary(src)):
        assert x.tobytes() == y.tobytes()
    H = graph(ei, n)                                                               # and another handle of the same graph
    assert H.hop_distances(src).tobytes() == a.tobytes()


def test_bad_input():
    from dcr import _lib
    ei, n = hops_ref.irregular330()
    G = graph(ei, n)
    for bad in (n, -1):
        with pytest.raises(ValueError):
            G.hop_distances([0, bad])
        with pytest.raises(ValueError):
            G.hop_summary([bad])
        src = np.array([0, bad], dtype=np.int32)                                   # the library's own check, behind the wrapper's
        ecc = np.zeros(2, dtype=np.int32)
        rc = _lib.lib().dcr_hop_distances(G._h, src.ctypes.data_as(_lib._i32p), 2, None, None, ecc.ctypes.data_as(_lib._i32p), None, None)
        assert rc == -1 and b'source' in _lib.lib().dcr_last_error()
    assert _lib.lib().dcr_hop_distances(G._h, None, n - 1, None, None, None, None, None) == -1   # NULL sources: P must be n
    with pytest.raises(ValueError):
        G.hop_summary([0], max_hops=-2)
    dist = G.hop_distances([])
    assert dist.shape == (0, n) and dist.dtype == np.int32
    assert [a.shape for a in G.hop_summary([])] == [(0,)] * 3
    e, r, t = G.hop_summary([3])                                                   # any of the outputs may be NULL
    only = ctypes.c_int64()
    src = np.array([3], dtype=np.int32)
    assert _lib.lib().dcr_hop_distances(G._h, src.ctypes.data_as(_lib._i32p), 1, None, None, None, ctypes.byref(only), None) == 0
    assert only.value == r[0]


# ---- many workgroups of k_hop_level, and k_hop_count past HOP_COUNT_BLOCKS ------------------------------------------------------------
# tests/test_scale_thresholds_cpu.py says what each size reaches; the reference is hops_ref.hops_sparse, which tests/test_hops_cpu.py
# holds against hops_ref.hops on every small graph and against scipy at 70,001 nodes.  Both graphs end in a path of 1,000 nodes
# that no chord reaches, so a search takes about a thousand levels: the tests print them.
_BIG = {}


def big(name):
    """(DcrGraph, edge_index, n) of scale_ref.whole_small() / fosr_large(), one handle a graph."""
    import scale_ref as sc
    if name not in _BIG:
        ei, n = sc.whole_small() if name == 'small' else sc.fosr_large()
        _BIG[name] = (graph(ei, n), ei, n)
    return _BIG[name]


def big_reference(key, name, sources, **kw):
    """hops_sparse of one source list on a big graph, computed once and never written to."""
    if key not in _REF:
        _, ei, n = big(name)
        t0 = time.perf_counter()
        out = hops_ref.hops_sparse(ei, n, sources, **kw)
        print(f'  host reference {key}: {time.perf_counter() - t0:.2f} s')
        for a in out:
            if a is not None:
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def equal_summaries(got, want, label):
    e, r, t = got
    assert (e.dtype, r.dtype, t.dtype) == (np.int32, np.int64, np.int64)
    assert np.array_equal(e, want[1]) and np.array_equal(r, want[2]) and np.array_equal(t, want[3]), label


def test_rows_and_summary_at_70001_nodes():
    import scale_ref as sc
    G, ei, n = big('small')
    src = sc.hop_sources_small()
    want = big_reference('small21', 'small', src)
    G.hop_summary(src[:1], max_hops=1)                                            # buffers and code objects
    t0 = time.perf_counter()
    dist = G.hop_distances(src)
    t1 = time.perf_counter()
    got = G.hop_summary(src)
    t2 = time.perf_counter()
    print(f'  n = {n}, {src.size} sources: levels {got[0].max()}, hop_distances {1e3 * (t1 - t0):.1f} ms, hop_summary {1e3 * (t2 - t1):.1f} ms')
    assert dist.dtype == np.int32 and dist.shape == (src.size, n) and np.array_equal(dist, want[0])
    equal_summaries(got, want, 'whole_small')
    assert got[1][:6].tolist() == [n - 3, n - 3, n - 3, 1, 1, n - 3] and (dist[:, -3:] == -1).sum() == 3 * src.size - 2


@pytest.mark.parametrize('words', ['1', '2', '4'])
def test_summary_at_262182_nodes(words, monkeypatch):
    """130 sources under every batch width, so each k_hop_count<W> and k_hop_level<W> takes the capped grid.  A connected source
    reaches 262,145 nodes: node 262,144 is the one connected node that only the second trip of the count kernel sees."""
    import scale_ref as sc
    G, ei, n = big('large')
    src = sc.hop_sources_large()
    want = big_reference('large130', 'large', src, rows=False)
    monkeypatch.setenv('DCR_HOPS_W', words)
    G.hop_summary(src[:1], max_hops=1)
    t0 = time.perf_counter()
    got = G.hop_summary(src)
    print(f'  n = {n}, {src.size} sources, W = {words}: levels {got[0].max()}, hop_summary {1e3 * (time.perf_counter() - t0):.1f} ms')
    equal_summaries(got, want, words)
    connected = src < n - 37
    assert connected.sum() >= 120 and (got[1][connected] == 262_145).all() and (got[1][~connected] == 1).all()
    assert got[0][src == 262_144].min() == got[0].max() >= 1_000                  # the end of the tail is the farthest node


def test_rows_at_262182_nodes():
    """Three sources, one word: the batch's block on the device is 3 x n int32 of a buffer of 64 x n (67 MB).  The source at node
    262,144 writes its distance 0 at dist[i * n + s] from k_hop_init at the far end of a row."""
    G, ei, n = big('large')
    src = np.array([262_144, 0, n - 1], dtype=np.int32)
    want = big_reference('large3', 'large', src)
    t0 = time.perf_counter()
    dist = G.hop_distances(src)
    print(f'  n = {n}, 3 sources: levels {want[1].max()}, hop_distances {1e3 * (time.perf_counter() - t0):.1f} ms')
    assert dist.dtype == np.int32 and dist.shape == (3, n)
    assert (dist[:2, 262_144] >= 0).all() and dist[0, 262_144] == 0 and (dist[:2, -1] == -1).all()
    assert dist[2, -1] == 0 and (dist[2, :-1] == -1).all()                        # the isolated source: its own node alone
    assert np.array_equal(dist, want[0])
    equal_summaries(G.hop_summary(src), want, 'three sources')


def test_hop_limit_at_262182_nodes():
    from experiment.hop_metrics import ball_sizes
    import scale_ref as sc
    G, ei, n = big('large')
    src = sc.hop_sources_large()
    want = big_reference('large130_2hops', 'large', src, max_hops=2, rows=False)
    t0 = time.perf_counter()
    got = G.hop_summary(src, max_hops=2)
    print(f'  n = {n}, {src.size} sources, max_hops = 2: hop_summary {1e3 * (time.perf_counter() - t0):.1f} ms')
    equal_summaries(got, want, 'max_hops = 2')
    assert got[0].max() == 2 and got[1][src == 262_144].tolist() == [3] * 5         # the end of a path: itself and two more
    assert np.array_equal(ball_sizes(G, 2, src), want[2])


def test_two_identical_calls_at_262182_nodes():
    import scale_ref as sc
    G, ei, n = big('large')
    src = sc.hop_sources_large()
    first, second = G.hop_summary(src), G.hop_summary(src)
    for x, y in zip(first, second):
        assert x is not y and x.tobytes() == y.tobytes()
    few = src[[0, 1, 5]]
    a, b = G.hop_distances(few), G.hop_distances(few)
    assert a is not b and a.tobytes() == b.tobytes()
