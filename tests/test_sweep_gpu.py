"""The sweep cut on the GPU (csrc/dcr_sweep.hip) against the numpy restatement tests/sweep_ref.py, bit for bit: no tolerance
anywhere but the theorem lambda_1 / 2 <= conductance <= sqrt(2 lambda_1), which needs none.  Run the file under a time limit
(``timeout 300 pytest -m gpu ...``): no test loops around a failing step."""
import ctypes
import warnings

import numpy as np
import pytest

import scale_ref
import spectral_ref
import sweep_ref

pytestmark = pytest.mark.gpu

DEFINITIONS = ['reference', 'conductance']


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


def assert_same(got, want, label=''):
    assert got.order.dtype == np.int32 and np.array_equal(got.order, want.order), label
    if got.profile is not None:
        assert got.profile.tobytes() == want.profile.tobytes(), label
    assert (got.value == want.value or (np.isinf(got.value) and np.isinf(want.value))) and got.size == want.size, (label, got.value, want.value, got.size, want.size)
    assert got.counts.dtype == np.int64 and np.array_equal(got.counts, want.counts), label


# ---- 1. the sort alone ---------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e308, -1e308, 1.0, -1.0])


def score_families(n, rng):
    x = rng.standard_normal(n)
    base = np.float64(1.5)
    low_byte = (np.full(n, base).view(np.uint64) + rng.integers(0, 256, n).astype(np.uint64)).view(np.float64)
    mix = rng.choice(SPECIALS, n)
    return {
        'normal': x,
        'seven_values': rng.integers(0, 7, n).astype(np.float64) - 3.0,
        'all_equal': np.full(n, 2.5),
        'sorted': np.sort(x),
        'reverse_sorted': np.sort(x)[::-1].copy(),
        'lowest_mantissa_byte': low_byte,
        'sign_only': np.where(rng.integers(0, 2, n) == 0, -1.0, 1.0) * 0.75,
        'specials': mix,
    }


@pytest.mark.parametrize('n', [2, 63, 64, 65, 1023, 1024, 1025, 4097, 70001])
def test_order_is_the_lexsort(dcr, n):
    ei, _ = spectral_ref.path(n)
    G = dcr(ei, n)
    rng = np.random.Generator(np.random.PCG64(n))
    for name, score in score_families(n, rng).items():
        got = G.sweep_cut(score).order
        assert np.array_equal(got, sweep_ref.order_of(score)), (n, name)


# Sizes past the scans' closing stride and the tile limit (tests/test_scale_thresholds_cpu.py says which boundary each one is past):
# a single edge, since the sort does not read the graph, and the families that can tell a wrong carry or tile bound: distinct
# keys, ties that must keep id order through every pass and across tile borders, and the special values.  np.lexsort of 4.2M keys
# takes a second, so the largest size runs two families.
LARGE_SORTS = [(n, name) for n in scale_ref.SORT_SIZES for name in ('normal', 'seven_values', 'specials')
               if not (n == scale_ref.SORT_SIZES[2] and name == 'specials')]


@pytest.mark.parametrize('n,name', LARGE_SORTS)
def test_order_is_the_lexsort_past_the_closing_strides(dcr, n, name):
    ei, _ = scale_ref.single_edge(n)
    rng = np.random.Generator(np.random.PCG64(n))    # the one family: all eight of score_families cost seconds at these sizes
    score = {'normal': lambda: rng.standard_normal(n), 'seven_values': lambda: rng.integers(0, 7, n).astype(np.float64) - 3.0,
             'specials': lambda: rng.choice(SPECIALS, n)}[name]()
    got = dcr(ei, n).sweep_cut(score).order
    want = sweep_ref.order_of(score)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (n, name, bad.size, bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())


# ---- 2. the whole call -----------------------------------------------------------------------------------------------------------
def whole_call_graphs():
    from dcr import synthetic
    er, ner = synthetic.erdos_renyi_graph(200, 0.05, seed=1)
    return {
        'single_edge': spectral_ref.path(2),
        'path5': spectral_ref.path(5),
        'star3000': spectral_ref.star(3001),
        'grid12x9': synthetic.grid_graph(12, 9),
        'powerlaw300': synthetic.powerlaw_graph(300, 2, seed=3),
        'er200_plus_isolated': (er, ner + 10),
        # every value inf under both definitions (test_every_prefix_has_a_zero_volume has the case with an edge)
        'no_edges': (np.zeros((2, 0), dtype=np.int64), 6),
    }


@pytest.mark.parametrize('definition', DEFINITIONS)
@pytest.mark.parametrize('name', list(whole_call_graphs()))
def test_whole_call_bit_exact(dcr, name, definition):
    ei, n = whole_call_graphs()[name]
    G = dcr(ei, n)
    rng = np.random.Generator(np.random.PCG64(99))
    for score in (rng.standard_normal(n), rng.integers(0, 4, n).astype(np.float64), np.arange(n, dtype=np.float64)):
        got = G.sweep_cut(score, definition=definition, return_profile=True)
        assert_same(got, sweep_ref.sweep(ei, n, score, definition), name)
    if name == 'no_edges':
        assert np.isinf(got.value) and got.size == 1 and np.isinf(got.profile).all()


_LARGE = {}


def large_case(size, score_name):
    """(edge_index, n, score, the counts of sweep_ref.prefix_counts): computed once, for both definitions."""
    if (size, score_name) not in _LARGE:
        ei, n = {scale_ref.WHOLE_SMALL: scale_ref.whole_small, scale_ref.WHOLE_LARGE: scale_ref.whole_large,
                 scale_ref.WHOLE_CARRY: scale_ref.whole_carry}[size]()
        rng = np.random.Generator(np.random.PCG64(size))
        score = {'normal': rng.standard_normal(n), 'four_values': rng.integers(0, 4, n).astype(np.float64),
                 'arange': np.arange(n, dtype=np.float64)}[score_name]
        _LARGE[size, score_name] = (ei, n, score, sweep_ref.prefix_counts(ei, n, score))
    return _LARGE[size, score_name]


@pytest.mark.parametrize('definition', DEFINITIONS)
@pytest.mark.parametrize('size', [scale_ref.WHOLE_SMALL, scale_ref.WHOLE_LARGE, scale_ref.WHOLE_CARRY])
def test_whole_call_bit_exact_past_the_closing_strides(dcr, size, definition):
    """70,001 nodes: more than 256 arg-min partials, all three row classes in k_sweep_edges.  524,289 nodes: a second grid-stride
    trip of k_sweep_keys and k_sweep_value, 257 blocks of the difference arrays' scan, 37 isolated nodes at the end.  525,788
    nodes: the same, and prefixes that read the 257th block, so a wrong carry shows (at 524,289 that block holds the count of
    the whole node set alone, which nothing reads).  With the node id as score the best prefix is found by a workgroup whose
    partial the closing loop reaches on a later trip (tests/test_scale_thresholds_cpu.py)."""
    G = None
    for score_name in ('normal', 'four_values', 'arange'):
        ei, n, score, counts = large_case(size, score_name)
        G = G or dcr(ei, n)
        got = G.sweep_cut(score, definition=definition, return_profile=True)
        assert_same(got, sweep_ref.from_counts(counts, definition), (size, score_name, definition))
        assert np.isfinite(got.value) and 1 <= got.size < n


def test_every_prefix_has_a_zero_volume(dcr):
    """One edge between the first and the last node of the order: under the reference definition 2 in = 0 for every proper prefix,
    so every value is inf and the answer is k = 1."""
    n = 9
    ei, _ = spectral_ref._und([(0, n - 1)], n)
    G = dcr(ei, n)
    score = np.arange(n, dtype=np.float64)
    got = G.sweep_cut(score, definition='reference', return_profile=True)
    assert_same(got, sweep_ref.sweep(ei, n, score, 'reference'))
    assert np.isinf(got.profile).all() and np.isinf(got.value) and got.size == 1 and got.counts.tolist() == [0, 1, 0, 0]


# ---- 3. / 4. live adjacency, and the counting kernel of the Monte-Carlo estimate -----------------------------------------------------
def test_live_adjacency_and_cheeger_counts(dcr):
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(2000, 3)
    G = dcr(ei, n)
    rng = np.random.Generator(np.random.PCG64(8))
    edits = 0
    while edits < 200:
        if edits % 2 == 0:
            u, v = (int(x) for x in rng.integers(0, n, 2))
            if u == v or G.has_edge(u, v):
                continue
            G.add_edge(u, v)
        else:
            eu, ev = G.edges()
            k = int(rng.integers(0, eu.shape[0]))
            G.remove_edge(int(eu[k]), int(ev[k]))
        edits += 1
    live = G.to_edge_index()
    assert not np.array_equal(live, ei)
    score = rng.standard_normal(n)
    for definition in DEFINITIONS:
        got = G.sweep_cut(score, definition=definition, return_profile=True)
        assert_same(got, sweep_ref.sweep(live, n, score, definition), definition)
        rank = np.empty(n, dtype=np.int64)
        rank[got.order] = np.arange(n)
        members = rank < got.size
        assert np.array_equal(G.cheeger_counts(members[None, :])[0], got.counts)


# ---- 5. the Fiedler path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sweep_ref.table_graphs(), ids=lambda c: c[0])
def test_fiedler_sweep(dcr, case):
    from experiment.cheeger_bounds import cheeger_sweep
    name, (ei, n), _, _, _, _ = case
    G = dcr(ei, n)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        plain = G.spectral_gap(seed=3)
        gap, cut, score = G.fiedler_sweep(seed=3)
        gap2, cut2, score2 = G.fiedler_sweep(seed=3)
    print(f'  {name}: lambda1/2={gap.lambda1 / 2!r} value={cut.value!r} k={cut.size} sqrt(2 lambda1)={np.sqrt(2 * gap.lambda1)!r}')
    assert gap == plain   # every field, vector None in both
    assert gap.lambda1.hex() == plain.lambda1.hex() and gap.residual.hex() == plain.residual.hex()
    assert_same(cut, sweep_ref.sweep(ei, n, score, 'conductance'), name)
    assert score.tobytes() == score2.tobytes() and gap == gap2
    assert_same(cut2, cut, name)
    assert gap.lambda1 / 2 <= cut.value <= np.sqrt(2 * gap.lambda1)
    if name == 'barbell20_4':
        assert cut.value == 1 / 385 and cut.size == 22
        assert (cut.counts[0], cut.counts[1] + cut.counts[2], cut.counts[3]) == (192, 1, 192)
    # the user-facing function: the side of smaller volume, whose conductance is the value
    for definition in DEFINITIONS:
        value, members, lam = cheeger_sweep(G, definition=definition, seed=3)
        assert lam == gap.lambda1 and members.dtype == np.bool_ and members.shape == (n,)
        a, b = sweep_ref.undirected_edges(ei)
        deg = np.bincount(np.concatenate([a, b]), minlength=n)
        assert 0 < deg[members].sum() <= deg[~members].sum()
        c_in, c_lo, c_hi, _ = G.cheeger_counts(members[None, :])[0]
        if definition == 'conductance':
            assert value == cut.value and value == (c_lo + c_hi) / deg[members].sum()
        else:
            both = [sweep_ref.sweep(ei, n, s, 'reference').value for s in (score, -score)]
            assert value == min(both)


# ---- 6. read-only ------------------------------------------------------------------------------------------------------------------
def test_read_only(dcr):
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(300, 2, seed=3)
    G = dcr(ei, n)
    G.curvature_pass('bfc')
    before = [np.array(x).tobytes() for x in G.curvature_read()]
    G.sweep_cut(np.random.Generator(np.random.PCG64(1)).standard_normal(n), return_profile=True)
    G.fiedler_sweep()
    after = [np.array(x).tobytes() for x in G.curvature_read()]
    assert before == after
    assert np.array_equal(G.to_edge_index(), dcr(ei, n).to_edge_index())


# ---- 7. bad arguments --------------------------------------------------------------------------------------------------------------
def test_errors(dcr):
    from dcr import _lib
    ei, n = spectral_ref.path(5)
    G = dcr(ei, n)
    L = _lib.lib()
    res, gap = _lib.SweepResult(), _lib.SpectralResult()
    score = np.arange(5, dtype=np.float64)
    sp = score.ctypes.data_as(_lib._f64p)
    with pytest.raises(ValueError, match='NaN'):
        G.sweep_cut(np.array([0.0, 1.0, np.nan, 2.0, 3.0]))
    with pytest.raises(ValueError):
        G.sweep_cut(np.zeros(4))
    with pytest.raises(ValueError):
        G.sweep_cut(np.zeros((5, 1)))
    with pytest.raises(KeyError):
        G.sweep_cut(score, definition='other')
    assert L.dcr_sweep_cut(G._h, sp, 2, ctypes.byref(res), None, None) == -1
    assert L.dcr_sweep_cut(G._h, sp, -1, ctypes.byref(res), None, None) == -1
    assert L.dcr_sweep_cut(G._h, sp, 1, None, None, None) == -1
    assert L.dcr_sweep_cut(G._h, None, 1, ctypes.byref(res), None, None) == -1
    assert L.dcr_sweep_cut(None, sp, 1, ctypes.byref(res), None, None) == -1
    assert L.dcr_fiedler_sweep(G._h, None, 2, ctypes.byref(gap), ctypes.byref(res), None, None) == -1
    assert L.dcr_fiedler_sweep(G._h, None, 1, ctypes.byref(gap), None, None, None) == -1
    assert L.dcr_fiedler_sweep(G._h, None, 1, None, ctypes.byref(res), None, None) == -1
    assert L.dcr_fiedler_sweep(None, None, 1, ctypes.byref(gap), ctypes.byref(res), None, None) == -1
    one = dcr(np.zeros((2, 0), dtype=np.int64), 1)
    with pytest.raises(ValueError):
        one.sweep_cut(np.zeros(1))
    empty = dcr(np.zeros((2, 0), dtype=np.int64), 5)
    with pytest.raises(ValueError, match='no positive eigenvalue'):
        empty.fiedler_sweep()
    # NULL options are the defaults, NULL outputs are skipped; the handle still works after the refusals
    assert L.dcr_fiedler_sweep(G._h, None, 1, ctypes.byref(gap), ctypes.byref(res), None, None) == 0
    assert res.value == G.fiedler_sweep()[1].value and gap.converged == 1
    assert L.dcr_sweep_cut(G._h, sp, 1, ctypes.byref(res), None, None) == 0
    assert res.value == sweep_ref.sweep(ei, n, score).value and res.size == sweep_ref.sweep(ei, n, score).size
