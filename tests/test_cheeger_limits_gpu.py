"""The Cheeger count kernels (csrc/dcr_cheeger.hip) at the limits tests/test_cheeger_gpu.py does not reach: every call there
launches ``k_cheeger_sliced`` with four runs per lane (tests/test_cheeger_steps_cpu.py lists them), so its counters never hold
more than 28 and the clamp of ``launch_sliced`` never acts.  Here:

  * the clamp graph of tests/cheeger_steps_ref.py at W = 200: 151 runs asked for, 146 run, every lane of workgroup 0 adds
    1,022 times and ``in``, ``lo`` and ``hi`` each reach 1,022 in one of its lanes; on a fresh handle (256 CUs assumed) and on
    one that has asked the device, both shapes, and after edits inside a saturated row;
  * the other instantiations on that graph.  WL < 16 cannot reach the clamp at a size a test can afford: it needs
    cap_total * groups >= 145 * (256 / WL) * 7 * 1,024, i.e. 16.6 M slots at W = 15, 33 M at W = 8, 66 M at W = 4, 133 M at
    W = 2 and 266 M at W = 1 (asserted in the CPU file); on the clamp graph's 1.33 M slots W = 15 runs 12 rounds (counters
    to 84, carries into plane 6) and W = 4, 2, 1 run 4.  ``planes_add1`` and ``planes_fold`` do not depend on WL, only the
    number of counters a thread converts (NB) does, and every NB is run here;
  * every W either side of every WL step, the word limit 65,535 and the first W beyond it, the argument errors of the four
    entry points, and Philox counters whose high word is not zero.

Every comparison is == on int64.  References: tests/cheeger_ref.py (plain loops) on the small graphs, ``palette_counts`` (a
K x K table of edge counts, pinned to the former on the CPU) on the large ones."""
import time

import numpy as np
import pytest

import cheeger_ref
import cheeger_steps_ref as steps

pytestmark = pytest.mark.gpu

SHAPES = ['sliced', 'lane']


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


@pytest.fixture(scope='module')
def clamp():
    """The clamp graph, its packed members [n, 200] (27 MB) and the reference counts, made once and left unchanged."""
    ei, n = steps.clamp_graph()
    pal, pw = steps.clamp_palette(steps.CLAMP_W)
    words = steps.palette_members(pal, pw)
    words.setflags(write=False)
    want = steps.palette_counts(ei, n, pal, pw)
    want.setflags(write=False)
    return dict(ei=ei, n=n, pal=pal, pw=pw, words=words, want=want, cap_total=1331200)


@pytest.fixture(scope='module')
def clamp_handle(dcr, clamp):
    """A handle on the clamp graph that never runs a curvature pass: its launches assume 256 CUs."""
    return dcr(clamp['ei'], clamp['n'])


@pytest.fixture(scope='module')
def small(dcr):
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(400, 4, seed=3)
    return ei, n


def differing(got, want):
    return np.flatnonzero((got != want).any(axis=1))[:10]


def check_one_word(G, ei, n):
    """The handle still answers: 64 subsets, W = 1."""
    rng = np.random.Generator(np.random.PCG64(77))
    members = rng.random((64, n)) < 0.5
    assert np.array_equal(G.cheeger_counts(members), cheeger_ref.counts(ei, members))


def test_clamp_graph_layout_is_the_one_the_geometry_was_computed_for(clamp, clamp_handle):
    lay = steps.slot_layout(clamp['ei'], clamp['n'])
    assert lay.cap_total == clamp['cap_total']
    G = clamp_handle
    assert G.number_of_edges() == 532480
    for v in (0, 31, 32, 16671):
        start, deg = lay.rowinfo[v]
        assert G.degree(v) == deg and G.neighbors(v) == lay.col[start:start + deg].tolist()
    eu, ev = G.edges()
    assert np.array_equal(eu[:16640], np.zeros(16640)) and np.array_equal(ev[:16640], np.arange(32, 16672))
    # what the counts of the clamp test are made of: each category reaches 1,022 in one lane of workgroup 0 (stream 0: in, hi; 1: lo)
    for stream, col in ((0, 0), (0, 2), (1, 1)):
        sub = np.stack([np.zeros(1022, dtype=np.int64), 32 + np.arange(stream, 16352, 16)])
        assert steps.palette_counts(sub, clamp['n'], clamp['pal'], clamp['pw'][:, :1])[:, col].max() == 1022


@pytest.mark.parametrize('shape', SHAPES)
def test_clamp_graph_at_146_rounds_before_and_after_the_handle_asks_the_device(dcr, clamp, monkeypatch, shape):
    """W = 200 on the clamp graph: (WL, groups, rounds, chunk, grid.x) = (16, 13, 146, 16352, 82) while the handle assumes 256
    CUs; after a pass the handle uses the device's count, the geometry may differ (printed) and the counts may not."""
    import torch
    monkeypatch.setenv('DCR_CHEEGER', shape)
    W = steps.CLAMP_W
    geom = steps.geometry(clamp['cap_total'], W, 0)
    assert geom.sliced == (16, 13, 146, 16352, 82) and geom.sliced[2] == steps.CH_MAX_ROUNDS
    G = dcr(clamp['ei'], clamp['n'])
    t0 = time.perf_counter()
    fresh = G.cheeger_counts(clamp['words'])
    t1 = time.perf_counter()
    assert fresh.shape == (64 * W, 4) and fresh.dtype == np.int64
    assert np.array_equal(fresh, clamp['want']), differing(fresh, clamp['want'])
    G.curvature_pass('1d')           # any pass makes the handle ask the device for its CU count
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t2 = time.perf_counter()
    after = G.cheeger_counts(clamp['words'])
    t3 = time.perf_counter()
    print(f'{shape}: fresh {1e3 * (t1 - t0):.1f} ms, after the pass {1e3 * (t3 - t2):.1f} ms; {cus} CUs:', steps.geometry(clamp['cap_total'], W, cus))
    assert np.array_equal(after, clamp['want']), differing(after, clamp['want'])
    assert np.array_equal(after, fresh)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('W,wl,groups,rounds', [(15, 8, 2, 12), (4, 4, 1, 4), (2, 2, 1, 4), (1, 1, 1, 4)])
def test_other_word_lane_widths_on_the_clamp_graph(clamp, clamp_handle, monkeypatch, shape, W, wl, groups, rounds):
    """The most rounds WL = 8, 4, 2, 1 reach at this size (the module docstring has the sizes at which they would clamp)."""
    monkeypatch.setenv('DCR_CHEEGER', shape)
    assert steps.geometry(clamp['cap_total'], W, 0).sliced[:3] == (wl, groups, rounds)
    pw = np.ascontiguousarray(clamp['pw'][:, 200 - W:])              # the random rows' last words, not their first
    want = steps.palette_counts(clamp['ei'], clamp['n'], clamp['pal'], pw)
    got = clamp_handle.cheeger_counts(steps.palette_members(clamp['pal'], pw))
    assert np.array_equal(got, want), differing(got, want)


STEP_WORDS = list(range(1, 19)) + [31, 32, 33]


@pytest.fixture(scope='module')
def step_cases(small):
    ei, n = small
    cases = {}
    for W in STEP_WORDS:
        B = 64 * W - 5
        rng = np.random.Generator(np.random.PCG64(1000 + W))
        members = rng.random((B, n)) < rng.random((B, 1))
        members[0], members[1] = True, False
        cases[W] = (members, cheeger_ref.counts(ei, members))
    return cases


@pytest.mark.parametrize('shape', SHAPES)
def test_every_word_count_either_side_of_every_step(dcr, small, step_cases, monkeypatch, shape):
    """W = 1..18, 31, 32, 33 with B = 64 W - 5: the partial word groups of WL = 4, 8 and 16 (W = 3; 5..7, 9..15; 17, 18, 31,
    33), a last group with one active word of 16 (W = 17, 33) and the unused bits of the last word."""
    monkeypatch.setenv('DCR_CHEEGER', shape)
    ei, n = small
    G = dcr(ei, n)
    for W in STEP_WORDS:
        members, want = step_cases[W]
        got = G.cheeger_counts(members)
        assert got.shape == want.shape and np.array_equal(got, want), (W, differing(got, want))


@pytest.fixture(scope='module')
def limit_case():
    """24 nodes, W = 65,535: 8 palette rows (12.6 MB of members) and their reference counts."""
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(24, 3, seed=1)
    W = steps.CHEEGER_MAX_WORDS
    rng = np.random.Generator(np.random.PCG64(65535))
    pw = rng.integers(0, 2 ** 64, size=(8, W), dtype=np.uint64)
    pw[0], pw[1] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)
    pw[2], pw[3] = np.uint64(0xAAAAAAAAAAAAAAAA), np.uint64(0x5555555555555555)
    pal = np.arange(n) % 8
    return ei, n, pal, pw, steps.palette_counts(ei, n, pal, pw)


@pytest.mark.parametrize('shape', SHAPES)
def test_word_limit_and_the_first_count_beyond_it(dcr, limit_case, monkeypatch, shape):
    """W = 65,535 is grid.y of the lane kernel and 4,096 word groups of the sliced one; W = 65,536 is refused (DCR_EINVAL, which
    the Python layer raises as ValueError with the library's message) and the handle goes on working."""
    monkeypatch.setenv('DCR_CHEEGER', shape)
    ei, n, pal, pw, want = limit_case
    W = steps.CHEEGER_MAX_WORDS
    assert W == 65535 and steps.geometry(steps.slot_layout(ei, n).cap_total, W, 0).sliced[:2] == (16, 4096)
    G = dcr(ei, n)
    t0 = time.perf_counter()
    got = G.cheeger_counts(steps.palette_members(pal, pw))
    print(f'{shape}: W = {W}: {1e3 * (time.perf_counter() - t0):.1f} ms')
    assert got.shape == (64 * W, 4) and np.array_equal(got, want), differing(got, want)
    with pytest.raises(ValueError, match='W out of range'):
        G.cheeger_counts(np.zeros((n, W + 1), dtype=np.uint64))
    with pytest.raises(ValueError, match='W out of range'):
        G.cheeger_philox_members(1, 0, W + 1)
    for call in (G.cheeger_philox_counts, G.cheeger_philox_values):
        with pytest.raises(ValueError, match='subset count out of range'):
            call(1, 0, 64 * W + 1)
    check_one_word(G, ei, n)


def test_argument_errors_of_the_four_entry_points(dcr, small):
    """Each is DCR_EINVAL (ValueError in Python) with its own message, found before any device work, and leaves the handle usable."""
    from dcr import _lib
    ei, n = small
    G = dcr(ei, n)
    L = _lib.lib()
    i64 = np.zeros(3 * 64, dtype=np.int64)
    f64 = np.zeros(64, dtype=np.float64)
    u64 = np.zeros(n, dtype=np.uint64)

    def refused(rc, text):
        assert rc == -1 and text in L.dcr_last_error().decode(), (rc, L.dcr_last_error())
        check_one_word(G, ei, n)

    # W = 0 (the Python layer refuses an empty packed matrix itself, so the C entry point is called as well)
    with pytest.raises(ValueError, match='W >= 1'):
        G.cheeger_counts(np.zeros((n, 0), dtype=np.uint64))
    refused(L.dcr_cheeger_counts(G._h, u64.ctypes.data, 0, i64.ctypes.data_as(_lib._i64p)), 'W out of range')
    refused(L.dcr_cheeger_philox_members(G._h, 1, 0, 0, u64.ctypes.data), 'W out of range')
    with pytest.raises(ValueError, match='W out of range'):
        G.cheeger_philox_members(1, 0, 0)
    # first negative, first not a multiple of 64
    for first in (-64, -1, 1, 32, 65):
        for call in (lambda: G.cheeger_philox_members(1, first, 1), lambda: G.cheeger_philox_counts(1, first, 64),
                     lambda: G.cheeger_philox_values(1, first, 64)):
            with pytest.raises(ValueError, match='first subset must be a non-negative multiple of 64'):
                call()
        check_one_word(G, ei, n)
    # count 0 (and below)
    for count in (0, -3):
        refused(L.dcr_cheeger_philox_counts(G._h, 1, 0, count, i64.ctypes.data_as(_lib._i64p)), 'subset count out of range')
        refused(L.dcr_cheeger_philox_values(G._h, 1, 0, count, 0, f64.ctypes.data_as(_lib._f64p)), 'subset count out of range')
    with pytest.raises(ValueError, match='subset count out of range'):
        G.cheeger_philox_counts(1, 0, 0)
    with pytest.raises(ValueError, match='subset count out of range'):
        G.cheeger_philox_values(1, 0, 0)
    # an unknown definition: a name the Python layer does not know, a code the library does not know
    with pytest.raises(KeyError):
        G.cheeger_philox_values(1, 0, 64, 'expansion')
    for code in (2, -1):
        refused(L.dcr_cheeger_philox_values(G._h, 1, 0, 64, code, f64.ctypes.data_as(_lib._f64p)), 'unknown definition')
    # null buffers
    refused(L.dcr_cheeger_counts(G._h, None, 1, i64.ctypes.data_as(_lib._i64p)), 'null argument')
    refused(L.dcr_cheeger_philox_counts(G._h, 1, 0, 64, None), 'null argument')
    # and the calls the errors stood in for
    members = cheeger_ref.philox_members(1, 0, 64, n)
    assert np.array_equal(G.cheeger_philox_counts(1, 0, 64), cheeger_ref.counts(ei, members))


@pytest.mark.parametrize('shape', SHAPES)
def test_philox_counter_with_a_high_word(dcr, monkeypatch, shape):
    """first = 64 (2^33 + 1) and 64 (2^33 + 2): membership words 2^33 + 1 (odd: the upper half of a Philox output) and 2^33 + 2,
    counter {v, 0, 0 or 1, 1}: the fourth counter word is 1 where every other test has 0."""
    from dcr import synthetic
    monkeypatch.setenv('DCR_CHEEGER', shape)
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    G = dcr(ei, n)
    seed = 0xC0FFEE_0000_0007
    low = cheeger_ref.philox_members(seed, 64, 64, n)
    for first in (64 * (2 ** 33 + 1), 64 * (2 ** 33 + 2)):
        assert (first >> 7) >> 32 == 1
        for count in (64, 200):
            members = cheeger_ref.philox_members(seed, first, count, n)
            assert not np.array_equal(members[:64], low)                 # (not the subsets of the counter's low words alone)
            W = (count + 63) // 64
            assert np.array_equal(cheeger_ref.unpack(G.cheeger_philox_members(seed, first, W), count), members), (first, count)
            want = cheeger_ref.counts(ei, members)
            assert np.array_equal(G.cheeger_philox_counts(seed, first, count), want), (first, count)
            for definition in ('reference', 'conductance'):
                got = G.cheeger_philox_values(seed, first, count, definition)
                assert [float(v).hex() for v in got] == [v.hex() for v in cheeger_ref.values(want, definition)], (first, count)


@pytest.mark.parametrize('shape', SHAPES)
def test_clamp_graph_edited_inside_a_saturated_row(dcr, clamp, monkeypatch, shape):
    """40 edges removed from the middle of hub 0's row (the row closes up: workgroup 0 still lies wholly inside it, 16,600 live
    slots) and 8 leaf-to-leaf edges added into the leaves' slack; the slots stay where they are, so the launch is the same."""
    monkeypatch.setenv('DCR_CHEEGER', shape)
    G = dcr(clamp['ei'], clamp['n'])
    gone = [32 + 8000 + k for k in range(40)]
    for leaf in gone:
        G.remove_edge(0, leaf)
    added = [(32 + 100 + k, 32 + 9000 + 3 * k) for k in range(8)]
    for a, b in added:
        G.add_edge(a, b)
    assert G.degree(0) == 16640 - 40 and G.number_of_edges() == 532480 - 40 + 8
    row = G.neighbors(0)
    assert not set(row) & set(gone) and len(set(row)) == 16600
    assert all(G.degree(a) == 33 and G.degree(b) == 33 for a, b in added) and G.degree(gone[0]) == 31
    assert steps.geometry(clamp['cap_total'], steps.CLAMP_W, 0).sliced[2] == 146 and 16352 <= 16600
    now = G.to_edge_index()
    want = steps.palette_counts(now, clamp['n'], clamp['pal'], clamp['pw'])
    assert not np.array_equal(want, clamp['want'])
    got = G.cheeger_counts(clamp['words'])
    assert np.array_equal(got, want), differing(got, want)
