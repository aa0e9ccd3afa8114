"""FoSR on the GPU (csrc/dcr_fosr.hip) against the numpy restatement tests/fosr_ref.py.  The pick is compared bit for bit with
the rule applied to the device's own y (and, up to 3,000 nodes, with the dense brute-force minimum); the loop's edge sequence
must equal the restatement's on fixtures whose runner-up margin tests/test_fosr_cpu.py asserts; only the iterate itself has a
tolerance, measured and recorded below.  Run the file under a time limit: no test loops around a failing step."""
import numpy as np
import pytest

import fosr_ref as ref
import scale_ref
import spectral_ref

pytestmark = pytest.mark.gpu

# Largest elementwise difference between the device's unit iterate and tests/fosr_ref.py's, as measured on an MI355X over the
# fixtures of this file, and the bound of the tests: 16 times that, which covers the spread of rounding between reduction orders.
# One step must stay below 1e-12 and the loops below 1e-9 whatever was measured: anything larger is not rounding.
POWER_1_SEEN, POWER_1_BOUND = 2.776e-17, 16 * 2.776e-17      # one step on irregular300 (entries about 0.06: two ulps)
POWER_50_SEEN, POWER_50_BOUND = 5.551e-17, 16 * 5.551e-17    # fifty steps
LOOP_X_SEEN, LOOP_X_BOUND = 2.290e-16, 16 * 2.290e-16        # the three loop fixtures (2.290e-16, 2.776e-17, 3.469e-17)
assert POWER_1_BOUND < 1e-12 and LOOP_X_BOUND <= 1e-9
# At 262,182 nodes the bound is not POWER_1_BOUND: a dot product of n terms rounds with n, and the device's sum order is not numpy's.
# It is 16 times what tests/fosr_ref.py's own float64 step differs from the same step in np.longdouble on the test's input (the
# reference against itself, computed in the test), under the same ceiling of 1e-12.  As measured: the reference against itself,
# and the device against the reference on an MI355X.
POWER_LARGE_REF_SEEN = {1: 1.685e-18, 5: 7.534e-18}     # bounds 2.696e-17 and 1.205e-16 (entries about 0.002: a few ulps)
POWER_LARGE_SEEN = {1: 1.735e-18, 5: 5.204e-18}


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def check_pick(G, ei, n, x, label, brute=True, fast=None):
    """The three conditions of a pick; returns it.  fast: the graph's CSR adjacency; the rule is then taken from
    ref.row_products_fast (equal to ref.row_products: tests/test_fosr_cpu.py) and no neighbour sets are built."""
    if fast is not None:
        deg, rows = np.diff(fast.indptr).astype(np.int64), None
    else:
        _, deg, rows = ref.degrees_and_rows(ei, n)
    got, y = G.fosr_pick(x, return_y=True)
    want_y = np.asarray(x, dtype=np.float64) / np.sqrt(deg + 1.0)
    assert (np.abs(y - want_y) <= 2 * np.spacing(np.abs(want_y))).all(), label
    want = ref.pick_of(*ref.row_products_fast(y, fast)) if fast is not None else ref.pick(y, rows)
    if want is None:
        assert got is None, (label, got)
    else:
        assert got is not None and got[:2] == want[:2] and same_bits(got[2], want[2]), (label, got, want)
        if brute and n <= 3000 and rows is not None:
            assert got[2] == ref.brute_minimum(y, rows), label
    return got


# ---- 1. the pick -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 3, 9, 33, 64, 65, 130, 300])
def test_pick_random_graphs(dcr, n):
    rng = np.random.Generator(np.random.PCG64(100 + n))
    for p in (0.05, 0.5, 0.9):
        ei, _ = ref.random_graph(n, p, rng)
        G = dcr(ei, n)
        for name, x in ref.vector_kinds(n, rng).items():
            check_pick(G, ei, n, x, (n, p, name))


def test_pick_smallest_graphs(dcr):
    rng = np.random.Generator(np.random.PCG64(1))
    empty = np.zeros((2, 0), dtype=np.int64)
    for name, x in ref.vector_kinds(2, rng).items():
        assert check_pick(dcr(spectral_ref.path(2)[0], 2), spectral_ref.path(2)[0], 2, x, name) is None     # its one edge is there
        got = check_pick(dcr(empty, 2), empty, 2, x, name)
        assert got is not None and got[:2] == (0, 1)
    for n in (3, 6, 40):
        ei, _ = spectral_ref.complete(n)
        for name, x in ref.vector_kinds(n, rng).items():
            assert check_pick(dcr(ei, n), ei, n, x, (n, name)) is None
    ei, n = spectral_ref.star(7)      # the centre is adjacent to everyone: no candidate from that row, whatever its y
    G = dcr(ei, n)
    for name, x in ref.vector_kinds(n, rng).items():
        got = check_pick(G, ei, n, x, name)
        assert got is not None and 0 not in got[:2]
    x = np.array([-9.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0])    # the centre's products would all be the smallest
    assert check_pick(G, ei, n, x, 'centre')[:2] == (1, 2)


def test_pick_at_the_class_limits(dcr):
    """Rows of degree 3, 32, 33, 2,048 and 2,049 in one graph; for each, the vector that fills the lowest d + 1 ranks with the row
    and its neighbours (the first free rank is the bitmap's last bit), the same from the top with y_u < 0, and one with rank 0 free."""
    ei, n = spectral_ref.row_classes_graph()
    _, deg, rows = ref.degrees_and_rows(ei, n)
    G = dcr(ei, n)
    targets = {3: 4 + 32, 32: 0, 33: 1, 2048: 2, 2049: 3}
    for d, u in targets.items():
        assert deg[u] == d
        for where in ('bottom', 'top', 'free0'):
            x = ref.packed_vector(deg, u, {u} | rows[u], where)
            y = ref.y_of(x, deg)
            _, partner = ref.row_products(y, rows)
            rank_of_partner = int(np.flatnonzero(ref.order_of(y) == partner[u])[0])
            assert rank_of_partner == {'bottom': d + 1, 'top': n - 1 - (d + 1), 'free0': 0}[where], (d, where)
            got = check_pick(G, ei, n, x, (d, where), brute=True)
            assert got[:2] == (u, int(partner[u])), (d, where, got)      # row u's own answer decided the pick


@pytest.mark.parametrize('name', spectral_ref.PLAN_NAMES)
def test_pick_on_the_plan_family(dcr, name):
    ei, n = next((e, m) for nm, e, m in spectral_ref.plan_family() if nm == name)
    x = np.random.Generator(np.random.PCG64(len(name))).standard_normal(n)
    check_pick(dcr(ei, n), ei, n, x, name)


def test_pick_in_the_second_window(dcr):
    """A hub of more neighbours than one LDS window has ranks, all of them below every other node: the first free rank lies in
    the second window (and, mirrored, from the top)."""
    from dcr.graph import FOSR_WINDOW
    d, n = FOSR_WINDOW + 500, FOSR_WINDOW + 3000
    pairs = [(0, 1 + i) for i in range(d)] + [(i, i + 1) for i in range(1, n - 1)]
    ei, _ = spectral_ref._und(pairs, n)
    _, deg, rows = ref.degrees_and_rows(ei, n)
    G = dcr(ei, n)
    for where in ('bottom', 'top'):
        x = ref.packed_vector(deg, 0, {0} | rows[0], where)
        y = ref.y_of(x, deg)
        _, partner = ref.row_products(y, rows)
        rank = int(np.flatnonzero(ref.order_of(y) == partner[0])[0])
        assert (rank if where == 'bottom' else n - 1 - rank) == d + 1 > FOSR_WINDOW
        assert check_pick(G, ei, n, x, where)[:2] == (0, int(partner[0]))        # the hub's row decided
    check_pick(G, ei, n, np.random.Generator(np.random.PCG64(3)).standard_normal(n), 'random')


_SCALE = {}


def scale_case(which):
    """(edge_index, n, CSR adjacency, degrees, the plan's row list) of the two large graphs, built once."""
    if which not in _SCALE:
        ei, n = scale_ref.whole_small() if which == 'small' else scale_ref.fosr_large()
        a = spectral_ref.adjacency(ei, n)
        deg = np.diff(a.indptr).astype(np.int64)
        long_, short = deg > spectral_ref.LONG_DEG, deg <= spectral_ref.SHORT_DEG
        rows = np.concatenate([np.flatnonzero(long_), np.flatnonzero(~long_ & ~short), np.flatnonzero(short)])
        _SCALE[which] = (ei, n, a, deg, rows)
    return _SCALE[which]


def placed_vector(deg, u, w, rng):
    """x whose pick is decided by the rows of u and w alone: y_u = -10, y_w = 10 and |y| < 1 elsewhere, so y_u y_w = -100 is the
    smallest product by far and only u (from the top of the order) and w (from the bottom) find it; every other row's best is
    y_v y_u > -10.  The rule names the smaller of the two as u."""
    y = np.tanh(rng.standard_normal(deg.shape[0])) * 0.99
    y[u], y[w] = -10.0, 10.0
    return y * np.sqrt(deg + 1.0)


@pytest.mark.parametrize('which', ['small', 'large'])
def test_pick_past_256_workgroups(dcr, which):
    """70,001 nodes (all three row classes) and 262,182 nodes: thousands of workgroups, so the closing loop of k_fosr_pick makes
    many trips over the partials, and the order comes from a sort beyond everything tests/test_sweep_gpu.py sorted before this
    size was added.  Bit for bit against the rule on the device's own y."""
    ei, n, a, deg, rows = scale_case(which)
    G = dcr(ei, n)
    rng = np.random.Generator(np.random.PCG64(n))
    kinds = ref.vector_kinds(n, rng)
    for name in ('normal', 'small_integers', 'both_zeros', 'negative'):
        assert check_pick(G, ei, n, kinds[name], (which, name), fast=a) is not None
    # the deciding rows in the last workgroup (the closing loop's last trip must carry them), then in the first
    u, w = int(rows[-2]), int(rows[-1])
    assert a[u, w] == 0 and u < w
    got = check_pick(G, ei, n, placed_vector(deg, u, w, rng), (which, 'last workgroup'), fast=a)
    assert got[:2] == (u, w) and got[2] == -100.0
    u = int(rows[0])
    w = int(next(v for v in rows[::-1] if a[u, v] == 0 and v > u and deg[v] > 0))     # far away in the list: another workgroup
    got = check_pick(G, ei, n, placed_vector(deg, u, w, rng), (which, 'first workgroup'), fast=a)
    assert got[:2] == (u, w) and got[2] == -100.0
    if which == 'large':   # both rows in workgroup 0, all other workgroups worse
        u, w = int(rows[0]), int(next(v for v in rows[2:32] if a[rows[0], v] == 0))
        got = check_pick(G, ei, n, placed_vector(deg, u, w, rng), (which, 'first workgroup alone'), fast=a)
        assert got[:2] == (u, w)


def test_pick_follows_the_edits(dcr):
    ei, n = spectral_ref.path(60)
    G = dcr(ei, n)
    rng = np.random.Generator(np.random.PCG64(4))
    for v in range(2, 45):            # row 0 grows past its capacity: the rows move
        G.add_edge(0, v)
    check_pick(G, G.to_edge_index(), n, rng.standard_normal(n), 'grown')
    G.remove_edge(0, 7)
    G.remove_edge(20, 21)
    now = G.to_edge_index()
    for name, x in ref.vector_kinds(n, rng).items():
        check_pick(G, now, n, x, name)
    assert np.array_equal(G.to_edge_index(), now)     # read-only


def test_pick_arguments(dcr):
    ei, n = spectral_ref.cycle(9)
    G = dcr(ei, n)
    before = G.to_edge_index()
    x = np.arange(9.0)
    x[4] = np.nan
    with pytest.raises(ValueError):
        G.fosr_pick(x)
    with pytest.raises(ValueError):
        G.fosr_pick(np.zeros(8))
    with pytest.raises(ValueError):
        dcr(np.zeros((2, 0), dtype=np.int64), 1).fosr_pick(np.zeros(1))
    with pytest.raises(ValueError):
        G.fosr(-1)
    with pytest.raises(ValueError):
        dcr(np.zeros((2, 0), dtype=np.int64), 5).fosr(1)      # no edges
    assert np.array_equal(G.to_edge_index(), before)


# ---- 2. the power step -------------------------------------------------------------------------------------------------------------
def test_power_step(dcr):
    ei, n = ref.irregular_graph(300, seed=5, isolated=1)
    assert spectral_ref.normalised_adjacency(ei, n)[1].min() == 0
    G = dcr(ei, n)
    x0 = np.random.Generator(np.random.PCG64(6)).standard_normal(n)
    for steps, bound in ((1, POWER_1_BOUND), (50, POWER_50_BOUND)):
        edges, x = G.fosr(0, steps, x0=x0, return_vector=True)
        want = ref.loop(ei, n, 0, steps, x0)[1]
        diff = float(np.abs(x - want).max())
        print(f'power step x{steps}: largest difference {diff:.3e} (bound {bound:.3e})')
        assert edges.shape == (2, 0) and diff <= bound
        assert G.fosr(0, steps, x0=x0, return_vector=True)[1].tobytes() == x.tobytes()      # the same bits again
    assert np.array_equal(G.to_edge_index(), dcr(ei, n).to_edge_index())


@pytest.mark.parametrize('steps', [1, 5])
def test_power_step_past_the_dot_cap(dcr, steps):
    """262,182 nodes: k_fosr_dot takes a second grid-stride trip and closes 1,024 partials, the mat-vec closes 8,194."""
    ei, n, a, deg, _ = scale_case('large')
    x0 = np.random.Generator(np.random.PCG64(26)).standard_normal(n)
    own = ref.own_rounding(a, deg, x0, steps)
    bound = 16 * own
    want = x0
    for _ in range(steps):
        want = ref.power_step(a, deg, want)
    G = dcr(ei, n)
    edges, x = G.fosr(0, steps, x0=x0, return_vector=True)
    diff = float(np.abs(x - want).max())
    print(f'power step x{steps} at n = {n}: the reference against itself {own:.3e}, bound {bound:.3e}, device against the reference {diff:.3e} '
          f'(recorded: {POWER_LARGE_REF_SEEN[steps]}, {POWER_LARGE_SEEN[steps]})')
    assert edges.shape == (2, 0) and 0 < bound < 1e-12
    assert diff <= bound
    assert abs(np.linalg.norm(x) - 1.0) < 1e-12 and abs(np.dot(x, np.sqrt(deg))) < 1e-9    # on the sphere, off the null vector


def test_power_step_that_vanishes_stops_the_loop(dcr):
    ei, n = spectral_ref.cycle(12)
    G = dcr(ei, n)
    edges, x = G.fosr(3, 2, x0=np.zeros(n), return_vector=True)       # |z| = 0 at the first step
    assert edges.shape == (2, 0) and not x.any() and G.number_of_edges() == 12


# ---- 3. the loop -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [f[0] for f in ref.LOOP_FIXTURES])
def test_loop_adds_the_restatements_edges(dcr, name):
    ei, n, x0, iters, (want_edges, _, _) = ref.loop_fixture(name)
    G = dcr(ei, n)
    edges, x = G.fosr(iters, ref.LOOP_INITIAL, x0=x0, return_vector=True)
    assert edges.dtype == np.int64 and np.array_equal(edges, want_edges), name         # every iteration
    want_x = ref.loop(ei, n, iters, ref.LOOP_INITIAL, x0, replay=edges)[1]
    diff = float(np.abs(x - want_x).max())
    print(f'{name}: final iterate differs by {diff:.3e} (bound {LOOP_X_BOUND:.3e})')
    assert diff <= LOOP_X_BOUND
    assert G.number_of_edges() == ei.shape[1] // 2 + iters
    if name == 'two_components600':
        assert spectral_ref.components(ei, n)[0] == 2
        first = dcr(ei, n)
        first.fosr(1, ref.LOOP_INITIAL, x0=x0)
        assert first.connected_components()[0] == 1


def test_loop_at_70001_nodes(dcr):
    """Ten iterations from a given x0 on the 70,001-node graph.  The device's picks are replayed through the restatement (fast row
    products): wherever the rule's runner-up margin on the replayed state is above the power step's bound, the device's pick must
    be the rule's; at most one iteration may fall under it (tests/test_fosr_cpu.py: none does in the restatement's own run)."""
    ei, n, a, deg, _ = scale_case('small')
    x0 = np.random.Generator(np.random.PCG64(ref.LOOP_LARGE_SEED)).standard_normal(n)
    bound = 16 * ref.own_rounding(a, deg, x0, 1)
    assert 0 < bound < 1e-12
    G = dcr(ei, n)
    edges, x = G.fosr(ref.LOOP_LARGE_ITERS, ref.LOOP_INITIAL, x0=x0, return_vector=True)
    assert edges.shape == (2, ref.LOOP_LARGE_ITERS) and G.number_of_edges() == ei.shape[1] // 2 + ref.LOOP_LARGE_ITERS
    _, want_x, margins, picks = ref.loop_fast(ei, n, ref.LOOP_LARGE_ITERS, ref.LOOP_INITIAL, x0, replay=edges)
    print(f'loop at n = {n}: margins {min(margins):.3e} .. {max(margins):.3e}, bound {bound:.3e}, final iterate differs by '
          f'{float(np.abs(x - want_x).max()):.3e}')
    under = 0
    for it, (margin, want) in enumerate(zip(margins, picks)):
        if margin > bound:
            assert (int(edges[0, it]), int(edges[1, it])) == want[:2], (it, edges[:, it].tolist(), want, margin)
        else:
            under += 1
    assert under <= 1 and len(margins) == ref.LOOP_LARGE_ITERS
    assert float(np.abs(x - want_x).max()) <= 1e-9      # the ceiling of the loops: anything larger is not rounding


def test_loop_bridges_the_bottleneck(dcr):
    ei, n, left, right = ref.two_cliques(20, 4)
    G = dcr(ei, n)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        before = G.spectral_gap().lambda1
        edges = G.fosr(20, 50, seed=1)
        after = G.spectral_gap().lambda1
    assert edges.shape == (2, 20)
    for u, v in edges[:, :5].T:
        assert (int(u) in left) != (int(v) in left), (u, v)
    assert after > before


def test_loop_seed_and_limits(dcr):
    ei, n = ref.irregular_graph(200, seed=1)
    a = dcr(ei, n).fosr(8, 10, seed=7)
    b = dcr(ei, n).fosr(8, 10, seed=7)
    assert a.shape == (2, 8) and np.array_equal(a, b)
    G = dcr(ei, n)
    assert G.fosr(0, 3).shape == (2, 0) and np.array_equal(G.to_edge_index(), dcr(ei, n).to_edge_index())
    K = dcr(spectral_ref.complete(6)[0], 6)
    assert K.fosr(4, 2, x0=np.arange(6.0)).shape == (2, 0) and K.number_of_edges() == 15
    # a graph two edges short of complete: they are added, then nothing is left
    pairs = [(i, j) for i in range(6) for j in range(i + 1, 6) if (i, j) not in ((0, 5), (2, 3))]
    S = dcr(spectral_ref._und(pairs, 6)[0], 6)
    got = S.fosr(5, 2, x0=np.array([1.0, -2.0, 3.0, -4.0, 5.0, -6.0]))
    assert {tuple(sorted(e)) for e in got.T.tolist()} == {(0, 5), (2, 3)} and S.number_of_edges() == 15


def test_rewiring_entry_point_feeds_the_gcn(dcr):
    import torch
    from dcr.data import Data, Dataset
    from models.gcn import GCN
    from rewiring.fosr import fosr
    ei, n, x0, _, (want_edges, _, _) = ref.loop_fixture('irregular200')
    g = torch.Generator(device='cuda').manual_seed(5)
    x = torch.rand(n, 24, device='cuda', generator=g)
    y = torch.randint(0, 4, (n,), device='cuda', generator=g)
    data = Data(x=x, edge_index=torch.from_numpy(ei).cuda(), y=y, num_nodes=n)
    out = fosr(data, 10, initial_power_iters=ref.LOOP_INITIAL, x0=x0)
    added = want_edges[:, :10]
    both = np.stack([added, added[::-1]], axis=2).reshape(2, -1)
    assert out.x is x and out.y is y and out.num_nodes == n and data.edge_index.shape[1] == ei.shape[1]
    assert out.edge_index.is_cuda and out.edge_index.dtype == torch.int64
    assert np.array_equal(out.edge_index.cpu().numpy(), np.concatenate([ei, both], axis=1))
    assert both[:, 0].tolist() == added[:, 0].tolist() and both[:, 1].tolist() == added[::-1, 0].tolist()
    assert out.edge_type.cpu().tolist() == [0] * ei.shape[1] + [1] * 20
    torch.manual_seed(3)
    model = GCN(Dataset(out, 4), hidden=[16], dropout=0.5).cuda()
    model.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(model(out)).all())
    live = dcr(ei, n)
    same = fosr(live, 10, initial_power_iters=ref.LOOP_INITIAL, x0=x0)
    assert np.array_equal(same.edge_index.numpy()[:, -20:], both) and live.number_of_edges() == ei.shape[1] // 2 + 10
    assert same.edge_index.shape[1] == ei.shape[1] + 20 and same.edge_type.sum().item() == 20


def test_handle_stays_usable(dcr):
    ei, n, x0, _, _ = ref.loop_fixture('irregular200')
    G = dcr(ei, n)
    G.curvature_pass('bfc')
    G.fosr(12, ref.LOOP_INITIAL, x0=x0)
    eu, ev, cv = G.curvature_all('bfc')
    fu, fv, fc = dcr(G.to_edge_index(), n).curvature_all('bfc')

    def keyed(u, v, c):
        lo, hi = np.minimum(u, v), np.maximum(u, v)
        order = np.lexsort((hi, lo))
        return lo[order], hi[order], c[order]
    a, b = keyed(eu, ev, cv), keyed(fu, fv, fc)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()
    G.curvature_pass('bfc', incremental=True)
    assert keyed(*G.curvature_read())[2].tobytes() == b[2].tobytes()
