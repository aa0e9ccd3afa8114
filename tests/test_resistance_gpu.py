"""Effective resistance on the GPU (csrc/dcr_resistance.hip) against closed forms and the dense restatement tests/resistance_ref.py
(pinned on the CPU by tests/test_resistance_cpu.py).

The one acceptance rule, used throughout:   lower - allow <= R_ref <= lower + residual^2 / lambda1_ref + allow
with R_ref and lambda1_ref from the dense restatement and allow = 64 n 2^-52 max(1, R_ref) for rounding (6.3e-13 on the 44-node
barbell, where the numpy CG deviates from pinv by 9e-14).  The left side holds for ANY iterate (R - lower is a squared energy
norm), the right side is |r|^2 / lambda_1 with the TRUE residual the call reports.  No test loops around a failing step."""
import ctypes
import time
import warnings

import numpy as np
import pytest

import resistance_ref as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


@pytest.fixture(scope='module')
def barbell():
    ei, n = ref.barbell(20, 4)
    return ei, n, ref.Dense(ei, n)


def solve(G, pairs, **kw):
    """effective_resistance that must converge: (lower, info)."""
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        lower, info = G.effective_resistance(pairs, return_info=True, **kw)
    assert lower.dtype == np.float64 and info['residual'].dtype == np.float64 and info['steps'].dtype == np.int32
    assert info['converged'].all()
    return lower, info


def accept(lower, residual, r_ref, lam, n, label):
    a = ref.allow(n, r_ref)
    below, above = lower - r_ref, r_ref - (lower + residual ** 2 / lam)
    print(f'  {label}: {len(lower)} pairs, max(lower - R) = {below.max():.3e}, max(R - upper) = {above.max():.3e}, '
          f'allow >= {a.min():.3e}, max residual {residual.max():.3e}')
    assert np.all(below <= a), (label, 'above the reference', np.flatnonzero(below > a)[:5])
    assert np.all(above <= a), (label, 'the upper side fails', np.flatnonzero(above > a)[:5])


def all_pairs(n):
    return np.array([(i, j) for i in range(n) for j in range(n) if i != j])


# ---- 1. closed forms -------------------------------------------------------------------------------------------------------------
def closed_form_cases():
    def star_r(pr):
        return np.where((pr[:, 0] == 0) | (pr[:, 1] == 0), 1.0, 2.0)
    return {
        'path8': (ref.path(8), lambda pr: np.abs(pr[:, 0] - pr[:, 1]).astype(float)),
        'cycle7': (ref.cycle(7), lambda pr: np.abs(pr[:, 0] - pr[:, 1]) * (7 - np.abs(pr[:, 0] - pr[:, 1])) / 7),
        'complete5': (ref.complete(5), lambda pr: np.full(len(pr), 2 / 5)),
        'star6': (ref.star(6), star_r),
        'complete40': (ref.complete(40), lambda pr: np.full(len(pr), 2 / 40)),   # every row in the wave class
    }


@pytest.mark.parametrize('name', ['path8', 'cycle7', 'complete5', 'star6', 'complete40'])
def test_closed_forms_all_pairs(dcr, name):
    (ei, n), form = closed_form_cases()[name]
    d = ref.Dense(ei, n)
    pr = all_pairs(n)
    lower, info = solve(dcr(ei, n), pr)
    accept(lower, info['residual'], form(pr), d.lambda1, n, name + ' (closed form)')
    accept(lower, info['residual'], d.resistance(pr), d.lambda1, n, name + ' (pinv)')
    print('  steps', info['steps'].min(), '..', info['steps'].max())
    if name == 'complete5':
        assert info['steps'].max() <= 2


def barbell_pairs(n=44):
    cross = [(i, 43 - (3 * i) % 20) for i in range(20)]
    return cross


def test_barbell_edges_and_cross_pairs(dcr, barbell):
    ei, n, d = barbell
    e = ref.edges(ei)
    assert len(e) == 385
    pr = np.concatenate([e, barbell_pairs()])
    lower, info = solve(dcr(ei, n), pr)
    accept(lower, info['residual'], d.resistance(pr), d.lambda1, n, 'barbell(20, 4)')
    print('  steps', info['steps'].min(), '..', info['steps'].max())


# ---- 2. Foster and the curvature ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['triangle_star_isolated', 'random300'])
def test_foster_and_curvature(dcr, name):
    from experiment.effective_resistance import edge_resistances, resistance_curvature
    ei, n = ref.triangle_star_isolated() if name == 'triangle_star_isolated' else ref.random_graph()
    c = 3 if name == 'triangle_star_isolated' else 1
    G = dcr(ei, n)
    assert G.connected_components()[0] == c
    eu, ev, R = edge_resistances(G)
    E = len(R)
    geu, gev = G.edges()
    assert E == G.number_of_edges() and np.array_equal(eu, geu) and np.array_equal(ev, gev)
    bound = E * ref.allow(n, 1.0)
    print(f'  {name}: sum R - (n - c) = {R.sum() - (n - c):.3e}, bound {bound:.3e}')
    assert abs(R.sum() - (n - c)) <= bound
    p, eu2, ev2, kappa = resistance_curvature(G)
    assert np.array_equal(eu2, eu) and np.array_equal(ev2, ev) and p.shape == (n,) and kappa.shape == (E,)
    print(f'  sum p - c = {p.sum() - c:.3e}')
    assert abs(p.sum() - c) <= bound
    if name == 'triangle_star_isolated':
        assert p[8] == 1.0
    d = ref.Dense(ei, n)
    want_p, want_e, want_k = d.curvature()
    order = np.lexsort((np.maximum(eu, ev), np.minimum(eu, ev)))   # the restatement's edges are sorted (a, b), a < b
    assert np.array_equal(np.stack([np.minimum(eu, ev), np.maximum(eu, ev)], axis=1)[order], want_e)
    assert np.allclose(p, want_p, rtol=0, atol=1e-9) and np.allclose(kappa[order], want_k, rtol=0, atol=1e-8)


# ---- 3. cases decided on the host ----------------------------------------------------------------------------------------------------
def test_host_decided_cases_mixed_with_solves(dcr):
    ei, n = ref.triangle_star_isolated()
    G = dcr(ei, n)
    d = ref.Dense(ei, n)
    pr = np.array([(0, 1), (2, 2), (0, 3), (4, 5), (4, 8), (8, 8), (1, 2), (3, 7), (8, 0), (5, 5), (7, 2)])
    lower, info = solve(G, pr)
    same, across = [1, 5, 9], [2, 4, 8, 10]
    assert np.all(lower[same] == 0.0) and not np.signbit(lower[same]).any()
    assert np.all(np.isposinf(lower[across]))
    for k in same + across:
        assert info['residual'][k] == 0.0 and info['steps'][k] == 0 and info['converged'][k]
    solvable = [0, 3, 6, 7]
    accept(lower[solvable], info['residual'][solvable], d.resistance(pr[solvable]), d.lambda1, n, 'mixed call')
    for k in solvable:   # the same bits as alone
        l1, i1 = solve(G, pr[k:k + 1])
        assert l1[0].hex() == lower[k].hex() and i1['residual'][0].hex() == info['residual'][k].hex()
        assert i1['steps'][0] == info['steps'][k]


# ---- 4. batch independence and determinism ---------------------------------------------------------------------------------------
def test_batch_independence_and_determinism(dcr, barbell):
    from dcr.graph import RESISTANCE_BATCH as B
    ei, n, d = barbell
    G = dcr(ei, n)
    target = (3, 30)
    others = [tuple(x) for x in ref.edges(ei)[::7]] + barbell_pairs()
    others = [x for x in others if x != target]
    assert len(others) >= 2 * B
    l0, i0 = solve(G, [target])
    want = (l0[0].hex(), i0['residual'][0].hex(), int(i0['steps'][0]))
    print('  alone:', l0[0], i0['residual'][0], i0['steps'][0])
    assert want[2] >= 3   # a cross pair of the barbell is not done in a step or two: the others freeze at other times
    for P in (B + 3, 2 * B):
        for pos in (0, P // 2, P - 1):
            pr = others[:P - 1]
            pr.insert(pos, target)
            for order in (pr, pr[::-1]):
                at = order.index(target)
                lower, info = solve(G, order)
                got = (lower[at].hex(), info['residual'][at].hex(), int(info['steps'][at]))
                assert got == want, (P, pos, at, got, want)
    pr = np.array(others[:2 * B - 3] + [target])
    a, ia = solve(G, pr)
    b, ib = solve(G, pr)
    assert a.tobytes() == b.tobytes() and ia['residual'].tobytes() == ib['residual'].tobytes()
    assert np.array_equal(ia['steps'], ib['steps'])


# ---- 5. the workgroup-per-row class -------------------------------------------------------------------------------------------------
def test_hub_row_takes_a_workgroup(dcr):
    leaves = 2100
    ei, n = ref.hub_with_tail(leaves)
    G = dcr(ei, n)
    assert G.degree(0) == leaves > 2048
    d = ref.Dense(ei, n)   # lambda_1 only: the resistances of a tree are path lengths
    pr = np.array([(2, 3), (17, 2100), (0, 5), (0, 2100), (9, n - 1), (1, n - 1), (0, n - 1), (1, 2)])
    want = np.array([2.0, 2.0, 1.0, 1.0, 5.0, 3.0, 4.0, 2.0])
    lower, info = solve(G, pr)
    accept(lower, info['residual'], want, d.lambda1, n, 'star of 2,100 leaves with a tail')
    print('  steps', info['steps'])


# ---- 6. live graph ------------------------------------------------------------------------------------------------------------------
def check_live(G, pairs, label):
    ei, n = G.to_edge_index(), G.number_of_nodes()
    d = ref.Dense(ei, n)
    lower, info = solve(G, pairs)
    want = d.resistance(pairs)
    fin = np.isfinite(want)
    assert np.array_equal(np.isposinf(lower), ~fin), label
    if fin.any():
        accept(lower[fin], info['residual'][fin], want[fin], d.lambda1, n, label)
    return lower, want


def test_live_graph_edits(dcr):
    G = dcr(*ref.path(4))
    lower, want = check_live(G, [(0, 3)], 'path 0-1-2-3')
    assert want[0] == pytest.approx(3.0, abs=1e-12)
    G.add_edge(0, 3)
    lower, want = check_live(G, [(0, 3), (0, 2)], 'cycle after add_edge(0, 3)')
    assert want.tolist() == pytest.approx([0.75, 1.0], abs=1e-12)
    G.remove_edge(1, 2)
    lower, want = check_live(G, [(1, 2), (0, 3), (1, 3)], 'path 1-0-3-2 after remove_edge(1, 2)')
    assert want.tolist() == pytest.approx([3.0, 1.0, 2.0], abs=1e-12)
    H = dcr(*ref._und([(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (4, 5), (3, 5)], 6))
    check_live(H, [(0, 5), (2, 3)], 'two triangles and a bridge')
    H.remove_edge(2, 3)
    lower, want = check_live(H, [(0, 5), (2, 3), (0, 1), (4, 5)], 'bridge removed')
    assert np.isposinf(lower[:2]).all() and np.isfinite(lower[2:]).all()


def test_live_graph_after_sdrf_at_coras_shape():
    import torch
    from dcr import synthetic
    from dcr.data import Data
    from rewiring.sdrf_no_cuda import SdrfRun
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    np.random.seed(0)
    run = SdrfRun(Data(edge_index=torch.from_numpy(ei), num_nodes=n), 'bfc', True, 0.5, 50)
    for i in range(50):
        assert run.step(more=i + 1 < 50)
    assert not np.array_equal(run.G.to_edge_index(), ei)
    pairs = np.random.default_rng(11).integers(0, n, size=(32, 2))
    check_live(run.G, pairs, 'after 50 SDRF iterations')


# ---- 7. cut short ---------------------------------------------------------------------------------------------------------------------
def test_cut_short_is_still_a_lower_bound(dcr, barbell):
    ei, n, d = barbell
    pr = np.array(barbell_pairs())
    with pytest.warns(RuntimeWarning):
        lower, info = dcr(ei, n).effective_resistance(pr, max_steps=2, return_info=True)
    want = d.resistance(pr)
    assert not info['converged'].any() and np.all(info['steps'] == 2)
    a = ref.allow(n, want)
    print('  after 2 steps: lower / R in', (lower / want).min(), '..', (lower / want).max(), ' residual', info['residual'].min(), '..',
          info['residual'].max())
    assert np.all(lower <= want + a)
    assert np.all(want <= lower + info['residual'] ** 2 / d.lambda1 + a)


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_and_empty(dcr):
    from dcr import _lib
    ei, n = ref.path(4)
    G = dcr(ei, n)
    with pytest.raises(ValueError):
        G.effective_resistance([(0, n)])
    with pytest.raises(ValueError):
        G.effective_resistance([(-1, 2)])
    with pytest.raises(ValueError):
        G.effective_resistance([(0, 1)], tol=-1.0)
    with pytest.raises(ValueError):
        G.effective_resistance([(0, 1)], tol=float('nan'))
    with pytest.raises(ValueError):
        G.effective_resistance([(0, 1)], max_steps=0)
    out = G.effective_resistance([])
    assert out.shape == (0,) and out.dtype == np.float64
    out, info = G.effective_resistance(np.zeros((0, 2), dtype=np.int64), return_info=True)
    assert out.shape == (0,) and info['steps'].shape == (0,) and info['converged'].shape == (0,)
    L = _lib.lib()
    u = (ctypes.c_int32 * 1)(0)
    v = (ctypes.c_int32 * 1)(3)
    lo, re = (ctypes.c_double * 1)(-7.0), (ctypes.c_double * 1)(-7.0)
    assert L.dcr_effective_resistance(None, u, v, 1, None, lo, re, None) == -1
    assert L.dcr_effective_resistance(G._h, None, v, 1, None, lo, re, None) == -1
    assert L.dcr_effective_resistance(G._h, u, None, 1, None, lo, re, None) == -1
    assert L.dcr_effective_resistance(G._h, u, v, 1, None, None, re, None) == -1
    assert L.dcr_effective_resistance(G._h, u, v, 1, None, lo, None, None) == -1
    assert L.dcr_effective_resistance(G._h, u, v, -1, None, lo, re, None) == -1
    assert L.dcr_effective_resistance(G._h, u, v, 0, None, lo, re, None) == 0 and lo[0] == -7.0 and re[0] == -7.0
    assert L.dcr_effective_resistance(G._h, u, v, 1, None, lo, re, None) == 0   # NULL options are the defaults, steps may be NULL
    assert abs(lo[0] - 3.0) <= 1e-12 and 0.0 <= re[0] <= TOL
    E = dcr(np.zeros((2, 0), dtype=np.int64), 5)
    lower, info = solve(E, [(0, 1), (3, 2), (4, 4)])
    assert np.isposinf(lower[:2]).all() and lower[2] == 0.0 and np.all(info['steps'] == 0)


# ---- 9. scale, one batch --------------------------------------------------------------------------------------------------------------
def test_scale_s100k_one_batch(dcr):
    from dcr import synthetic
    from dcr.graph import RESISTANCE_BATCH as B
    scale = load_golden('cheeger_bounds_reference.json')['scale']
    ei, n = synthetic.powerlaw_graph(*scale['generator']['powerlaw_graph'][:2], seed=scale['generator']['powerlaw_graph'][2])
    G = dcr(ei, n)
    rng = np.random.default_rng(9)
    pairs = np.stack([rng.permutation(n)[:B], rng.permutation(n)[:B]], axis=1)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    solve(G, pairs[:1])   # buffers and code objects
    t0 = time.perf_counter()
    lower, info = solve(G, pairs)
    dt = time.perf_counter() - t0
    lam = G.spectral_gap().lambda1
    deg = np.bincount(ei[0], minlength=n).astype(float)
    inv = 1 / deg[pairs[:, 0]] + 1 / deg[pairs[:, 1]]
    a = ref.allow(n, lower)
    print(f'  S100k, {len(pairs)} pairs: steps {info["steps"].min()} .. {info["steps"].max()}, {dt * 1e3:.1f} ms, '
          f'{dt * 1e6 / info["steps"].max():.1f} us per step, max residual {info["residual"].max():.3e}, lambda1 {lam}')
    print('  lower / (inv / 2) in', (lower / (0.5 * inv)).min(), '..', (lower / (0.5 * inv)).max())
    assert np.all(0.5 * inv - a <= lower)          # Lovász: 1/2 (1/d_u + 1/d_v) <= R, and R - lower <= residual^2 / lambda_1 ~ 1e-20
    assert np.all(lower <= inv / lam + a)          # a sanity check, not a certificate: a Lanczos lambda_1 is never below the true one


# ---- 10. past the cap of the element-wise kernels --------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def past_cap(dcr):
    """scale_ref.diffusion_large(), 33,133 nodes: n COL_CP elements are more than 256 COL_UPDATE_BLOCKS, so k_col_start, update,
    direction and scale take a second, ragged grid-stride trip (the lattice's last 356 nodes, every hub, the isolated nodes)
    and k_col_update closes a full 1,024 partials, 32 a thread group (tests/test_scale_thresholds_cpu.py).  The reference is
    resistance_ref.sparse_resistance, measured against itself by a second grounding (e_ref), and lam_lo is a certified lower
    bound of lambda_1 (tests/test_resistance_cpu.py pins both on the CPU); neither comes from the device.  One 19-pair call,
    shared by the tests below: 17 pairs take a column (the second batch has 15 padding columns), two are decided on the host."""
    import scale_ref as sc
    ei, n, names = sc.diffusion_large()
    pairs, solved, _ = sc.resistance_pairs()
    t0 = time.perf_counter()
    r_ref = ref.sparse_resistance(ei, n, pairs)
    e_ref = float(np.abs(r_ref[solved] - ref.sparse_resistance(ei, n, pairs, ground='largest')[solved]).max())
    lam_lo, theta, ritz = ref.lambda1_lower(ei, n, 0)
    t1 = time.perf_counter()
    G = dcr(ei, n)
    with warnings.catch_warnings():   # (the first test asserts that every pair converged: a fixture that raises is an error, not a failure)
        warnings.simplefilter('ignore', RuntimeWarning)
        G.effective_resistance(pairs[:1])   # buffers and code objects
        t2 = time.perf_counter()
        lower, info = G.effective_resistance(pairs, return_info=True)
        t3 = time.perf_counter()
    print(f'  n = {n}: host reference {t1 - t0:.2f} s, e_ref = {e_ref:.3e}, lambda_1 >= {lam_lo:.6e} (Ritz residual {ritz:.3e}); '
          f'the 19-pair call {1e3 * (t3 - t2):.1f} ms')
    for a in (r_ref, lower, info['residual'], info['steps']):
        a.setflags(write=False)
    return dict(G=G, n=n, pairs=pairs, solved=solved, r_ref=r_ref, e_ref=e_ref, lam_lo=lam_lo, lower=lower, info=info)


def test_past_the_cap_against_the_sparse_reference(past_cap):
    """Per solved pair, with a = allow(n, R_ref) + e_ref:  lower <= R_ref + a  and  R_ref - lower <= residual^2 / lam_lo + a."""
    p = past_cap
    n, pairs, solved, lower, info = p['n'], p['pairs'], p['solved'], p['lower'], p['info']
    host = np.setdiff1d(np.arange(len(pairs)), solved)
    assert np.isposinf(lower[5]) and lower[6] == 0.0 and not np.signbit(lower[6])
    assert np.all(info['steps'][host] == 0) and np.all(info['residual'][host] == 0.0)
    r_ref, res, steps = p['r_ref'][solved], info['residual'][solved], info['steps'][solved]
    a = ref.allow(n, r_ref) + p['e_ref']
    gap = r_ref - lower[solved]
    print(f'  steps {steps.min()} .. {steps.max()}, residual {res.min():.3e} .. {res.max():.3e}, R_ref - lower in {gap.min():.3e} .. {gap.max():.3e}, '
          f'residual^2 / lam_lo <= {(res ** 2 / p["lam_lo"]).max():.3e}, a >= {a.min():.3e}')
    assert np.all(np.isfinite(res)) and np.all(np.isfinite(lower[solved]))
    assert info['converged'].all(), ('not converged', np.flatnonzero(~info['converged']))
    assert np.all(steps > 0) and np.all(steps < 20000)
    assert np.all(lower[solved] <= r_ref + a), ('above the reference', np.flatnonzero(lower[solved] > r_ref + a))
    assert np.all(gap <= res ** 2 / p['lam_lo'] + a), ('the bound of the header comment fails', np.flatnonzero(gap > res ** 2 / p['lam_lo'] + a))


def test_past_the_cap_a_column_depends_on_its_own_pair_only(past_cap):
    from dcr.graph import RESISTANCE_BATCH as B
    p = past_cap
    G, pairs, solved = p['G'], p['pairs'], p['solved']
    at = 2                                                                          # (33,000, 33,100): both nodes in the second trip
    others = pairs[solved[solved != at]][:B - 1]
    t0 = time.perf_counter()
    calls = {'alone': (pairs[at:at + 1], 0), 'column 0': (np.concatenate([pairs[at:at + 1], others]), 0),
             f'column {B - 1}': (np.concatenate([others, pairs[at:at + 1]]), B - 1)}
    want = (p['lower'][at:at + 1].tobytes(), p['info']['residual'][at:at + 1].tobytes(), p['info']['steps'][at:at + 1].tobytes())
    for label, (pr, k) in calls.items():
        assert len(pr) in (1, B)
        lower, info = solve(G, pr)
        got = (lower[k:k + 1].tobytes(), info['residual'][k:k + 1].tobytes(), info['steps'][k:k + 1].tobytes())
        assert got == want, (label, lower[k], p['lower'][at], info['steps'][k], p['info']['steps'][at])
    print(f'  three calls {1e3 * (time.perf_counter() - t0):.1f} ms')


def test_past_the_cap_two_calls_give_the_same_bytes(past_cap):
    p = past_cap
    t0 = time.perf_counter()
    lower, info = solve(p['G'], p['pairs'])
    print(f'  the 19-pair call again {1e3 * (time.perf_counter() - t0):.1f} ms')
    assert lower.tobytes() == p['lower'].tobytes() and info['residual'].tobytes() == p['info']['residual'].tobytes()
    assert info['steps'].tobytes() == p['info']['steps'].tobytes()
