"""The host replica of the Lanczos driver (tests/spectral_lanczos_ref.py) against facts that do not depend on it, so that the
step-by-step comparison on the GPU (tests/test_spectral_steps_gpu.py) is a comparison with something that is itself pinned: the
start vector against the Random123 known answers, the projector, a full-length run against the dense eigenvalue, and, on every
case of the GPU test, the Ritz gap above a stated floor, no breakdown, and the distance between the float64 and the longdouble
run, which the GPU test's allowance rests on (printed: run with -s)."""
from fractions import Fraction

import numpy as np
import pytest

import spectral_lanczos_ref as ref
import spectral_ref

L = np.longdouble
GAP_FLOOR = 2.0 ** -8       # of the two largest Ritz values of the last T_k, on every case
BETA_FLOOR = 2.0 ** -20     # every beta the breakdown test sees: far above SP_BREAKDOWN = 2^-40


# ---- the start vector ---------------------------------------------------------------------------------------------------------------
def value_of_words(r0, r1):
    """((float64)bits + 0.5) * 2^-52 - 1.0 in rational arithmetic, rounded to nearest even where float64 rounds: float() of a
    Fraction rounds correctly."""
    bits = (r0 | (r1 << 32)) >> 11
    t = float(Fraction(bits) + Fraction(1, 2))
    t = float(Fraction(t) * Fraction(1, 2 ** 52))
    return float(Fraction(t) - 1)


# Random123 kat_vectors, philox4x32 10 rounds, as tests/test_dropout_stream_cpu.py has them: (counter words, key words, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def test_start_vector_known_answers():
    """Counter {node lo, node hi, restart lo, restart hi}, key {seed lo, seed hi}: the second and third vectors have a node and a
    seed above 2^32, and the third tells the node from the restart word and the low from the high halves."""
    big = 0
    for (c0, c1, c2, c3), (k0, k1), out in KAT:
        node, restart, seed = c0 | (c1 << 32), c2 | (c3 << 32), k0 | (k1 << 32)
        got = ref.start_values(np.array([node], dtype=np.uint64), seed, restart)
        assert got.dtype == np.float64 and got[0] == value_of_words(out[0], out[1]), (hex(node), hex(seed))
        big += (out[0] | (out[1] << 32)) >> 11 >= 2 ** 52
    assert big >= 2      # bits + 0.5 rounds there
    # the pi vector, literally
    assert value_of_words(0xD16CFE09, 0x94FDCCEB) == float.fromhex('0x1.4fdccebd16d00p-3')
    assert ref.start_values(np.array([0x85A308D3243F6A88], dtype=np.uint64), 0x299F31D0A4093822, 0x0370734413198A2E)[0] == \
        float.fromhex('0x1.4fdccebd16d00p-3')
    # swapped counter arguments, a dropped high word: another value
    assert ref.start_values(np.array([0x0370734413198A2E], dtype=np.uint64), 0x299F31D0A4093822, 0x85A308D3243F6A88)[0] != \
        float.fromhex('0x1.4fdccebd16d00p-3')
    # start_vector is start_values over the node ids, 0 on isolated nodes, restart 0 by default
    deg = np.array([3, 0, 1, 2, 0, 7])
    v = ref.start_vector(deg, 2 ** 40 + 3)
    assert np.array_equal(v, np.where(deg > 0, ref.start_values(np.arange(6), 2 ** 40 + 3, 0), 0.0))
    assert not np.array_equal(v, ref.start_vector(deg, 3)) and not np.array_equal(v, ref.start_vector(deg, 2 ** 40 + 3, 1))


def test_rounding_at_the_top_of_the_range():
    """bits + 0.5 is exact below 2^52 and rounds to even from there on."""
    assert value_of_words(0, 0) == -1.0 + 2.0 ** -53 and value_of_words(0xFFFFF800, 0x7FFFFFFF) == -(2.0 ** -53)
    assert value_of_words(0x00000800, 0x80000000) == 2.0 ** -51      # bits = 2^52 + 1: 2^52 + 1.5 -> 2^52 + 2


@pytest.mark.parametrize('key', sorted({c[0] for c in ref.CASES}))
def test_start_vector_range(key):
    ei, n = ref.graph(key)
    deg = np.bincount(ei[0], minlength=n)
    v = ref.start_vector(deg, ref.SEED)
    assert v.shape == (n,) and (np.abs(v) < 1.0).all()
    assert (v[deg > 0] != 0.0).all() and (v[deg == 0] == 0.0).all()


# ---- the projector ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ['irregular513', 'multi', 'path4_iso2', 'k5_k7_iso', 'long3_mid9_short63'])
def test_project(key):
    ei, n = ref.graph(key)
    R = ref.Replica(ei, n)
    K64 = spectral_ref.null_vectors(ei, n)
    with_edge = [k for k in K64 if np.count_nonzero(k) > 1]
    assert len(with_edge) == len(R.K) and len(K64) == R.components
    for mine, theirs in zip(R.K, with_edge):     # the k_C of spectral_ref, to float64
        assert np.abs(mine - theirs).max() <= 4 * 2.0 ** -53
    bound = 4 * n * 2.0 ** -64
    rng = np.random.Generator(np.random.PCG64(1))
    w = rng.standard_normal(n).astype(L)
    w /= np.sqrt(w @ w)
    p = R.project(w)
    print(f'{key}: |PPw - Pw| = {float(np.abs(R.project(p) - p).max()):.3e}, |K Pw| = {float(np.abs(R.K @ p).max()):.3e}, '
          f'|P k| = {max(float(np.abs(R.project(k)).max()) for k in R.K):.3e}, bound {bound:.3e}')
    assert np.abs(R.project(p) - p).max() <= bound
    assert np.abs(R.K @ p).max() <= bound
    for k in R.K:
        assert np.abs(R.project(k)).max() <= bound
    assert np.array_equal(ref.project((ei, n), w), p)


def test_apply_B_is_two_minus_the_laplacian():
    ei, n = ref.graph('path4_iso2')
    v = np.random.Generator(np.random.PCG64(2)).standard_normal(n)
    v[4:] = 0.0      # the solver's vectors are zero on the isolated nodes, where B is I and 2 - L is 2
    want = 2 * v - spectral_ref.laplacian(ei, n) @ v
    assert np.abs(ref.apply_B((ei, n), v).astype(np.float64) - want).max() <= 8 * 2.0 ** -52
    assert np.abs(ref.apply_B((ei, n), v, np.float64) - want).max() <= 8 * 2.0 ** -52


# ---- a full-length run is the dense eigenvalue ----------------------------------------------------------------------------------------
def small_graphs():
    import fosr_ref
    return [('path3', ref.graph('path3')), ('path4_iso2', ref.graph('path4_iso2')), ('path7', spectral_ref.path(7)),
            ('hypercube3', spectral_ref.hypercube(3)), ('irregular40', fosr_ref.irregular_graph(40, 40)),
            ('two_components60_iso2', fosr_ref.irregular_graph(60, 60, components=2, isolated=2))]


@pytest.mark.parametrize('name', [g[0] for g in small_graphs()])
def test_full_length_run_reaches_the_dense_eigenvalue(name):
    """s = n - components steps span the whole deflated space (or an invariant part of it that holds the start vector: the
    hypercube's, where the replica walks the driver's breakdown branch): the top Ritz value is theta_max."""
    ei, n = dict(small_graphs())[name]
    c, _ = spectral_ref.components(ei, n)
    s = n - c
    lam, res, y, steps, restarts = ref.schedule((ei, n), ref.SEED, s + 1, max_basis=n)
    want = spectral_ref.lambda1(ei, n)
    print(f'{name}: n={n} s={s} steps={steps} restarts={restarts} lambda1={float(lam)!r} dense={want!r} residual={float(res):.3e}')
    assert restarts == 1 and steps <= s + 1
    assert abs(float(lam) - want) <= spectral_ref.bound(float(res), n)
    assert float(res) <= 64 * n * 2.0 ** -52      # and the pair is an eigenpair: nothing of the space is left
    assert abs(float(np.sqrt(y @ y)) - 1) <= 4 * n * 2.0 ** -64


# ---- every case of the GPU test -------------------------------------------------------------------------------------------------------
def test_the_multi_component_graph_is_laid_out_as_planned():
    """Components with an edge of exactly 1024, 1025, 2049 and 2 nodes in the device's order (by smallest node id), three isolated
    nodes, n no multiple of 64; the 1025- and the 2049-node component start at chunks 1 and 3 with 2 and 3 chunks; every
    component's nodes spread over the whole id range."""
    ei, n = ref.graph('multi')
    R = ref.Replica(ei, n)
    assert n == 4103 and n % 64 != 0 and R.components == 7
    assert [int((R.labels == r).sum()) for r in R.roots] == list(ref.MULTI_SIZES)
    chunks, one = R.chunks()
    assert not one and [(c[2], c[3]) for c in chunks] == [(0, 1), (1, 2), (1, 2), (3, 3), (3, 3), (3, 3), (6, 1)]
    assert [c[1] - c[0] for c in chunks] == [1024, 1024, 1, 1024, 1024, 1, 2]
    for r in R.roots[:3]:
        ids = np.flatnonzero(R.labels == r)
        assert ids.min() < 64 and ids.max() > n - 64
    assert int((R.deg == 0).sum()) == 3
    assert -(-n // ref.SP_WAVE_ELEMS) == 9      # three workgroups of k_spec_gs_coef, one live wave in the last


def test_the_one_component_graphs_are_laid_out_as_planned():
    for n, waves in ((511, 1), (512, 1), (513, 2), (1024, 2), (1025, 3), (2049, 5)):
        ei, n_ = ref.graph(f'irregular{n}')
        R = ref.Replica(ei, n_)
        assert n_ == n and R.components == 1 and -(-n // ref.SP_WAVE_ELEMS) == waves
        chunks, one = R.chunks()
        assert one and len(chunks) == -(-n // ref.SP_CHUNK)
    assert chunks[-1][:2] == (2048, 2049)       # the third chunk of the ONE path holds one node
    ei, n = ref.graph('lattice')
    assert n == 33_133 and -(-n // ref.SP_WAVE_ELEMS) == 65
    assert ref.Replica(ei, n).chunks()[1]       # one component with an edge; the isolated nodes are not deflated


@pytest.mark.parametrize('case', ref.CASES, ids=ref.case_id)
def test_case_on_the_replica(case):
    key, ms, mb = case
    r = ref.reference(case)
    lam, res, y, steps, restarts = r['long']
    gap, betas = r['trace']['gap'], r['trace']['betas']
    print(f'{ref.case_id(case)}: n={r["n"]} d_max={r["d_max"]} steps={steps} restarts={restarts} ritz={r["trace"]["ritz"]} '
          f'lambda1={float(lam)!r} residual={float(res):.6e} gap={gap:.3e} min beta={min(betas, default=np.inf):.3e}')
    print(f'    float64 against longdouble: lambda1 {r["dist"][0]:.3e}, residual {r["dist"][1]:.3e}, vector {r["dist"][2]:.3e}; '
          f'counted {r["counted"]:.3e}, for the vector {r["counted_vector"]:.3e}')
    # the two precisions walk the same schedule
    assert (steps, restarts) == r['f64'][3:] and r['trace']['ritz'] == r['trace64']['ritz']
    if key in ref.BREAKS_DOWN:
        # beta_0 is 0 in exact arithmetic: both precisions land far below the threshold, and the driver stops after two steps
        assert max(r['trace']['betas'] + r['trace64']['betas'], default=0.0) <= ref.SP_BREAKDOWN * 2.0 ** -8
        assert (steps, restarts) == ((1, 0) if ms == 1 else (2, 1))
    else:
        assert steps == ms and min(betas + r['trace64']['betas'], default=np.inf) >= BETA_FLOOR
        if mb is None:
            assert restarts == (0 if ms == 1 else 1) and r['trace']['ritz'] == ([] if ms == 1 else [ms - 1])
    assert gap >= GAP_FLOOR and r['trace64']['gap'] >= GAP_FLOOR
    # the returned triple belongs together: unit, deflated, and lambda1 and the residual are the vector's own
    R = ref.operators(key)['long']
    tiny = 64 * r['n'] * 2.0 ** -64
    assert abs(float(np.sqrt(y @ y)) - 1) <= tiny and np.abs(R.K @ y).max() <= tiny
    by = R.apply_B(y)
    assert abs(float(2 - y @ by - lam)) <= tiny
    t = R.project(by) - (y @ by) * y
    assert abs(float(np.sqrt(t @ t) - res)) <= 2 * (2 + r['basis']) * tiny
    assert (y[R.deg == 0] == 0).all()


def test_chained_restarts_on_the_replica():
    """max_basis = 4, max_steps = 11: cycles of 4, 4 and 2 steps and the closing step; max_basis = 16, max_steps = 41: 16, 16, 8."""
    a, b = ref.reference(('irregular513', 11, 4)), ref.reference(('irregular513', 41, 16))
    assert a['long'][3:] == (11, 3) and a['trace']['ritz'] == [4, 4, 2]
    assert b['long'][3:] == (41, 3) and b['trace']['ritz'] == [16, 16, 8]
    c, d = ref.reference(('path3', 3, None)), ref.reference(('path4_iso2', 4, None))
    assert c['long'][3:] == (3, 1) and c['trace']['ritz'] == [2] and ref.basis_columns(3, 1) == 2
    assert d['long'][3:] == (4, 1) and d['trace']['ritz'] == [3] and ref.basis_columns(6, 3) == 3


def test_largest_distances():
    """The largest float64-against-longdouble distance per quantity over the cases, which the GPU test's docstring records."""
    refs = [ref.reference(c) for c in ref.CASES]
    worst = [max(r['dist'][i] for r in refs) for i in range(3)]
    print(f'largest float64-against-longdouble distances: lambda1 {worst[0]:.3e}, residual {worst[1]:.3e}, vector {worst[2]:.3e}')
    print(f'smallest Ritz gap: {min(r["trace"]["gap"] for r in refs):.3e}')
    for r, c in zip(refs, ref.CASES):
        # the counted bound is the allowance everywhere: were a measured distance above it, the first-order count would be missing
        # an amplification, and the docstring of ref.counted says which
        assert r['dist'][0] <= r['counted'] and r['dist'][1] <= r['counted'] and r['dist'][2] <= r['counted_vector'], c
