"""The inputs of tests/test_bfc_dense_gpu.py, checked without a GPU: the restatement of csrc/dcr_bfc_dense.hip in
tests/bfc_dense_ref.py equals oracle/bfc_cuda_oracle.py (pinned to the reference's own kernels) bit for bit on every family
graph, both equal the values recorded from the reference's kernels above 64 nodes (tests/golden/bfc_cuda_curvature_wide.json),
the closed forms hold, and — the point of the families — a kernel that loses the tail of its 64-wide stride loop would
change at least one value on every graph.  Everything is compared as uint32 bit patterns."""
import functools
import time

import numpy as np
import pytest

import bfc_dense_ref as bd
from conftest import load_golden
from oracle import bfc_cuda_oracle as bo

FAMILY = bd.family_graphs()
NAMES = [g[0] for g in FAMILY]
BY_NAME = {g[0]: g for g in FAMILY}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u32hex(a):
    return [f'{int(v):08x}' for v in bits(a).ravel()]


@functools.lru_cache(maxsize=None)
def oracle_curvature(name):
    t0 = time.perf_counter()
    C = bo.balanced_forman_curvature(BY_NAME[name][1])
    C.setflags(write=False)
    return C, time.perf_counter() - t0


def queries_of(name):
    _, A, _, directed = BY_NAME[name]
    return [(x, y) + bd.neighbour_lists(A, x, y, directed) for x, y in bd.base_queries(A, oracle_curvature(name)[0], directed)]


def all_queries(name):
    """The post-delta queries of the GPU test: the three above, and for a directed graph an edge with a candidate j == x
    and one with a candidate i == y."""
    _, A, _, directed = BY_NAME[name]
    extra = [(x, y) + bd.neighbour_lists(A, x, y, directed) for x, y in bd.directed_queries(A)] if directed else []
    return queries_of(name) + extra


@pytest.mark.parametrize('name', NAMES)
def test_restatement_equals_the_oracle(name):
    _, A, _, _ = BY_NAME[name]
    want, secs = oracle_curvature(name)
    print(f'{name}: nnz {np.count_nonzero(A)}, oracle curvature {secs:.2f} s')
    assert np.array_equal(bits(bd.curvature(A)), bits(want))
    for x, y, i_nb, j_nb in queries_of(name):
        t0 = time.perf_counter()
        wantD = bo.balanced_forman_post_delta(A, x, y, i_nb, j_nb)
        print(f'{name}: post-delta ({x}, {y}) {len(i_nb)} x {len(j_nb)}, oracle {time.perf_counter() - t0:.2f} s')
        assert np.array_equal(bits(bd.post_delta(A, x, y, i_nb, j_nb)), bits(wantD)), (x, y)


def wide_case_matrix(case):
    N = case['num_nodes']
    A = np.zeros((N, N), dtype=np.float32)
    A[case['pairs'][0], case['pairs'][1]] = np.asarray(case['weights'], dtype=np.float32)
    return A


def test_recorded_wide_fixture_equals_oracle_and_restatement():
    """tests/golden/bfc_cuda_curvature_wide.json: the reference's two kernels evaluated on hub_last / directed_tail graphs of
    65 to 257 nodes (tools/make_golden_cuda_compat.py), values at the non-zero pairs only, float32 bit patterns as hex."""
    fix = load_golden('bfc_cuda_curvature_wide.json')
    assert [(c['family'], c['num_nodes']) for c in fix['cases']] == [('hub_last', 65), ('hub_last', 130), ('hub_last', 257),
                                                                    ('directed_tail', 70), ('directed_tail', 130)]
    for c in fix['cases']:
        A = wide_case_matrix(c)
        N = c['num_nodes']
        built = bd.hub_last(N, c['seed']) if c['family'] == 'hub_last' else bd.directed_tail(N, c['seed'])[0]
        assert np.array_equal(A, built), 'the seeded family no longer builds the recorded graph'
        nz = np.nonzero(A)
        assert [list(map(int, nz[0])), list(map(int, nz[1]))] == c['pairs']
        for C in (bo.balanced_forman_curvature(A), bd.curvature(A)):
            assert u32hex(C[nz]) == c['C'], (c['family'], N)
            assert np.count_nonzero(C) <= len(c['C']) and not C[A == 0].any()
        assert len(c['post_delta']) == 3 and any(N - 1 in (pd['x'], pd['y']) for pd in c['post_delta'])
        for pd in c['post_delta']:
            for f in (bo.balanced_forman_post_delta, bd.post_delta):
                D = f(A, pd['x'], pd['y'], pd['i_neighbors'], pd['j_neighbors'])
                assert u32hex(D) == pd['D'], (c['family'], N, pd['x'], pd['y'])


@pytest.mark.parametrize('n', [4, 5, 8, 64, 65, 129])
def test_closed_form_complete(n):
    A = bd.complete(n)
    C = bo.balanced_forman_curvature(A)
    assert np.array_equal(bits(C[A != 0]), np.full(n * (n - 1), bits(bd.complete_value(n))))
    assert np.array_equal(bits(bd.curvature(A)), bits(C))


def test_closed_form_complete_known_values():
    assert [float(bd.complete_value(n)) for n in (4, 5, 8, 65)] == [2.0, 1.75, float(np.float32(1.4285715)), 1.046875]


@pytest.mark.parametrize('n', [7, 65, 300])
def test_closed_form_star(n):
    A = bd.star(n)
    C = bo.balanced_forman_curvature(A)
    assert np.array_equal(bits(C[A != 0]), np.full(2 * (n - 1), bits(bd.star_value(n))))
    assert np.array_equal(bits(bd.curvature(A)), bits(C))


@pytest.mark.parametrize('n', [5, 64, 65])
def test_closed_form_cycle(n):
    A = bd.cycle(n)
    C = bo.balanced_forman_curvature(A)
    assert float(bd.cycle_value(n)) == 1.0
    assert np.array_equal(bits(C[A != 0]), np.full(2 * n, bits(bd.cycle_value(n))))
    assert np.array_equal(bits(bd.curvature(A)), bits(C))


@pytest.mark.parametrize('name', NAMES)
def test_a_kernel_that_loses_its_tail_is_caught(name):
    """Discrimination: with the loop cut at the start of its last trip (k_limit = 64 * ((N - 1) // 64), or N - 64 where N is
    a multiple of 64) the curvature differs on at least one non-zero pair, and so does at least one post-delta query."""
    _, A, _, _ = BY_NAME[name]
    N = A.shape[0]
    limit = bd.tail_limit(N)
    assert limit == (N - 64 if N in (64, 128) else 64 * ((N - 1) // 64)) and 0 <= limit < N
    full, cut = bd.curvature(A), bd.curvature(A, k_limit=limit)
    nz = A != 0
    n_diff = int(np.count_nonzero(bits(full)[nz] != bits(cut)[nz]))
    print(f'{name}: k_limit {limit}: {n_diff} of {int(nz.sum())} non-zero pairs change')
    assert n_diff >= 1
    hits = 0
    for x, y, i_nb, j_nb in queries_of(name):
        d = bits(bd.post_delta(A, x, y, i_nb, j_nb)) != bits(bd.post_delta(A, x, y, i_nb, j_nb, z_limit=limit))
        hits += bool(d.any())
    assert hits >= 1


def test_special_entries_of_directed_tail():
    for name, A, sp, directed in FAMILY:
        if not directed:
            continue
        s, (u, v), q = sp['source'], sp['two'], sp['diag']
        assert A[:, s].sum() == 0 and A[s].sum() >= 2 and A[u, v] == 2.0 and A[q, q] == 1.0
        assert set(np.unique(A)) == {0.0, 1.0, 2.0}
        C = oracle_curvature(name)[0]
        assert not C[s].any()                              # d_in[s] == 0: the degree product is zero
        assert C[u, v] != 0 and C[q, q] != 0
        assert not np.array_equal(A, A.T)


def test_tied_graphs_are_tied():
    """The SDRF tie-break test (GPU) relies on it: on the torus and on the copies the oracle's first-iteration minimum is
    attained more than once."""
    for A, n_tied_at_least in ((bd.torus(18, 18), 1296), (bd.copies(bd.cycle(5), 40), 2), (bd.copies(bd.complete(4), 33), 2)):
        C = bo.balanced_forman_curvature(A)
        assert int(np.sum(C == C.min())) >= n_tied_at_least
        assert int(np.sum(C == C.max())) > 1


def test_query_set_of_the_gpu_test_covers_its_shapes():
    """Over the whole set of post-delta queries dim_i * dim_j takes all four residues mod 4 (the last workgroup of
    k_bfc_dense_post_delta holds 1, 2, 3 and 4 waves) and one query has more than 100 x 5 entries."""
    residues, largest = set(), 0
    for name in NAMES:
        for x, y, i_nb, j_nb in all_queries(name):
            residues.add(len(i_nb) * len(j_nb) % 4)
            largest = max(largest, len(i_nb) * len(j_nb))
    assert residues == {0, 1, 2, 3} and largest > 500
