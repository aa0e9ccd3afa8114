"""csrc/dcr_bfc_dense.hip (k_bfc_dense, k_bfc_dense_post_delta) and the dense SDRF loop past one trip of the kernels' 64-wide
stride loop and at tied extrema, against oracle/bfc_cuda_oracle.py, the values recorded from the reference's kernels
(tests/golden/bfc_cuda_curvature_wide.json) and closed forms.  The graphs come from tests/bfc_dense_ref.py;
tests/test_bfc_dense_cpu.py proves on the CPU that each of them would catch a kernel that loses its loop's tail.
Sizes: 63, 64, 65, 127, 128, 129, 257 (trip counts 1, 1, 2 for lane 0 only, 2, 2, 3 for lane 0 only, 5).  float32 results are
compared bit for bit (as uint32): the kernels do exact integer work in float32 and then one fixed float64 expression."""
import ctypes

import numpy as np
import pytest
import torch

import bfc_dense_ref as bd
from conftest import load_golden
from oracle import bfc_cuda_oracle as bo
from test_bfc_dense_cpu import BY_NAME, NAMES, all_queries, bits, oracle_curvature, u32hex, wide_case_matrix

pytestmark = pytest.mark.gpu

DIRECTED = [n for n in NAMES if BY_NAME[n][3]]


def dev(A):
    return torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).cuda()


def device_curvature(A):
    """C of the device for the host matrix A, after the checks every call gets: float32 on the device, and a
    caller-provided C pre-filled with 7.0 is returned and overwritten everywhere."""
    from curvature.bfc_cuda import balanced_forman_curvature
    Ad = dev(A)
    C = balanced_forman_curvature(Ad, numerics='bfc_cuda')
    assert C.dtype == torch.float32 and C.is_cuda and tuple(C.shape) == A.shape
    got = C.cpu().numpy()
    C2 = torch.full_like(C, 7.0)
    assert balanced_forman_curvature(Ad, C=C2, numerics='bfc_cuda') is C2
    assert np.array_equal(bits(C2.cpu().numpy()), bits(got))
    return got


def check_curvature(A, want, label):
    got = device_curvature(A)
    nz = A != 0
    bad = np.argwhere(nz & (bits(got) != bits(want)))
    assert bad.size == 0, (label, 'first differing pair', bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))
    assert not bits(got)[~nz].any(), (label, 'a zero entry of A did not get +0.0')
    return got


# ---- k_bfc_dense --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_curvature_on_family_graphs(name):
    check_curvature(BY_NAME[name][1], oracle_curvature(name)[0], name)


@pytest.mark.parametrize('name', DIRECTED)
def test_curvature_special_entries(name):
    """Each on its own, so that a failure names the one that broke: every pair out of the node without in-edges (the
    d_max * d_min == 0 branch writes 0), the entry equal to 2 and the diagonal entry."""
    _, A, sp, _ = BY_NAME[name]
    want = oracle_curvature(name)[0]
    got = device_curvature(A)
    s, (u, v), q = sp['source'], sp['two'], sp['diag']
    out = np.nonzero(A[s])[0]
    assert len(out) >= 2
    for j in out:
        assert bits(want[s, j]) == 0 and bits(got[s, j]) == 0, ('zero in-degree', s, int(j))
    assert want[u, v] != 0 and bits(got[u, v]) == bits(want[u, v]), ('entry equal to 2', u, v, float(got[u, v]), float(want[u, v]))
    assert want[q, q] != 0 and bits(got[q, q]) == bits(want[q, q]), ('diagonal entry', q, float(got[q, q]), float(want[q, q]))


def test_recorded_values_above_64_nodes():
    from curvature.bfc_cuda import balanced_forman_post_delta
    for c in load_golden('bfc_cuda_curvature_wide.json')['cases']:
        A = wide_case_matrix(c)
        label = (c['family'], c['num_nodes'])
        got = device_curvature(A)
        assert u32hex(got[np.nonzero(A)]) == c['C'], label
        assert not bits(got)[A == 0].any(), label
        for pd in c['post_delta']:
            D = balanced_forman_post_delta(dev(A), pd['x'], pd['y'], pd['i_neighbors'], pd['j_neighbors'], numerics='bfc_cuda')
            assert u32hex(D.cpu().numpy()) == pd['D'], (label, pd['x'], pd['y'])


def test_partly_filled_last_workgroup():
    """Four waves share a workgroup: with the last 0, 1, 2 and 3 non-zero pairs of directed_tail(129) dropped, nnz mod 4
    takes all four values and the last workgroup holds 4, 3, 2 and 1 live waves."""
    A = BY_NAME['directed_tail-129'][1].copy()
    seen = set()
    for drop in range(4):
        if drop:
            nz = np.nonzero(A)
            A[nz[0][-1], nz[1][-1]] = 0.0
        seen.add(int(np.count_nonzero(A)) % 4)
        check_curvature(A, bo.balanced_forman_curvature(A), ('drop', drop))
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize('kind,n', [('complete', n) for n in (4, 5, 8, 64, 65, 129)] + [('star', n) for n in (7, 65, 300)] +
                         [('cycle', n) for n in (5, 64, 65)])
def test_closed_forms(kind, n):
    """K_n, S_n (hub with the last id; at n = 300 d_max = 299 and the count is 300) and C_n."""
    A = getattr(bd, kind)(n)
    value = getattr(bd, kind + '_value')(n)
    got = device_curvature(A)
    nz = A != 0
    assert np.array_equal(bits(got)[nz], np.full(int(nz.sum()), bits(value))), (kind, n, float(value))
    assert not bits(got)[~nz].any()


# ---- k_bfc_dense_post_delta ---------------------------------------------------------------------------------------------
def check_post_delta(A, x, y, i_nb, j_nb, label):
    from curvature.bfc_cuda import balanced_forman_post_delta
    Ad = dev(A)
    D = balanced_forman_post_delta(Ad, x, y, i_nb, j_nb, numerics='bfc_cuda')
    assert D.dtype == torch.float32 and D.is_cuda and tuple(D.shape) == (len(i_nb), len(j_nb))
    got = D.cpu().numpy()
    want = bo.balanced_forman_post_delta(A, x, y, i_nb, j_nb)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (label, x, y, 'first differing entry', bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))
    sentinel = np.array([[i == j or A[i, j] != 0 for j in j_nb] for i in i_nb])
    assert np.array_equal(got == np.float32(-1000.0), sentinel), (label, x, y)
    D2 = torch.full_like(D, 7.0)                          # a caller-provided D: returned, every entry overwritten
    assert balanced_forman_post_delta(Ad, x, y, i_nb, j_nb, D=D2, numerics='bfc_cuda') is D2
    assert np.array_equal(bits(D2.cpu().numpy()), bits(got)), (label, x, y)
    return got


@pytest.mark.parametrize('name', NAMES)
def test_post_delta_on_family_graphs(name):
    """Queries: the most negative edge, an edge at the last-id hub from both sides and, directed, an edge with a candidate
    j == x and one with a candidate i == y; the loop's own neighbour lists.  Over the whole set dim_i * dim_j takes all
    four residues mod 4 and one query exceeds 100 x 5 entries (asserted by test_bfc_dense_cpu.py on the same builder)."""
    _, A, _, directed = BY_NAME[name]
    qs = all_queries(name)
    assert len(qs) == (5 if directed else 3) and any(A.shape[0] - 1 in (q[0], q[1]) for q in qs)
    if directed:
        (x, y, i_nb, j_nb), (x2, y2, i_nb2, j_nb2) = qs[3], qs[4]
        assert any(j == x and i != j and A[i, j] == 0 for i in i_nb for j in j_nb)
        assert any(i == y2 and j != x2 and i != j and A[i, j] == 0 for i in i_nb2 for j in j_nb2)
    for x, y, i_nb, j_nb in qs:
        check_post_delta(A, x, y, i_nb, j_nb, name)


@pytest.mark.parametrize('name', ['hub_last-129', 'directed_tail-257'])
def test_post_delta_with_a_repeated_node(name):
    """A node listed twice (the dense loop's lists repeat x when x has a self-loop): its second row equals its first."""
    _, A, _, directed = BY_NAME[name]
    x, y, i_nb, j_nb = all_queries(name)[1]
    i_nb, j_nb = i_nb + [i_nb[0]], j_nb + [j_nb[1]]
    got = check_post_delta(A, x, y, i_nb, j_nb, name)
    assert np.array_equal(bits(got[-1]), bits(got[0])) and np.array_equal(bits(got[:, -1]), bits(got[:, 1]))
    assert (got[0] != np.float32(-1000.0)).any()


# ---- the dense SDRF loop at tied extrema --------------------------------------------------------------------------------
def _tied_graphs():
    return {'torus-18x18': (bd.torus(18, 18), True), 'C5x40': (bd.copies(bd.cycle(5), 40), True),
            'K4x33': (bd.copies(bd.complete(4), 33), True), 'hub_last-257': (BY_NAME['hub_last-257'][1], True),
            'directed_tail-130': (bd.directed_tail(130, 1130)[0], False)}


@pytest.mark.parametrize('tau', [float('inf'), 25.0])
@pytest.mark.parametrize('graph', ['torus-18x18', 'C5x40', 'K4x33', 'hub_last-257', 'directed_tail-130'])
def test_sdrf_dense_loop_at_tied_extrema(graph, tau):
    """Six iterations of sdrf_cuda_bfc(numerics='bfc_cuda') against the oracle, whose arg-min / arg-max over the dense matrix
    are numpy's first occurrence.  On the torus (1,296 tied entries) and the copies the extrema tie massively, so the run
    depends on which tied index the device reduction returns.  (torch documents the first occurrence for argmin / argmax,
    and that is what the MI355X returned on every graph here when this test was written; _dense_loop relies on it.)"""
    from dcr.data import Data
    from rewiring.sdrf_cuda_bfc import sdrf_cuda_bfc
    A, undirected = _tied_graphs()[graph]
    N = A.shape[0]
    if graph in ('torus-18x18', 'C5x40', 'K4x33'):
        C = bo.balanced_forman_curvature(A)
        assert np.sum(C == C.min()) > 1 and np.sum(C == C.max()) > 1      # the test keeps its point
    ei = bd.edge_index(A)
    ta, tb = [], []
    np.random.seed(3)
    want = bo.sdrf_cuda_bfc(ei, N, 6, True, 0.4, tau, undirected, trace=ta)
    np.random.seed(3)
    got = sdrf_cuda_bfc(Data(edge_index=torch.from_numpy(ei), num_nodes=N), 6, True, 0.4, tau, undirected, trace=tb,
                        numerics='bfc_cuda').edge_index.numpy()
    assert len(ta) == len(tb) == 6
    for it, (a, b) in enumerate(zip(ta, tb)):
        assert a['argmin'] == b['argmin'], (it, a['argmin'], b['argmin'])
        assert a['n_candidates'] == b['n_candidates'], it
        assert a['improvements'] == b['improvements'] and a['choice'] == b['choice'], it
        assert [list(e) for e in a['events']] == [list(e) for e in b['events']], (it, a['events'], b['events'])
    assert np.array_equal(want, got)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def _abi_inputs():
    A = dev(bd.cycle(8))
    A2 = A @ A
    d_in, d_out = A.sum(dim=0), A.sum(dim=1)
    pairs = torch.nonzero(A).contiguous()
    return A, A2, d_in, d_out, pairs


def _expect_einval(L, rc, what):
    assert rc == -1, (what, rc)
    assert L.dcr_last_error(), what


def test_abi_of_the_curvature_entry_point():
    from dcr import _lib
    L = _lib.lib()
    A, A2, d_in, d_out, pairs = _abi_inputs()
    N, nnz = A.shape[0], pairs.shape[0]
    C = torch.full((N, N), 7.0, dtype=torch.float32, device=A.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = [A.data_ptr(), A2.data_ptr(), d_in.data_ptr(), d_out.data_ptr(), N, pairs.data_ptr(), nnz, C.data_ptr(), stream]
    for pos, what in ((0, 'A'), (1, 'A2'), (2, 'd_in'), (3, 'd_out'), (7, 'C'), (5, 'pairs with nnz > 0')):
        args = list(good)
        args[pos] = None
        _expect_einval(L, L.dcr_bfc_dense_f32_dev(*args), 'NULL ' + what)
    for pos, value, what in ((4, -1, 'N < 0'), (6, -1, 'nnz < 0')):
        args = list(good)
        args[pos] = value
        _expect_einval(L, L.dcr_bfc_dense_f32_dev(*args), what)
    for pairs_ptr in (pairs.data_ptr(), None):             # nnz == 0: nothing to do, with or without pairs
        args = list(good)
        args[5], args[6] = pairs_ptr, 0
        assert L.dcr_bfc_dense_f32_dev(*args) == 0
    torch.cuda.synchronize()
    assert bool((C == 7.0).all())                           # none of the calls above touched the output
    assert L.dcr_bfc_dense_f32_dev(*good) == 0              # the well-formed call launches
    torch.cuda.synchronize()
    got, nz = C.cpu().numpy(), bd.cycle(8) != 0
    assert np.array_equal(bits(got)[nz], np.full(16, bits(bd.cycle_value(8)))) and bool((got[~nz] == 7.0).all())


def test_abi_of_the_post_delta_entry_point():
    from dcr import _lib
    L = _lib.lib()
    A, A2, _, _, _ = _abi_inputs()
    N, x, y = A.shape[0], 0, 1
    i_nb, j_nb = [1, 7, 0], [0, 2, 1]
    nb = torch.tensor(i_nb + j_nb, dtype=torch.int32, device=A.device)
    D = torch.full((3, 3), 7.0, dtype=torch.float32, device=A.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = [A.data_ptr(), A2.data_ptr(), 2.0, 2.0, N, D.data_ptr(), x, y, nb.data_ptr(), nb.data_ptr() + 12, 3, 3, stream]
    for pos, what in ((0, 'A'), (1, 'A2'), (5, 'D'), (8, 'i_neighbors'), (9, 'j_neighbors')):
        args = list(good)
        args[pos] = None
        _expect_einval(L, L.dcr_bfc_dense_post_delta_f32_dev(*args), 'NULL ' + what)
    for pos, value, what in ((4, -1, 'N < 0'), (6, -1, 'x < 0'), (6, N, 'x == N'), (7, -1, 'y < 0'), (7, N, 'y == N'),
                             (10, -1, 'dim_i < 0'), (11, -1, 'dim_j < 0')):
        args = list(good)
        args[pos] = value
        _expect_einval(L, L.dcr_bfc_dense_post_delta_f32_dev(*args), what)
    for pos in (10, 11):                                    # an empty list: nothing to do
        args = list(good)
        args[pos] = 0
        assert L.dcr_bfc_dense_post_delta_f32_dev(*args) == 0
    torch.cuda.synchronize()
    assert bool((D == 7.0).all())
    assert L.dcr_bfc_dense_post_delta_f32_dev(*good) == 0
    torch.cuda.synchronize()
    want = bo.balanced_forman_post_delta(bd.cycle(8), x, y, i_nb, j_nb)
    assert np.array_equal(bits(D.cpu().numpy()), bits(want))
