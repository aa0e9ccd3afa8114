"""csrc/dcr_gemm.hip through the raw C ABI (``dcr_atb_f32_workspace`` / ``dcr_atb_f32_dev``, include/dcr.h): every tile
configuration switch and tile edge in M and N, every slab count at which the slab sum's unrolled loop or its tail changes,
every fill level of a ragged last slab, leading dimensions wider than the widths, a dirty workspace, K = 0 and the refusals.

The operands are small integers (tests/atb_ref.py), so every fp32 partial sum is exact and the result must equal the integer
product BIT FOR BIT in any summation order: the tolerance is zero.  tests/test_atb_ref_cpu.py shows that a dropped row, a slab
counted twice, a swapped 4-row interleave or a padding column in the sum would each break that equality.

Protocol of every case (``run_exact``): lda = M + 3, ldb = N + 5, sixteen rows past K, all padding NaN; C is [M, N + 7] and the
workspace ``need + 64`` floats, both pre-filled with one NaN bit pattern; after the call C[:, :N] is the exact product, C's
padding columns and the 64 floats past ``need`` keep the pattern, and a second call into the now dirty workspace gives the same
bits.  The slab count of a case is read from the ABI (``need // (M·N)``) and asserted, so a changed plan fails these tests
rather than quietly testing less."""
import ctypes

import numpy as np
import pytest
import torch

import atb_ref as ar

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY = -1, -4
PAD_A, PAD_B, PAD_C, EXTRA_ROWS, WS_GUARD = 3, 5, 7, 16, 64


def L():
    from dcr import _lib
    return _lib.lib()


def workspace_floats(K, M, N):
    need = ctypes.c_int64(-1)
    assert L().dcr_atb_f32_workspace(K, M, N, ctypes.byref(need)) == 0
    assert need.value > 0 and need.value % (M * N) == 0
    return need.value


def slab_count(K, M, N):
    """Slabs of the library's plan, from the ABI; held against the restatement whose tile grid the docstrings quote."""
    s = workspace_floats(K, M, N) // (M * N)
    assert s == ar.plan(K, M, N)[4], (K, M, N, s, ar.plan(K, M, N))
    return s


def ptr(t):
    return None if t is None else t.data_ptr()


def call(a, b, c, K, M, N, lda, ldb, ldc, ws, ws_floats):
    from models.gcn import _stream
    anchor = next(t for t in (c, ws, a, b) if t is not None)
    return L().dcr_atb_f32_dev(ptr(a), ptr(b), ptr(c), K, M, N, lda, ldb, ldc, ptr(ws), ws_floats, _stream(anchor))


def run_exact(K, M, N, a_buf, b_buf, want, label):
    """The common protocol.  ``a_buf`` [K + 16, M + 3], ``b_buf`` [K + 16, N + 5] fp32 (host or device), ``want`` the int64 product."""
    lda, ldb, ldc = M + PAD_A, N + PAD_B, N + PAD_C
    assert tuple(a_buf.shape) == (K + EXTRA_ROWS, lda) and tuple(b_buf.shape) == (K + EXTRA_ROWS, ldb)
    a, b = a_buf.cuda(), b_buf.cuda()
    want = torch.from_numpy(want).to(torch.float32).cuda()
    need = workspace_floats(K, M, N)
    C = ar.sentinel_filled((M, ldc), 'cuda')
    ws = ar.sentinel_filled(need + WS_GUARD, 'cuda')
    assert call(a, b, C, K, M, N, lda, ldb, ldc, ws, need) == 0, label
    if not torch.equal(C[:, :N], want):
        bad = (C[:, :N] != want).nonzero()
        m, n = bad[0].tolist()
        raise AssertionError((label, 'entries that differ', len(bad), 'first (m, n)', (m, n), 'got', C[m, n].item(),
                              'want', want[m, n].item()))
    assert ar.same_bits(C[:, N:], ar.SENTINEL), (label, 'padding columns of C were written')
    assert ar.same_bits(ws[need:], ar.SENTINEL), (label, 'the workspace was written past its stated size')
    first = C.clone()
    C2 = ar.sentinel_filled((M, ldc), 'cuda')
    assert call(a, b, C2, K, M, N, lda, ldb, ldc, ws, need) == 0, label
    assert ar.same_bits(C2, first), (label, 'a dirty workspace changed the result')
    assert ar.same_bits(ws[need:], ar.SENTINEL), (label, 'the workspace was written past its stated size (second call)')


def run_int_case(K, M, N, seed, label=None):
    A, B, a_buf, b_buf = ar.int_operands(K, M, N, seed, lda=M + PAD_A, ldb=N + PAD_B, extra_rows=EXTRA_ROWS)
    run_exact(K, M, N, a_buf, b_buf, ar.exact_product(A, B), label or (K, M, N))


# ---- tiles ---------------------------------------------------------------------------------------------------------------
TILE_M = (1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 160, 257)
TILE_N = (1, 7, 31, 32, 33, 127, 128, 129, 255, 256, 257, 513)


@pytest.mark.parametrize('M', TILE_M)
def test_every_tile_edge_exact(M):
    """Both sides of the configuration switches (M = 32/33: 32 x 128 -> 64 x 256 tiles, 64/65: -> 128 x 256), the second wave row
    of the 128-row configuration wholly (65 … 96) or partly (97 … 127) outside M, a second and third tile row (129, 160, 257), and
    in N the tile edges 128/129 (32-row configuration) and 256/257, N below one 32-column MFMA tile, and up to three tile
    columns.  K = 1019 is odd: two slabs of 512 and 507 rows everywhere; (257, 513) is a 3 x 3 tile grid, (129, 257) 2 x 2."""
    K = 1019
    for N in TILE_N:
        assert slab_count(K, M, N) == 2
        run_int_case(K, M, N, seed=1000 * M + N)
    if M == 257:
        assert ar.plan(K, 257, 513)[2:4] == (3, 3)
    if M == 129:
        assert ar.plan(K, 129, 257)[2:4] == (2, 2)


# ---- slabs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', (1, 2, 3, 4, 5, 12, 13, 15, 16, 17, 20, 28, 29, 32, 33))
def test_every_slab_count_exact(s):
    """k_atb_reduce: thread group zg adds slabs zg, zg + 4, …; the 16-way unrolled loop runs while z + 12 < splits and a tail
    takes the rest, so the work of a group changes at 4/5, 12/13, 16/17, 28/29 and 32/33 slabs.  K = 512·s − 5 gives exactly s
    slabs of 512 rows, the last one ragged, in the 32 x 128 and in the 128 x 256 configuration; a dropped or doubled slab cannot
    equal the integer product."""
    K = 512 * s - 5
    for M, N in ((16, 128), (128, 256)):
        assert workspace_floats(K, M, N) // (M * N) == s
        assert slab_count(K, M, N) == s and ar.plan(K, M, N)[5] == 512
        run_int_case(K, M, N, seed=7 * s + M)


def test_ragged_last_slab_every_residue():
    """K = 1024 − r, r = 0 … 15: two slabs of 512 rows, the last holding 512 − r, so that every fill level of the final 16-row
    load group — and each half of the wave, which holds the even or the odd rows — supplies the last valid row once; in the 32-row
    and the 64-row configuration.  Then K below, at and just above one load group, and K = 513 (two slabs of 272 and 241)."""
    for r in range(16):
        K = 1024 - r
        for M, N in ((16, 128), (33, 70)):
            assert slab_count(K, M, N) == 2 and ar.plan(K, M, N)[5] == 512
            run_int_case(K, M, N, seed=100 + r)
    for K, slabs, chunk in ((1, 1, 16), (2, 1, 16), (15, 1, 16), (16, 1, 16), (17, 1, 32), (513, 2, 272)):
        assert slab_count(K, 33, 70) == slabs and ar.plan(K, 33, 70)[5] == chunk
        run_int_case(K, 33, 70, seed=200 + K)


# ---- index maps ----------------------------------------------------------------------------------------------------------
def test_one_hot_rows_land_where_they_belong():
    """One 1 in A at (k*, m*): C is B[k*] in row m* and exactly zero elsewhere.  k* on both sides of the slab boundaries (K = 1531:
    three slabs of 512 rows; the library's count is read from the ABI, the slab length from the restatement that gives the same
    count) and m* on both sides of the 4-row interleave, the 32-row MFMA tile, the wave row (64) and the tile row (128) of the
    2 x 2 tile grid."""
    K, M, N = 1531, 129, 257
    assert slab_count(K, M, N) == 3
    chunk = ar.plan(K, M, N)[5]
    assert chunk == 512 and ar.plan(K, M, N)[2:4] == (2, 2)
    _, B, _ = ar.one_hot_case(K, M, N, 0, 0)
    b_buf = ar.padded(B, N + PAD_B, EXTRA_ROWS).cuda()
    a_buf = ar.padded(np.zeros((K, M), dtype=np.int64), M + PAD_A, EXTRA_ROWS).cuda()
    for k_star in (0, 1, chunk - 1, chunk, chunk + 1, K - 1):
        for m_star in (0, 3, 4, 31, 32, 63, 64, 127, 128):
            A, B1, want = ar.one_hot_case(K, M, N, k_star, m_star)
            assert np.array_equal(B1, B)
            a_buf[k_star, m_star] = 1.0
            run_exact(K, M, N, a_buf, b_buf, want, ('one hot', k_star, m_star))
            a_buf[k_star, m_star] = 0.0


# ---- strides -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,M,N,slabs', [(4099, 16, 128, 9), (2500, 100, 300, 5), (777, 64, 1433, 2)])
def test_strided_call_is_bitwise_the_contiguous_call(K, M, N, slabs):
    """Random normal data: the summation order depends on (K, M, N) alone, so the ABI call on operands with lda > M, ldb > N,
    ldc > N — finite or NaN padding — gives the bits of ``atb_hip`` on the contiguous copies, which in turn meets the 2e-6
    relative bound against fp64 of test_gcn.py::test_atb_mfma_vs_torch."""
    from models.gcn import atb_hip
    assert slab_count(K, M, N) == slabs
    lda, ldb, ldc = M + PAD_A, N + PAD_B, N + PAD_C
    g = torch.Generator(device='cuda').manual_seed(K + M + N)
    a_buf = torch.randn(K + EXTRA_ROWS, lda, device='cuda', generator=g)
    b_buf = torch.randn(K + EXTRA_ROWS, ldb, device='cuda', generator=g) + torch.arange(ldb, device='cuda') * 0.01
    a, b = a_buf[:K, :M].contiguous(), b_buf[:K, :N].contiguous()
    ref = atb_hip(a, b)
    want = a.double().t() @ b.double()
    scale = (a.double().abs().t() @ b.double().abs()).clamp_min(1.0)
    assert ((ref.double() - want).abs() / scale).max().item() < 2e-6
    need = workspace_floats(K, M, N)
    for padding in ('finite', 'nan'):
        if padding == 'nan':
            a_buf[:, M:] = float('nan')
            b_buf[:, N:] = float('nan')
            a_buf[K:] = float('nan')
            b_buf[K:] = float('nan')
        C = ar.sentinel_filled((M, ldc), 'cuda')
        ws = ar.sentinel_filled(need + WS_GUARD, 'cuda')
        assert call(a_buf, b_buf, C, K, M, N, lda, ldb, ldc, ws, need) == 0
        assert torch.equal(C[:, :N], ref) and ar.same_bits(C[:, :N], ref), padding
        assert ar.same_bits(C[:, N:], ar.SENTINEL) and ar.same_bits(ws[need:], ar.SENTINEL), padding
    # the wrapper on column slices of wider tensors (finite padding again: the slices themselves hold no NaN either way)
    wide_a = torch.randn(K, M + 9, device='cuda', generator=g)
    wide_b = torch.randn(K, N + 11, device='cuda', generator=g)
    sa, sb = wide_a[:, 4:4 + M], wide_b[:, 6:6 + N]
    assert not sa.is_contiguous() and not sb.is_contiguous()
    assert ar.same_bits(atb_hip(sa, sb), atb_hip(sa.clone(memory_format=torch.contiguous_format),
                                                 sb.clone(memory_format=torch.contiguous_format)))
    assert ar.same_bits(atb_hip(a_buf[:K, :M], b_buf[:K, :N]), ref)     # NaN all around the slices


# ---- degenerate and refused calls ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N', [(16, 32), (129, 7)])
def test_k_zero_and_null_operands(M, N):
    """K = 0 with A = B = NULL: an empty sum, C[:, :N] is +0.0 in every bit, the padding columns are left alone."""
    assert slab_count(0, M, N) == 1
    need = workspace_floats(0, M, N)
    ldc = N + PAD_C
    C = ar.sentinel_filled((M, ldc), 'cuda')
    ws = ar.sentinel_filled(need + WS_GUARD, 'cuda')
    assert call(None, None, C, 0, M, N, M + PAD_A, N + PAD_B, ldc, ws, need) == 0
    assert ar.same_bits(C[:, :N], 0)
    assert ar.same_bits(C[:, N:], ar.SENTINEL) and ar.same_bits(ws[need:], ar.SENTINEL)


def test_refusals_leave_the_output_alone():
    """Bad strides, bad shapes and null pointers are DCR_EINVAL, a workspace one float short is DCR_ECAPACITY; each leaves a
    message in dcr_last_error(), writes nothing to C, and does not disturb the next valid call."""
    K, M, N = 1019, 33, 70
    lda, ldb, ldc = M + PAD_A, N + PAD_B, N + PAD_C
    A, B, a_buf, b_buf = ar.int_operands(K, M, N, 11, lda=lda, ldb=ldb, extra_rows=EXTRA_ROWS)
    want = ar.exact_product(A, B)
    a, b = a_buf.cuda(), b_buf.cuda()
    need = workspace_floats(K, M, N)
    C = ar.sentinel_filled((M, ldc), 'cuda')
    ws = ar.sentinel_filled(need + WS_GUARD, 'cuda')
    good = dict(a=a, b=b, c=C, K=K, M=M, N=N, lda=lda, ldb=ldb, ldc=ldc, ws=ws, ws_floats=need)
    refused = [('lda = M - 1', dict(lda=M - 1), EINVAL), ('ldb = N - 1', dict(ldb=N - 1), EINVAL),
               ('ldc = N - 1', dict(ldc=N - 1), EINVAL), ('M = 0', dict(M=0), EINVAL), ('N = 0', dict(N=0), EINVAL),
               ('K = -1', dict(K=-1), EINVAL), ('NULL C', dict(c=None), EINVAL), ('NULL workspace', dict(ws=None), EINVAL),
               ('NULL A with K > 0', dict(a=None), EINVAL), ('NULL B with K > 0', dict(b=None), EINVAL),
               ('workspace one float short', dict(ws_floats=need - 1), ECAPACITY)]
    for label, change, code in refused:
        assert call(**{**good, **change}) == code, label
        assert len(L().dcr_last_error()) > 0, label
        torch.cuda.synchronize()
        assert ar.same_bits(C, ar.SENTINEL), (label, 'a refused call wrote to C')
        assert ar.same_bits(ws, ar.SENTINEL), (label, 'a refused call wrote to the workspace')
        run_exact(K, M, N, a, b, want, ('valid call after', label))
    need_out = ctypes.c_int64(-7)
    for shape in ((-1, M, N), (K, 0, N), (K, M, 0)):
        assert L().dcr_atb_f32_workspace(*shape, ctypes.byref(need_out)) == EINVAL and need_out.value == -7
    assert L().dcr_atb_f32_workspace(K, M, N, None) == EINVAL
