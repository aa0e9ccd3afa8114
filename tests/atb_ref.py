"""Inputs and exact references for the tests of csrc/dcr_gemm.hip (``dcr_atb_f32_dev``: C[M x N] = Aᵀ·B, A [K x M], B [K x N]).

With integer operands in −4 … 4 every product is an integer of magnitude <= 16 and every partial sum of up to K of them an
integer of magnitude <= 16·K.  While 16·K < 2**24 each of them is exactly representable in fp32, so an fp32 kernel equals the
integer product BIT FOR BIT whatever its summation order (k-ordered fmaf chains inside a slab, slab sums in groups of four):
the tolerance of such a test is zero.  ``assert_exact_range`` guards that condition.

No GPU is needed here; tests/test_atb_ref_cpu.py shows that these inputs tell a right kernel from a wrong one."""
import numpy as np
import torch

# one fixed quiet-NaN bit pattern (payload 0x5a5a5): memory the kernel must not write is filled with it and compared as int32
SENTINEL = 0x7FC5A5A5


def sentinel_filled(shape, device='cpu'):
    """fp32 tensor whose every element has the bits of SENTINEL."""
    return torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), SENTINEL, dtype=torch.int32,
                      device=device).view(torch.float32)


def same_bits(t, pattern):
    """Every element of the fp32 tensor ``t`` has exactly the int32 bit pattern ``pattern`` (an int, or a tensor of patterns)."""
    assert t.dtype == torch.float32
    bits = t.contiguous().view(torch.int32)
    if isinstance(pattern, torch.Tensor):
        if pattern.dtype == torch.float32:
            pattern = pattern.contiguous().view(torch.int32)
        return bits.shape == pattern.shape and bool((bits == pattern.to(bits.device)).all())
    if pattern >= 2 ** 31:
        pattern -= 2 ** 32
    return bool((bits == pattern).all())


def assert_exact_range(K):
    """Fails unless every fp32 partial sum of K products of entries in −4 … 4 is exact (16·K < 2**24)."""
    assert 0 <= K and 16 * K < 2 ** 24, f'K = {K}: 16·K reaches 2**24, fp32 partial sums of ±16 products are no longer exact'


def padded(X, ld, extra_rows):
    """The fp32 device-layout buffer [rows + extra_rows, ld] of the integer (or float) matrix X: X in the leading columns, a quiet
    NaN in every padding column and every extra row."""
    K, W = X.shape
    assert ld >= W and extra_rows >= 0
    buf = np.full((K + extra_rows, ld), np.nan, dtype=np.float32)
    buf[:K, :W] = X
    return torch.from_numpy(buf)


def int_operands(K, M, N, seed, lda=None, ldb=None, extra_rows=0):
    """int64 A [K, M], B [K, N] with entries in −4 … 4, and their fp32 buffers [K + extra_rows, lda], [K + extra_rows, ldb]
    (NaN in the padding).  A seeded draw plus a pattern that differs along rows and columns, and between A and B, so that a
    transposed, shifted or swapped index map cannot give the same product."""
    assert_exact_range(K)
    lda = M if lda is None else lda
    ldb = N if ldb is None else ldb
    rng = np.random.default_rng(seed)
    k = np.arange(K, dtype=np.int64)[:, None]
    m = np.arange(M, dtype=np.int64)[None, :]
    n = np.arange(N, dtype=np.int64)[None, :]
    A = np.clip(rng.integers(-4, 5, size=(K, M), dtype=np.int64) + (k + 2 * m) % 3, -4, 4)
    B = np.clip(rng.integers(-4, 5, size=(K, N), dtype=np.int64) + (3 * k + n) % 5 - 2, -4, 4)
    return A, B, padded(A, lda, extra_rows), padded(B, ldb, extra_rows)


def exact_product(A, B):
    """Aᵀ·B in int64.  Formed in float64, which is exact here (every partial sum is an integer far below 2**53) and goes through
    the BLAS instead of numpy's slow integer loop."""
    assert A.shape[0] == B.shape[0]
    bound = float(np.abs(A).max(initial=0)) * float(np.abs(B).max(initial=0)) * max(A.shape[0], 1)
    assert bound < 2 ** 53
    C = A.T.astype(np.float64) @ B.astype(np.float64)
    Ci = np.rint(C).astype(np.int64)
    assert np.array_equal(Ci.astype(np.float64), C)
    return Ci


def one_hot_case(K, M, N, k_star, m_star):
    """A all zero except A[k*, m*] = 1 and B[k, n] = 1 + (k·N + n) % 251 (int64): the product is zero except row m*, which is
    B[k*].  Returns A, B and that expected C."""
    assert 0 <= k_star < K and 0 <= m_star < M
    A = np.zeros((K, M), dtype=np.int64)
    A[k_star, m_star] = 1
    B = 1 + (np.arange(K, dtype=np.int64)[:, None] * N + np.arange(N, dtype=np.int64)[None, :]) % 251
    C = np.zeros((M, N), dtype=np.int64)
    C[m_star] = B[k_star]
    return A, B, C


def plan(K, M, N):
    """Restatement of csrc/dcr_gemm.hip's ``atb_plan``: (tile rows, tile columns, tiles_m, tiles_n, slabs, rows per slab).  The GPU
    tests hold its slab count against ``dcr_atb_f32_workspace`` for every case, so it cannot drift from the library unnoticed; the
    tile grid is not visible through the ABI and is taken from here."""
    tm = 128 if M > 64 else 64 if M > 32 else 32
    tn = 128 if tm == 32 else 256
    tiles_m, tiles_n = -(-M // tm), -(-N // tn)
    splits = max(512 // (tiles_m * tiles_n), 1)
    splits = max(min(splits, (K + 511) // 512), 1)
    chunk = -(-K // splits)
    chunk = max(-(-chunk // 16) * 16, 16)
    return tm, tn, tiles_m, tiles_n, max(-(-K // chunk), 1), chunk
