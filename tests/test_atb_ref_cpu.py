"""tests/atb_ref.py, the inputs of tests/test_atb_gemm_gpu.py, checked without a GPU: an fp32 emulation of a slabbed Aᵀ·B that
sums rows and slabs in a scrambled order equals the integer product bit for bit on these operands, and each planted fault of
the kind csrc/dcr_gemm.hip could have — a slab that loses its last row, a slab counted twice, the 4-row interleave of the MFMA
row map swapped in the write-out, a padding column let into the sum — makes it differ.  So exact equality on the GPU means
what it says."""
import numpy as np
import pytest
import torch

import atb_ref as ar

# (K, M, N, rows per slab of the emulation): one slab plus a ragged one; several slabs, M and N off the tiles; the 272-row chunk
SHAPES = [(37, 8, 5, 32), (300, 33, 70, 64), (531, 16, 129, 272)]
FAULTS = ['drop_last_row_of_a_slab', 'count_a_slab_twice', 'swap_m_with_m_xor_4', 'nan_padding_column']


def emulate(a_buf, b_buf, K, M, N, chunk, seed, fault=None):
    """fp32 Aᵀ·B from the padded buffers: per slab of ``chunk`` rows an fp32 accumulator over the rows in a shuffled order, then
    the slabs added in a shuffled order.  ``fault`` plants one mistake."""
    a, b = a_buf.numpy(), b_buf.numpy()
    rng = np.random.default_rng(seed)
    slabs = -(-K // chunk)
    parts = []
    for z in range(slabs):
        rows = np.arange(z * chunk, min(K, (z + 1) * chunk))
        if fault == 'drop_last_row_of_a_slab' and z == slabs - 1:
            rows = rows[:-1]
        rng.shuffle(rows)
        acc = np.zeros((M, N), dtype=np.float32)
        for k in rows:
            brow = b[k, :N].copy()
            if fault == 'nan_padding_column' and k == z * chunk:
                brow[N - 1] += b[k, N]
            acc += np.outer(a[k, :M], brow).astype(np.float32)
        parts.append(acc)
    order = list(rng.permutation(slabs))
    if fault == 'count_a_slab_twice':
        order.append(order[0])
    out = np.zeros((M, N), dtype=np.float32)
    for z in order:
        out += parts[z]
    if fault == 'swap_m_with_m_xor_4':
        m = np.arange(M)
        src = np.where((m ^ 4) < M, m ^ 4, m)
        out = out[src]
    return out


def as_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('K,M,N,chunk', SHAPES)
def test_scrambled_fp32_sum_is_the_integer_product(K, M, N, chunk):
    A, B, a_buf, b_buf = ar.int_operands(K, M, N, seed=K, lda=M + 3, ldb=N + 5, extra_rows=16)
    want = ar.exact_product(A, B)
    assert np.array_equal(want, A.T @ B)                                # the float64 route of exact_product is the int64 product
    for seed in (1, 2, 3):
        got = emulate(a_buf, b_buf, K, M, N, chunk, seed)
        assert np.array_equal(as_bits(got), as_bits(want.astype(np.float32))), seed


@pytest.mark.parametrize('fault', FAULTS)
@pytest.mark.parametrize('K,M,N,chunk', SHAPES)
def test_planted_fault_is_seen(K, M, N, chunk, fault):
    A, B, a_buf, b_buf = ar.int_operands(K, M, N, seed=K, lda=M + 3, ldb=N + 5, extra_rows=16)
    want = ar.exact_product(A, B).astype(np.float32)
    got = emulate(a_buf, b_buf, K, M, N, chunk, 1, fault)
    assert not np.array_equal(as_bits(got), as_bits(want))
    assert not torch.equal(torch.from_numpy(got), torch.from_numpy(want))   # the comparison the GPU tests make


def test_operands_are_small_asymmetric_and_nan_padded():
    K, M, N = 300, 33, 70
    A, B, a_buf, b_buf = ar.int_operands(K, M, N, seed=5, lda=M + 3, ldb=N + 5, extra_rows=16)
    assert A.dtype == np.int64 and B.dtype == np.int64 and A.shape == (K, M) and B.shape == (K, N)
    for X in (A, B):
        assert X.min() == -4 and X.max() == 4
    assert a_buf.dtype == torch.float32 and tuple(a_buf.shape) == (K + 16, M + 3) and tuple(b_buf.shape) == (K + 16, N + 5)
    assert np.array_equal(a_buf[:K, :M].numpy(), A.astype(np.float32)) and np.array_equal(b_buf[:K, :N].numpy(), B.astype(np.float32))
    for buf, w in ((a_buf, M), (b_buf, N)):
        assert torch.isnan(buf[:, w:]).all() and torch.isnan(buf[K:]).all() and not torch.isnan(buf[:K, :w]).any()
    # same seed, same operands; a shifted, reversed or swapped index map gives another product
    A2, B2, _, _ = ar.int_operands(K, M, N, seed=5)
    assert np.array_equal(A, A2) and np.array_equal(B, B2)
    want = ar.exact_product(A, B)
    assert not np.array_equal(want, ar.exact_product(np.roll(A, 1, axis=0), B))
    assert not np.array_equal(want, ar.exact_product(np.roll(A, 1, axis=1), B))
    assert not np.array_equal(want, ar.exact_product(A, np.roll(B, 1, axis=1)))
    assert not np.array_equal(want, ar.exact_product(A[:, ::-1], B))
    As, Bs, _, _ = ar.int_operands(K, N, N, seed=5)
    assert not np.array_equal(ar.exact_product(As, Bs), ar.exact_product(As, Bs).T)
    # the default leading dimensions are the widths
    _, _, a0, b0 = ar.int_operands(7, 3, 4, seed=0)
    assert tuple(a0.shape) == (7, 3) and tuple(b0.shape) == (7, 4) and not torch.isnan(a0).any()


def test_exact_range_guard():
    ar.assert_exact_range(17000)
    ar.assert_exact_range(2 ** 20 - 1)
    with pytest.raises(AssertionError):
        ar.assert_exact_range(2 ** 20)
    with pytest.raises(AssertionError):
        ar.int_operands(2 ** 20, 1, 1, seed=0)


def test_one_hot_case():
    K, M, N = 531, 16, 129
    A, B, C = ar.one_hot_case(K, M, N, 272, 5)
    assert A.sum() == 1 and A[272, 5] == 1 and B.min() == 1 and B.max() == 251
    assert np.array_equal(C, ar.exact_product(A, B))
    assert np.array_equal(C[5], B[272]) and not C[:5].any() and not C[6:].any()
    assert not np.array_equal(B[272], B[271]) and not np.array_equal(B[272], B[273])   # neighbouring rows are told apart
    a_buf, b_buf = ar.padded(A, M + 3, 16), ar.padded(B, N + 5, 16)
    got = emulate(a_buf, b_buf, K, M, N, 272, 1)
    assert np.array_equal(as_bits(got), as_bits(C.astype(np.float32)))
    assert not np.array_equal(as_bits(emulate(a_buf, b_buf, K, M, N, 272, 1, 'swap_m_with_m_xor_4')), as_bits(C.astype(np.float32)))


def test_sentinel_and_same_bits():
    t = ar.sentinel_filled((3, 5))
    assert t.dtype == torch.float32 and torch.isnan(t).all() and ar.same_bits(t, ar.SENTINEL)
    assert ar.same_bits(t[:, 2:], ar.SENTINEL)                          # a strided slice
    assert not ar.same_bits(torch.full((3, 5), float('nan')), ar.SENTINEL)   # another NaN is not the sentinel
    t[1, 4] = 0.0
    assert not ar.same_bits(t, ar.SENTINEL)
    z = torch.zeros(4)
    assert ar.same_bits(z, 0) and not ar.same_bits(-z, 0) and ar.same_bits(-z, 0x80000000)
    assert ar.same_bits(z, torch.zeros(4)) and not ar.same_bits(z, -torch.zeros(4))


def test_plan_restatement_at_the_shapes_the_gpu_tests_name():
    """The facts tests/test_atb_gemm_gpu.py relies on; there the slab counts are held against the library as well."""
    assert ar.plan(1019, 257, 513)[:5] == (128, 256, 3, 3, 2)
    assert ar.plan(1019, 129, 257)[:5] == (128, 256, 2, 2, 2)
    assert ar.plan(1019, 64, 257)[:5] == (64, 256, 1, 2, 2)
    assert ar.plan(1019, 32, 129)[:5] == (32, 128, 1, 2, 2)
    for s in (1, 2, 3, 4, 5, 12, 13, 15, 16, 17, 20, 28, 29, 32, 33):
        for M, N in ((16, 128), (128, 256)):
            assert ar.plan(512 * s - 5, M, N)[2:] == (1, 1, s, 512)
    for r in range(16):
        assert ar.plan(1024 - r, 16, 128)[4:] == (2, 512) and ar.plan(1024 - r, 33, 70)[4:] == (2, 512)
    assert [ar.plan(K, 33, 70)[4:] for K in (1, 2, 15, 16, 17, 513)] == [(1, 16)] * 4 + [(1, 32), (2, 272)]
    assert ar.plan(1531, 129, 257)[2:] == (2, 2, 3, 512)
    assert ar.plan(0, 16, 32)[4:] == (1, 16)
