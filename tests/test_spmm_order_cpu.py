"""tests/spmm_order_ref.py against the dense float64 product, on inputs where every fp32 operation is exact (weights powers of
two, small integers in the operand): whatever the order, the replica must then give the product itself, bit for bit.  This says
the replica gathers the right slots into the right places; that its ORDER is the kernels' is tests/test_spmm_order_gpu.py."""
import numpy as np
import pytest

import spmm_order_ref as ref

N_REL = 3


@pytest.fixture(scope='module')
def graph():
    return ref.typed_graph(N_REL)


def dense(rowptr, col, val, rel, n_rel):
    A = np.zeros((n_rel, ref.N_ROWS, ref.N_COLS))
    rows = np.repeat(np.arange(ref.N_ROWS), np.diff(rowptr))
    np.add.at(A, (rel, rows, col), val.astype(np.float64))
    return A


def ints(shape, seed):
    return np.random.default_rng(seed).integers(-8, 9, shape).astype(np.float32)


def test_graph_has_the_rows_the_order_depends_on(graph):
    rowptr, col, val, rel = graph
    lengths = np.diff(rowptr)
    assert set(ref.LENGTHS) <= set(lengths.tolist()) and ref.SPMM_LONG in lengths and ref.SPMM_LONG + 1 in lengths
    assert all(np.all(np.diff(rel[rowptr[i]:rowptr[i + 1]].astype(int)) >= 0) for i in range(ref.N_ROWS))
    present = [set(rel[rowptr[i]:rowptr[i + 1]].tolist()) for i in range(ref.N_ROWS)]
    hubs = [i for i in range(ref.N_ROWS) if lengths[i] > ref.SPMM_LONG]
    assert any(len(present[i]) == N_REL for i in hubs) and any(len(present[i]) == 1 for i in hubs)      # a hub with an absent relation
    assert any(0 < len(present[i]) < N_REL for i in range(ref.N_ROWS) if 0 < lengths[i] <= ref.SPMM_LONG)
    assert set(np.log2(val).tolist()) <= {0.0, -1.0, -2.0, -3.0}
    # one width per LPR, so every number of lane groups a hub row can be dealt to
    assert {ref.groups(f) for f in ref.WIDTHS} == {64, 32, 16, 8, 4}
    assert all(ref.vec_lpr(f) == want for f, want in ref.WIDTHS.items())


@pytest.mark.parametrize('n_feat', sorted(ref.WIDTHS))
def test_plain_rows_equal_the_dense_product(graph, n_feat):
    rowptr, col, val, rel = graph
    B = ints((ref.N_COLS, n_feat), n_feat)
    bias = ints(n_feat, 1000 + n_feat)
    want = dense(rowptr, col, val, rel, N_REL).sum(0) @ B.astype(np.float64)
    G = ref.groups(n_feat)
    sums = ref.plain_sums(rowptr, col, val, B, G)
    assert sums.dtype == np.float32 and np.array_equal(sums.astype(np.float64), want)
    assert np.array_equal(ref.close(sums, bias=bias, relu=True).astype(np.float64), np.maximum(want + bias, 0))
    picked = np.array([5, 0, 69, 5, 1, 7], dtype=np.int64)
    assert np.array_equal(ref.plain_sums(rowptr, col, val, B, G, rows=picked).astype(np.float64), want[picked])


@pytest.mark.parametrize('n_feat', sorted(ref.WIDTHS))
@pytest.mark.parametrize('self_block', (0, 1))
def test_typed_rows_equal_the_dense_products(graph, n_feat, self_block):
    rowptr, col, val, rel = graph
    A = dense(rowptr, col, val, rel, N_REL)
    G = ref.groups(n_feat)
    wide = ints((ref.N_COLS, (N_REL + self_block) * n_feat), n_feat)
    bias = ints(n_feat, 1000 + n_feat)
    want = sum(A[r] @ wide[:, r * n_feat:(r + 1) * n_feat].astype(np.float64) for r in range(N_REL))
    own = wide[:ref.N_ROWS, N_REL * n_feat:] if self_block else None
    got = ref.close(ref.typed_gather_sums(rowptr, col, val, rel, wide, n_feat, G), own=own, bias=bias)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want + (own if self_block else 0) + bias)
    Gm = ints((ref.N_COLS, n_feat), 2000 + n_feat)
    got = ref.typed_expand(rowptr, col, val, rel, Gm, N_REL, G, self_block)
    blocks = [A[r] @ Gm.astype(np.float64) for r in range(N_REL)] + ([Gm[:ref.N_ROWS].astype(np.float64)] if self_block else [])
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), np.concatenate(blocks, axis=1))


def test_the_order_shows_in_the_bits_on_random_floats(graph):
    """What makes the GPU comparison a statement about order: on random fp32 operands another order of the same sum gives other
    bits in most elements of a long row (the short-row chain read backwards, a hub row dealt to another number of groups)."""
    rowptr, col, val, rel = graph
    B = np.random.default_rng(3).standard_normal((ref.N_COLS, 64)).astype(np.float32)
    e0, e1 = int(rowptr[4]), int(rowptr[5])                                  # 96 slots
    forward, backward = ref.chain(val[e0:e1], B[col[e0:e1]]), ref.chain(val[e0:e1][::-1], B[col[e0:e1]][::-1])
    assert np.mean(forward != backward) > 0.25
    e0, e1 = int(rowptr[0]), int(rowptr[1])                                  # 400 slots
    assert np.mean(ref.strided(val[e0:e1], B[col[e0:e1]], 16) != ref.strided(val[e0:e1], B[col[e0:e1]], 32)) > 0.25
    assert np.mean(ref.strided(val[e0:e1], B[col[e0:e1]], 16) != ref.chain(val[e0:e1], B[col[e0:e1]])) > 0.25
