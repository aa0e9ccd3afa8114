"""The summation order of the CSR aggregation kernels (csrc/dcr_spmm.hip), restated on the host in numpy fp32.

Every entry point promises one order, whatever (LPR, VEC) instantiation runs:

* a row of at most SPMM_LONG slots: ``acc = 0``, then ``acc = fmaf(val[e], B[col[e], :], acc)`` slot by slot;
* a longer row: G = 256 / LPR lane groups, group g the slots e0 + g, e0 + g + G, ... from ``acc = 0``, and the row is
  ``0.f + p_0 + p_1 + ... + p_{G-1}`` added in that order;
* the expand does either per relation segment of the row (the stride starting at the segment's first slot), writing zeros for
  a relation the row lacks; whether a row is long is decided by the whole row, not by the segment;
* then ``+ own block``, ``+ bias``, ReLU: one rounding each.

numpy has no fma.  With ``val`` a power of two and no underflow ``val * b`` is exact in fp32, so ``fmaf(val, b, acc)`` is the one
fp32 addition ``acc + val * b`` that numpy rounds the same way: on such inputs this module gives the kernels' bits, and random
``B`` makes every other order give different ones.  tests/test_spmm_order_cpu.py checks the module itself; tests/test_spmm_order_gpu.py
compares the kernels with it."""
import numpy as np

from rgcn_shapes import vec_lpr

SPMM_LONG = 96
F32 = np.float32


def groups(n_feat, *lds, residues=()):
    """Lane groups that share a long row: 256 / LPR of the instantiation the dispatch picks for this width and alignment."""
    return 256 // vec_lpr(n_feat, *lds, residues=residues)[1]


def chain(val, rows_of_b):
    """Slots in order into one accumulator; ``rows_of_b`` [slots, F] are the operand rows the slots gather."""
    acc = np.zeros(rows_of_b.shape[1], dtype=F32)
    for w, b in zip(val, rows_of_b):
        acc = acc + F32(w) * b
    return acc


def strided(val, rows_of_b, G):
    """G partial sums over every G-th slot, added in group order onto 0."""
    total = np.zeros(rows_of_b.shape[1], dtype=F32)
    for g in range(G):
        total = total + chain(val[g::G], rows_of_b[g::G])
    return total


def segment_sum(val, rows_of_b, G, long_row):
    return strided(val, rows_of_b, G) if long_row else chain(val, rows_of_b)


def close(sums, own=None, bias=None, relu=False):
    out = sums.astype(F32)
    if own is not None:
        out = out + own.astype(F32)
    if bias is not None:
        out = out + bias.astype(F32)
    if relu:
        out = np.where(out > 0, out, F32(0))
    return out


def plain_sums(rowptr, col, val, B, G, rows=None):
    """Row sums of A·B before the closing steps; ``rows``: the rows of A to compute (output row k = row rows[k])."""
    rows = np.arange(rowptr.size - 1) if rows is None else rows
    out = np.zeros((len(rows), B.shape[1]), dtype=F32)
    for k, i in enumerate(rows):
        e0, e1 = int(rowptr[i]), int(rowptr[i + 1])
        out[k] = segment_sum(val[e0:e1], B[col[e0:e1]], G, e1 - e0 > SPMM_LONG)
    return out


def typed_gather_sums(rowptr, col, val, rel, B, n_feat, G):
    """Row sums of the typed gather: slot e reads column block rel[e] of the wide operand; the row is ONE sum over all its slots."""
    n_rows = rowptr.size - 1
    out = np.zeros((n_rows, n_feat), dtype=F32)
    for i in range(n_rows):
        e0, e1 = int(rowptr[i]), int(rowptr[i + 1])
        picked = np.stack([B[c, r * n_feat:(r + 1) * n_feat] for c, r in zip(col[e0:e1], rel[e0:e1])]) if e1 > e0 else \
            np.zeros((0, n_feat), dtype=F32)
        out[i] = segment_sum(val[e0:e1], picked, G, e1 - e0 > SPMM_LONG)
    return out


def typed_expand(rowptr, col, val, rel, Gm, n_rel, G, self_block):
    """[n_rows, (n_rel + self_block)·F]: per row and relation the sum over that relation's slots, then the row's own copy."""
    n_rows, n_feat = rowptr.size - 1, Gm.shape[1]
    out = np.zeros((n_rows, (n_rel + self_block) * n_feat), dtype=F32)
    for i in range(n_rows):
        e0, e1 = int(rowptr[i]), int(rowptr[i + 1])
        for r in range(n_rel):
            at = e0 + np.flatnonzero(rel[e0:e1] == r)           # (sorted by relation: one contiguous segment)
            out[i, r * n_feat:(r + 1) * n_feat] = segment_sum(val[at], Gm[col[at]], G, e1 - e0 > SPMM_LONG)
        if self_block:
            out[i, n_rel * n_feat:] = Gm[i]
    return out


# ---- the inputs both test modules use -------------------------------------------------------------------------------------
N_ROWS = 70                                   # two workgroups at 64 rows per workgroup (LPR 4), eighteen at 4 (LPR 64)
N_COLS = 80                                   # rows of the gathered operand (>= N_ROWS: the own block reads row i)
LENGTHS = (400, 0, 1, 95, 96, 97, 130, 200)   # the first rows; the rest hold 0..8 slots
ONE_RELATION = {0: 2, 2: 0, 5: 1, 7: 0}       # rows whose every slot is of this relation (hubs 0, 5, 7 lack the others)
# width -> (VEC, LPR) when nothing but the width narrows VEC: one width per LPR, and 64, the hidden width of the benchmark
WIDTHS = {4: (4, 4), 7: (1, 8), 18: (2, 16), 68: (4, 32), 65: (1, 64), 64: (4, 16)}


def typed_graph(n_rel, seed=5):
    """(rowptr int64, col int32, val float32 powers of two, rel uint8 sorted inside each row)."""
    rng = np.random.default_rng(seed)
    lengths = np.array([LENGTHS[i] if i < len(LENGTHS) else rng.integers(0, 9) for i in range(N_ROWS)], dtype=np.int64)
    rowptr = np.zeros(N_ROWS + 1, dtype=np.int64)
    np.cumsum(lengths, out=rowptr[1:])
    col = rng.integers(0, N_COLS, int(rowptr[-1])).astype(np.int32)
    val = (0.5 ** rng.integers(0, 4, col.size)).astype(F32)
    rel = np.zeros(col.size, dtype=np.uint8)
    for i in range(N_ROWS):
        e0, e1 = int(rowptr[i]), int(rowptr[i + 1])
        only = ONE_RELATION.get(i)
        rel[e0:e1] = np.sort(rng.integers(0, n_rel, e1 - e0)) if only is None else min(only, n_rel - 1)
    return rowptr, col, val, rel
