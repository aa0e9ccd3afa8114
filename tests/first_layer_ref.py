"""Inputs, exact references and plan restatements for the tests of csrc/dcr_gcn_first.hip (the one-kernel first GCN layer:
``dcr_first_layer_fwd_ws_f32_dev``, ``dcr_first_layer_bwd_f32_dev``).  numpy only; nothing here imports the package under test.

    forward    pre = (Â·X)·W1ᵀ + b1,   h = keep ? pre·scale : 0,   z_train = h·W2ᵀ,   z_eval = relu(pre)·W2ᵀ
    backward   dpre = keep ? (dz·W2)·scale : 0,   db1 = Σ_rows dpre,   dW2 = dzᵀ·(keep ? pre·scale : 0),   dW1 = dpreᵀ·(Â·X)

All operands are small integers held in float32 — Â·X, W1 and dz in −2 … 2, W2 in −1 … 1, b1 in −3 … 3, the backward's pre in
−4 … 4, scale = 1 / (1 − p) with p in {0, 0.5}: 1 or 2 — so every product is an integer, and while the sum of the ABSOLUTE
products of an output entry stays below 2**24 every fp32 partial sum of them, taken in any order and grouped in any way (MFMA
chains, K chunks added by the last workgroup, workgroup parts added by the slab reduction), is an exactly representable integer:
the device must EQUAL the int64 result and the tolerance is zero.  ``assert_exact`` checks that condition entry by entry for every
output; it is an assert, not a tolerance.  tests/test_first_layer_ref_cpu.py runs it for every shape the GPU file uses and shows
that the mistakes these kernels could make each break the equality.

The plan restatements cite csrc/dcr_gcn_first.hip by function and line; tests/test_first_layer_exact_gpu.py holds them against
the device (workspace sizes through the ABI, the CU count) in every case, so a changed plan fails a test instead of quietly
testing less."""
import numpy as np
import torch

import atb_ref
import dropout_ref

SENTINEL = atb_ref.SENTINEL
sentinel_filled = atb_ref.sentinel_filled
same_bits = atb_ref.same_bits

EXACT_LIMIT = 2 ** 24
LDX_PAD, EXTRA_ROWS, LDZ_PAD, WS_GUARD = 8, 16, 6, 64
ROW_LIMIT = 100000          # a case whose derived row count exceeds this on the device at hand is skipped, with the reason


def cdiv(a, b):
    return -(-int(a) // int(b))


def f16_of(feats):
    return cdiv(feats, 16) * 16


def scale_of(p):
    assert p in (0.0, 0.5)
    return 1 if p == 0.0 else 2


# ---- the plans, restated from csrc/dcr_gcn_first.hip -------------------------------------------------------------------------
# (source line, text that must stand there): tests/test_first_layer_ref_cpu.py reads the file and compares
CITED = {
    325: 'static size_t first_layer_lds_bytes(int F, int H) { return sizeof(float) * ((size_t)H * ((F + 63) / 64 * 64) + 16 * (size_t)H + H); }',
    342: 'int64_t grid = (n_units + FIRST_WAVES * NR - 1) / (FIRST_WAVES * NR);',
    343: 'if (grid > cus) grid = cus;',
    345: 'const int64_t upw = (n_units + waves - 1) / waves;',
    509: 'constexpr int CU_ = 32 / HM;',
    538: 'static int64_t wide_chunks(int F, int H) { return ((F + 15) / 16 * 16 + 16384 / H - 1) / (16384 / H); }',
    539: 'static int64_t wide_groups(int64_t n_rows) { return ((n_rows + 15) / 16 + 3) / 4; }',
    541: 'return wide_chunks(F, H) * ((n_rows + 15) / 16 * 16) * H + wide_groups(n_rows);',
    557: 'int64_t gx = (2 * (int64_t)cus + n_chunks - 1) / n_chunks;',
    558: 'if (gx > n_groups) gx = n_groups;',
    959: 'const int64_t n_stages = ((n_rows + 15) / 16 + BWD_UR - 1) / BWD_UR;',
    961: 'int64_t blocks = ((int64_t)cus * BWD_WGS + fblocks - 1) / fblocks;',
    962: 'if (blocks > n_stages) blocks = n_stages;',
    971: 'return in_features >= 16 && (in_features % 16) == 0 && first_layer_lds_bytes(in_features, hidden) <= 160 * 1024;',
    1089: 'const int64_t upw = (n_stages + blocks - 1) / blocks;',
}
FIRST_WAVES, FIRST_NR, BWD_UR, BWD_WGS = 8, 2, 2, 1     # DCR_FIRST_WAVES, DCR_FIRST_NR, DCR_BWD_UR, 8 / DCR_BWD_WAVES (lines 31-34, 652-657)


def first_layer_resident(feats, hidden):
    """first_layer_resident (line 970) with first_layer_lds_bytes (line 325): W1 whole in one CU's LDS."""
    lds = 4 * (hidden * cdiv(feats, 64) * 64 + 16 * hidden + hidden)
    return feats >= 16 and feats % 16 == 0 and lds <= 160 * 1024


def resident_wave_units(n, cus):
    """launch_first_layer (lines 341-345) and k_first_layer_fwd (lines 304-307): the number of 16-row units in the range of
    every wave that has one.  A wave walks its range NR = 2 units at a time and takes what is left one by one (lines 311-322)."""
    n_units = cdiv(n, 16)
    grid = min(cdiv(n_units, FIRST_WAVES * FIRST_NR), cus)
    upw = cdiv(n_units, grid * FIRST_WAVES)
    return [min(upw, n_units - w * upw) for w in range(grid * FIRST_WAVES) if w * upw < n_units]


def resident_rows_pair_then_single(cus):
    """The smallest n at which a wave of k_first_layer_fwd takes NR = 2 units together and ends on a single one.  While
    n_units <= 16·cus the grid grows with the rows and no wave has more than 2 units; at n_units = 16·cus + 1 the grid is at
    its cap of cus workgroups and units_per_wave = 3: n = 256·cus + 1."""
    return 256 * cus + 1


def resident_rows_prefetch(cus):
    """The smallest n at which units_per_wave = 4: a wave takes two pairs, the second one's first piece loaded under the first
    one's epilogue (first_chunk's u_next, line 315)."""
    return 384 * cus + 1


def wide_kch(hidden):
    return 16384 // hidden                                  # wide_kch (line 379): columns of W1 per chunk


def wide_chunks(feats, hidden):
    return cdiv(f16_of(feats), wide_kch(hidden))            # line 538


def wide_groups(n):
    return cdiv(cdiv(n, 16), 4)                             # line 539


def wide_ws_floats(n, feats, hidden):
    return wide_chunks(feats, hidden) * cdiv(n, 16) * 16 * hidden + wide_groups(n)      # lines 540-542


def wide_gx(n, feats, hidden, cus):
    """launch_first_layer_wide (lines 557-559): workgroups along the row groups; workgroup x walks groups x, x + gx, …"""
    return max(min(cdiv(2 * cus, wide_chunks(feats, hidden)), wide_groups(n)), 1)


def wide_in_flight(hidden):
    return 32 // (hidden // 16)                             # line 509: chunks' tiles the closing loop loads per batch (32 / HM)


def bwd_stages(n):
    return cdiv(cdiv(n, 16), BWD_UR)                        # line 959 (a stage is BWD_UR = 2 units: 32 rows)


def bwd_blocks(n, feats, cus):
    """first_layer_bwd_blocks (lines 951-964): workgroups along the rows."""
    fblocks = cdiv(f16_of(feats), 256)
    return max(min(cdiv(cus * BWD_WGS, fblocks), bwd_stages(n)), 1)


def bwd_stages_per_wg(n, feats, cus):
    return cdiv(bwd_stages(n), bwd_blocks(n, feats, cus))   # line 1089


def bwd_ws_floats(n, feats, hidden, cus):
    return bwd_blocks(n, feats, cus) * (hidden * f16_of(feats) + 17 * hidden)           # line 1062


def bwd_rows_for(stages_per_wg, residue, feats, cus):
    """n with ``residue`` rows (1 … 32) in its last stage such that every workgroup but the last walks ``stages_per_wg`` stages
    and the last one one fewer (stages_per_wg = 1: all one)."""
    full = cdiv(cus * BWD_WGS, cdiv(f16_of(feats), 256))
    n_stages = full if stages_per_wg == 1 else stages_per_wg * full - 1
    n = 32 * (n_stages - 1) + residue
    assert 1 <= residue <= 32 and bwd_stages(n) == n_stages and bwd_blocks(n, feats, cus) == full
    assert bwd_stages_per_wg(n, feats, cus) == stages_per_wg
    return n


# ---- the cases of tests/test_first_layer_exact_gpu.py (functions of the CU count where the plan depends on it) ---------------
RESIDENT_SHAPES = ((16, 128), (64, 128), (80, 128), (256, 128), (576, 64))        # (feats, hidden)
RESIDENT_ROWS = (1, 15, 16, 17, 31, 33)
CLASSES = (1, 7, 16)
# (hidden, feats, chunks)
WIDE_SHAPES = ((128, 23, 1), (128, 272, 3), (128, 512, 4), (128, 528, 5), (128, 1040, 9),
               (64, 592, 3), (64, 1792, 7), (64, 2048, 8), (64, 2064, 9), (64, 4112, 17))
WIDE_ROWS = (1, 63, 64, 65)
WIDE_WALK = (4112, 64)                                     # (feats, hidden) of the case with n_groups > gx
BWD_SMALL_FEATS = (16, 240, 256, 272)
BWD_DEEP_FEATS = 3703
BWD_RESIDUES = (1, 15, 16, 17, 31, 32)                     # rows of the last stage; 32: n mod 32 = 0
BWD_STAGES_PER_WG = (1, 2, 3, 4)
BWD_PIPELINE_EXTRA = ((272, 128, 7, 2, 17), (16, 64, 16, 2, 31), (272, 64, 1, 3, 32))   # (feats, hidden, classes, stages per wg, residue)


def wide_walk_rows(cus):
    """n just above gx·64 rows: n_groups = gx + 1, so workgroup 0 keeps its chunk of W1 and walks two row groups."""
    feats, hidden = WIDE_WALK
    gx = cdiv(2 * cus, wide_chunks(feats, hidden))
    return gx * 64 + 1


def bwd_deep_cases(cus):
    """(hidden, classes, stages per workgroup, residue, n): every stage depth at every (hidden, classes), the six residues dealt
    so that each depth sees all of them."""
    out = []
    for s in BWD_STAGES_PER_WG:
        k = 0
        for hidden in (64, 128):
            for classes in CLASSES:
                residue = BWD_RESIDUES[(k + s) % 6]
                out.append((hidden, classes, s, residue, bwd_rows_for(s, residue, BWD_DEEP_FEATS, cus)))
                k += 1
    return out


# ---- operands ----------------------------------------------------------------------------------------------------------------
def _ints(rng, lo, hi, shape, pattern):
    """Seeded integers in lo … hi plus a pattern that differs along rows and columns (a transposed or shifted index map cannot
    give the same result), clipped back into the range."""
    return np.clip(rng.integers(lo, hi + 1, size=shape, dtype=np.int64) + pattern, lo, hi)


def forward_operands(n, feats, hidden, classes, seed):
    """int64 Â·X [n, feats], W1 [hidden, feats], b1 [hidden], W2 [classes, hidden]."""
    rng = np.random.default_rng(seed)
    r = np.arange(n, dtype=np.int64)[:, None]
    f = np.arange(feats, dtype=np.int64)[None, :]
    h = np.arange(hidden, dtype=np.int64)[:, None]
    ax = _ints(rng, -2, 2, (n, feats), (r + 2 * f) % 3 - 1)
    w1 = _ints(rng, -2, 2, (hidden, feats), (3 * h + f) % 5 - 2)
    b1 = _ints(rng, -3, 3, (hidden,), np.arange(hidden, dtype=np.int64) % 3 - 1)
    w2 = _ints(rng, -1, 1, (classes, hidden), (np.arange(classes, dtype=np.int64)[:, None] + h.T) % 2)
    return dict(ax=ax, w1=w1, b1=b1, w2=w2)


def dz_rows(n, classes, rng, dense_every=1):
    """int64 dz [n, classes] in −2 … 2.  Row r is dense when r % dense_every == 0 and one-hot (±1 or ±2 in one class) otherwise:
    thinner rows keep the sums of absolute products of the long, wide shapes low without leaving any row out of the sums."""
    r = np.arange(n, dtype=np.int64)[:, None]
    c = np.arange(classes, dtype=np.int64)[None, :]
    dz = _ints(rng, -2, 2, (n, classes), (2 * r + c) % 3 - 1)
    if dense_every > 1:
        hot = rng.integers(0, classes, size=n)
        val = rng.choice(np.array([-2, -1, 1, 2], dtype=np.int64), size=n)
        thin = np.zeros_like(dz)
        thin[np.arange(n), hot] = val
        dz = np.where(r % dense_every == 0, dz, thin)
    return dz


def backward_operands(n, feats, hidden, classes, seed, dense_every=1):
    """int64 Â·X [n, feats], dz [n, classes], W2 [classes, hidden], pre [n, hidden] (−4 … 4) and a boolean keep mask [n, hidden]
    from numpy's generator: tied neither to Philox nor to the sign of pre."""
    rng = np.random.default_rng(seed)
    r = np.arange(n, dtype=np.int64)[:, None]
    f = np.arange(feats, dtype=np.int64)[None, :]
    h = np.arange(hidden, dtype=np.int64)[None, :]
    ax = _ints(rng, -2, 2, (n, feats), (r + 2 * f) % 3 - 1)
    dz = dz_rows(n, classes, rng, dense_every)
    w2 = _ints(rng, -1, 1, (classes, hidden), (np.arange(classes, dtype=np.int64)[:, None] + h) % 2)
    pre = _ints(rng, -4, 4, (n, hidden), (3 * r + h) % 5 - 2)
    keep = rng.random((n, hidden)) < 0.6
    return dict(ax=ax, dz=dz, w2=w2, pre=pre, keep=keep)


def forward_case_operands(n, feats, hidden, classes):
    """The operands of the GPU file's forward case of this shape (the seed is the shape's)."""
    return forward_operands(n, feats, hidden, classes, seed=(n * 4099 + feats) * 131 + hidden + classes)


def backward_case_operands(n, feats, hidden, classes):
    """The operands of the GPU file's backward case of this shape; dz thinned to one dense row in four at the wide and the long
    shapes."""
    dense_every = 4 if feats > 1024 or n > 4096 else 1
    return backward_operands(n, feats, hidden, classes, seed=(n * 4099 + feats) * 131 + hidden + classes, dense_every=dense_every)


# ---- exact references --------------------------------------------------------------------------------------------------------
def matmul_exact(A, B):
    """A·B of int64 matrices, formed in float64 (exact: every partial sum is an integer far below 2**53) through the BLAS."""
    A, B = np.asarray(A), np.asarray(B)
    bound = float(np.abs(A).max(initial=0)) * float(np.abs(B).max(initial=0)) * max(A.shape[-1], 1)
    assert bound < 2 ** 53
    C = A.astype(np.float64) @ B.astype(np.float64)
    Ci = np.rint(C).astype(np.int64)
    assert np.array_equal(Ci.astype(np.float64), C)
    return Ci


def assert_exact(name, abs_sum):
    """The exactness guard: ``abs_sum`` holds, per output entry, the sum of the absolute values of everything added into it."""
    worst = int(np.max(abs_sum, initial=0))
    assert worst < EXACT_LIMIT, f'{name}: an entry adds absolute products up to {worst} >= 2**24; its fp32 partial sums need not be exact'
    return worst


def forward_pre(ops):
    """pre in int64, guarded."""
    pre = matmul_exact(ops['ax'], ops['w1'].T) + ops['b1'][None, :]
    assert_exact('pre', matmul_exact(np.abs(ops['ax']), np.abs(ops['w1']).T) + np.abs(ops['b1'])[None, :])
    return pre


def forward_reference(ops, keep, scale):
    """(pre, z_train, z_eval) in int64 for a boolean keep mask [n, hidden].  The guard of both z bounds |h| by relu(pre)·scale,
    which holds for every mask that keeps only positive entries — so it can run before the device has drawn one."""
    pre = forward_pre(ops)
    relu = np.maximum(pre, 0)
    keep = np.asarray(keep, dtype=np.bool_).reshape(pre.shape)
    assert not (keep & (pre <= 0)).any(), 'a keep bit on an entry that is not positive'
    assert_exact('z_train, z_eval', matmul_exact(relu * scale, np.abs(ops['w2']).T))
    z_train = matmul_exact(np.where(keep, pre * scale, 0), ops['w2'].T)
    z_eval = matmul_exact(relu, ops['w2'].T)
    return pre, z_train, z_eval


def backward_reference(ops, scale):
    """(dpre, db1, dW2, dW1) in int64 for ops['keep'], every output guarded."""
    keep, dz, w2, pre, ax = ops['keep'], ops['dz'], ops['w2'], ops['pre'], ops['ax']
    assert_exact('dpre', matmul_exact(np.abs(dz), np.abs(w2)) * scale)
    dpre = np.where(keep, matmul_exact(dz, w2) * scale, 0)
    h = np.where(keep, pre * scale, 0)
    assert_exact('db1', np.abs(dpre).sum(0))
    assert_exact('dW2', matmul_exact(np.abs(dz).T, np.abs(h)))
    assert_exact('dW1', matmul_exact(np.abs(dpre).T, np.abs(ax)))
    return dpre, dpre.sum(0), matmul_exact(dz.T, h), matmul_exact(dpre.T, ax)


# ---- device-layout buffers ---------------------------------------------------------------------------------------------------
def ax_buffer(ax, extra_rows=EXTRA_ROWS, pad=LDX_PAD):
    """fp32 [n + extra_rows, F16 + pad]: Â·X in the leading columns, ZERO in the columns feats … F16 (the forward's contract), a
    quiet NaN in the columns F16 … ldx and in the rows past n."""
    n, feats = ax.shape
    F16 = f16_of(feats)
    buf = np.full((n + extra_rows, F16 + pad), np.nan, dtype=np.float32)
    buf[:n, :F16] = 0.0
    buf[:n, :feats] = ax
    return torch.from_numpy(buf)


def rows_buffer(X, extra_rows=EXTRA_ROWS):
    """fp32 [rows + extra_rows, width]: X, then rows of quiet NaN."""
    return atb_ref.padded(np.asarray(X), X.shape[1], extra_rows)


def f32(X):
    return torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))


def pack_keep(keep, extra_words=4):
    """The keep mask as include/dcr.h's bit words (dropout_ref.pack_bits), as int64 for torch; bits of no element and the extra
    words are zero."""
    n = keep.size
    words = dropout_ref.pack_bits(keep, n, words=dropout_ref.bits_words(n) + extra_words)
    return torch.from_numpy(words.view(np.int64).copy())


# ---- fp32 emulations that add in the kernels' groupings, in a scrambled order, with planted faults ---------------------------
FORWARD_FAULTS = ('chunk_added_twice', 'chunk_skipped', 'b1_once_per_chunk', 'keep_bit_one_column_on')
BACKWARD_FAULTS = ('unit_dropped', 'stage_reads_previous_rows_of_ax', 'keep_bit_one_column_on', 'pad_column_in_dw1')


def emulate_forward(ops, keep, scale, seed, fault=None):
    """fp32 (pre, z_train, z_eval) the way k_first_layer_wide adds: a partial tile per K chunk of wide_kch columns (its columns
    added in a shuffled order), the chunks' tiles added in a shuffled order, + b1, then the second contraction over the hidden
    columns in a shuffled order.  ``fault`` plants one mistake."""
    rng = np.random.default_rng(seed)
    ax, w1 = ops['ax'].astype(np.float32), ops['w1'].astype(np.float32)
    b1, w2 = ops['b1'].astype(np.float32), ops['w2'].astype(np.float32)
    n, feats = ax.shape
    hidden = w1.shape[0]
    kch = wide_kch(hidden)
    chunks = wide_chunks(feats, hidden)
    parts = []
    for c in range(chunks):
        cols = np.arange(c * kch, min(feats, (c + 1) * kch))
        rng.shuffle(cols)
        acc = np.zeros((n, hidden), dtype=np.float32)
        for k in cols:
            acc += np.outer(ax[:, k], w1[:, k]).astype(np.float32)
        if fault == 'b1_once_per_chunk':
            acc += b1[None, :]
        parts.append(acc)
    order = list(rng.permutation(chunks))
    if fault == 'chunk_added_twice':
        order.append(order[0])
    if fault == 'chunk_skipped':
        order = order[1:]
    pre = np.zeros((n, hidden), dtype=np.float32)
    for c in order:
        pre += parts[c]
    if fault != 'b1_once_per_chunk':
        pre += b1[None, :]
    keep = np.asarray(keep, dtype=np.bool_).reshape(n, hidden)
    if fault == 'keep_bit_one_column_on':
        keep = np.roll(keep, 1, axis=1)
    h_tr = np.where(keep, pre * np.float32(scale), np.float32(0.0)).astype(np.float32)
    h_ev = np.maximum(pre, np.float32(0.0))
    z_tr = np.zeros((n, w2.shape[0]), dtype=np.float32)
    z_ev = np.zeros_like(z_tr)
    for k in rng.permutation(hidden):
        z_tr += np.outer(h_tr[:, k], w2[:, k]).astype(np.float32)
        z_ev += np.outer(h_ev[:, k], w2[:, k]).astype(np.float32)
    return pre, z_tr, z_ev


def emulate_backward(ops, scale, blocks, seed, fault=None):
    """fp32 (db1, dW2, dW1) the way k_first_layer_bwd adds: the stages of 32 rows dealt to ``blocks`` workgroups in contiguous
    ranges, each workgroup adding its stages' rows (in a shuffled order) into its own part, partial dW1 tiles F16 columns wide
    with the pad column taken from the Â·X buffer, then the parts added in a shuffled order and dW1 cut to the true width."""
    rng = np.random.default_rng(seed)
    dz, w2, pre, keep = (ops[k] for k in ('dz', 'w2', 'pre', 'keep'))
    n, feats = ops['ax'].shape
    hidden = w2.shape[1]
    F16 = f16_of(feats)
    axb = np.zeros((n, F16), dtype=np.float32)
    axb[:, :feats] = ops['ax']
    axb[:, feats:] = 1.0 if fault == 'pad_column_in_dw1' else 0.0          # (the backward promises nothing about a finite pad)
    if fault == 'keep_bit_one_column_on':
        keep = np.roll(keep, 1, axis=1)
    dpre = np.where(keep, (dz.astype(np.float32) @ w2.astype(np.float32)) * np.float32(scale), np.float32(0.0)).astype(np.float32)
    h = np.where(keep, pre.astype(np.float32) * np.float32(scale), np.float32(0.0)).astype(np.float32)
    dzf = dz.astype(np.float32)
    n_stages = bwd_stages(n)
    per = cdiv(n_stages, blocks)
    p_b1 = np.zeros((blocks, hidden), dtype=np.float32)
    p_w2 = np.zeros((blocks, dz.shape[1], hidden), dtype=np.float32)
    p_w1 = np.zeros((blocks, hidden, F16), dtype=np.float32)
    dropped = cdiv(n, 16) // 2                                              # the unit a planted fault leaves out
    for b in range(blocks):
        for st in range(b * per, min(n_stages, (b + 1) * per)):
            rows = np.arange(32 * st, min(n, 32 * st + 32))
            if fault == 'unit_dropped':
                rows = rows[rows // 16 != dropped]
            rng.shuffle(rows)
            for r in rows:
                xr = r
                if fault == 'stage_reads_previous_rows_of_ax' and st == n_stages - 1 and st > 0 and r - 32 >= 0:
                    xr = r - 32
                p_b1[b] += dpre[r]
                p_w2[b] += np.outer(dzf[r], h[r]).astype(np.float32)
                p_w1[b] += np.outer(dpre[r], axb[xr]).astype(np.float32)
    db1 = np.zeros(hidden, dtype=np.float32)
    dw2 = np.zeros_like(p_w2[0])
    dw1 = np.zeros_like(p_w1[0])
    for b in rng.permutation(blocks):
        db1 += p_b1[b]
        dw2 += p_w2[b]
        dw1 += p_w1[b]
    if fault == 'pad_column_in_dw1':
        # the slab reduction reading the F16-wide tiles with the true width as its stride: pad columns land in dW1
        return db1, dw2, dw1.reshape(-1)[:hidden * feats].reshape(hidden, feats)
    return db1, dw2, dw1[:, :feats]
