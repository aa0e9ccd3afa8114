"""The summation order of the attention kernels (csrc/dcr_gat.hip), restated on the host in fp32 with numpy, operation by
operation, on the inputs where that is possible bit for bit.

THE INPUTS.  s_src[:, h] = a_h and s_dst[:, h] = b_h, constant over the nodes.  Then every slot of head h has the same
pre = a_h + b_h (one fp32 addition), the same e = leaky(pre), so m = e, e − m is exactly 0 and w = expf(0).  ASSUMED: expf(0) is
exactly 1 (no ulp figure for expf is documented where this was written; the exact-quotient test of tests/test_gat_gpu.py rests
on the same assumption).  With w = 1, den is the slot count, an exact fp32, and fmaf(1, z, acc) is the one fp32 addition
acc + z.  Three kinds of head run both arms of leaky and of the backward's flag: a_h + b_h > 0, < 0 and = 0.

THE ORDER, as the file header of csrc/dcr_gat.hip promises it:

* a unit (row, head) of at most GAT_LONG slots: acc = 0.f, one operation per slot in slot order;
* a longer one: G = 256 / LPH groups, group g the slots g, g + G, ... from 0.f, the G partial sums added in group order onto 0.f;
* O = acc / den, one fp32 division; rec = (m, den), (0, 1) on a row without slots;
* a dot over a head's C channels: lane l fmaf's its VEC products (channels l·VEC ..) in channel order from 0.f, then the butterfly
  p[l] += p[l ^ k] for k = 1, 2, 4, ... over the LPH lanes, lanes past C / VEC holding 0: D = <dO[i,h,:], O[i,h,:]> per unit and
  t = <dO[i,h,:], Z[j,h,:]> per slot;
* per slot α = 1.f / den_i (w = 1), g = (α·(t − D_i))·flag, one rounding per operation (the file is built -ffp-contract=off),
  flag = pre > 0 ? 1 : slope;
* dZ[j,h,:]: fmaf(α, dO[i,h,:], acc) over the slots of row j of the transposed CSR, long rows strided by the same G;
  dS_src[j,h]: += g over the same slots in the same order;
* dS_dst[i,h]: the sum of g over the slots of target row i in slot order; a long row strided by G = 64 (k_gat_dst_sum deals
  4 lanes a row whatever LPH the other kernels ran).

THE EXACT fmaf.  numpy has no fma and float64(a)·b + c rounds twice.  ``fmaf`` below is the definition: the three fp32 operands
as integers times powers of two, the exact integer a·b + c, ONE rounding to 24 bits (or to the subnormal quantum 2⁻¹⁴⁹), ties to
even.  ``fmaf_v`` is the array form the replica runs.  Its route and why it is exact: a·b of two fp32 is exact in fp64 (48 bits);
TwoSum gives s = RN64(a·b + c) and the exact error err = a·b + c − s; where err != 0 and s's last mantissa bit is even, s is
moved to its neighbour on err's side, which makes s the ROUND-TO-ODD fp64 value of the exact sum.  Rounding to odd at p + k bits
with k >= 2 and then to nearest-even at p bits equals rounding the exact value once (Boldo and Melquiond, "Emulation of FMA and
correctly rounded sums: proved algorithms using rounding to odd", IEEE TC 2008, Theorem 1): an odd last bit at 53 bits keeps the
value off every midpoint and every representable point of the 24-bit grid that the exact value is not on.  53 >= 24 + 2, and the
fp64 grid is finer than fp32's subnormal quantum too.  tests/test_gat_order_cpu.py checks fmaf_v against fmaf on hand-built and
random triples.

The module shares no code with models/gat.py: ``csr_arrays`` builds the slot arrays from the documented rule (stable sort by
target, an added self-loop last; the source CSR by a stable sort of those slots by source)."""
import math

import numpy as np

from gat_ref import vec_lph

F32 = np.float32
GAT_LONG = 96          # tests/test_gat_order_cpu.py compares it with csrc/dcr_gat.hip
DST_LPR = 4            # k_gat_dst_sum


def groups(lph):
    """Lane groups of a workgroup: the partial sums of a long row."""
    return 256 // lph


def in_flight(lph):
    """Deal<LPH>::U: slots of a batch."""
    return 8 if lph <= 8 else 4


# ---- fmaf -----------------------------------------------------------------------------------------------------------------
def _int_exp(x):
    """x = m·2^e with m an integer, for a float that holds an fp32 value."""
    m, e = math.frexp(float(x))
    return int(m * 16777216.0), e - 24            # (|m| < 1 with at most 24 bits: the product is an exact integer)


def round_to_f32(num, exp):
    """The fp32 nearest to num·2^exp (num any integer), ties to even, as a Python float; overflow gives ±inf."""
    if num == 0:
        return 0.0
    sign, num = (-1.0, -num) if num < 0 else (1.0, num)
    q = max(exp + num.bit_length() - 24, -149)    # exponent of the result's last bit
    if q > exp:
        shift = q - exp
        rest, half = num & ((1 << shift) - 1), 1 << (shift - 1)
        num >>= shift
        if rest > half or (rest == half and num & 1):
            num += 1
        exp = q
    if exp + num.bit_length() > 128:
        return sign * math.inf
    return sign * math.ldexp(float(num), exp)


def fmaf(a, b, c):
    """fp32 fma of three fp32 values: the exact a·b + c rounded once."""
    (ma, ea), (mb, eb), (mc, ec) = _int_exp(a), _int_exp(b), _int_exp(c)
    mp, ep = ma * mb, ea + eb
    e = min(ep, ec)
    return round_to_f32((mp << (ep - e)) + (mc << (ec - e)), e)


def fmaf_twice_rounded(a, b, c):
    """What the exact one must NOT be: the fp64 sum rounded, then rounded again to fp32."""
    return float(F32(float(a) * float(b) + float(c)))


def fmaf_v(a, b, c):
    """``fmaf`` on arrays (fp32 in, fp32 out) by rounding to odd in fp64: see the module docstring."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    shape = a.shape
    p = a.astype(np.float64).reshape(-1) * b.astype(np.float64).reshape(-1)
    c = c.astype(np.float64).reshape(-1)
    s = p + c
    v = s - p
    err = (p - (s - v)) + (c - v)                                # TwoSum: p + c = s + err exactly
    bits = s.copy().view(np.int64)
    nudge = (err != 0) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)                                  # the neighbour on err's side is the larger in magnitude
    bits += np.where(nudge, np.where(away, 1, -1), 0)
    return bits.view(np.float64).astype(F32).reshape(shape)


# ---- the slot arrays ---------------------------------------------------------------------------------------------------------
def csr_arrays(edge_index, n, add_self_loops=False):
    """(rowptr, col, rowptr_t, col_t, slot_t) as numpy int64 arrays from ``edge_index = [source; target]``."""
    src, tgt = (np.asarray(r, dtype=np.int64) for r in edge_index)
    if add_self_loops:
        keep = src != tgt
        src, tgt = np.concatenate([src[keep], np.arange(n)]), np.concatenate([tgt[keep], np.arange(n)])
    perm = np.argsort(tgt, kind='stable')
    src, tgt = src[perm], tgt[perm]
    slot_t = np.argsort(src, kind='stable')
    ptr = lambda r: np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    return ptr(tgt), src, ptr(src), tgt[slot_t], slot_t


# ---- the order of a row ------------------------------------------------------------------------------------------------------
def plan_kernel(length, g):
    """The partial sums of a row of ``length`` slots as lists of slot numbers, in the order they are added."""
    if length <= GAT_LONG:
        return [range(length)]
    return [range(k, length, g) for k in range(g)]


def plan_chain(length, g):
    return [range(length)]


def plan_groups_reversed(length, g):
    return plan_kernel(length, g)[::-1]


def plan_slots_reversed(length, g):
    return [range(length - 1, -1, -1)]


def plan_other_groups(other_g):
    return lambda length, g: plan_kernel(length, other_g)


def row_sum(plan, length, g, zero, step):
    """Σ over the partial sums of ``plan`` in order onto 0, each a chain ``acc = step(acc, slot)`` from 0."""
    total = zero
    for part in plan(length, g):
        acc = zero
        for k in part:
            acc = step(acc, k)
        total = total + acc
    return total


# ---- the kernels -------------------------------------------------------------------------------------------------------------
def head_scores(a, b, slope):
    """(pre, e) per head in fp32: one addition, and the product of the slope arm."""
    pre = np.asarray(a, F32) + np.asarray(b, F32)
    return pre, np.where(pre > 0, pre, F32(slope) * pre).astype(F32)


def forward(rowptr, col, z, a, b, slope, lph, plan=plan_kernel, rows=None):
    """(O [n, H·C], rec [n·H, 2]) of k_gat_gather at unit weights; ``rows``: only these rows (the others stay 0)."""
    n, heads = rowptr.size - 1, len(a)
    c = z.shape[1] // heads
    _, e = head_scores(a, b, slope)
    out = np.zeros((n, heads * c), dtype=F32)
    rec = np.zeros((n, heads, 2), dtype=F32)
    rec[:, :, 1] = 1
    zero = np.zeros(heads * c, dtype=F32)
    for i in (range(n) if rows is None else rows):
        e0, e1 = int(rowptr[i]), int(rowptr[i + 1])
        if e1 == e0:
            continue
        zr = z[col[e0:e1]]
        acc = row_sum(plan, e1 - e0, groups(lph), zero, lambda s, k: s + zr[k])      # fmaf(1, z, acc)
        den = F32(e1 - e0)                                                           # any order of 1 + 1 + ... is exact
        out[i] = acc / den
        rec[i, :, 0], rec[i, :, 1] = e, den
    return out, rec.reshape(n * heads, 2)


def dots(x, y, heads, vec, lph):
    """<x[r, h, :], y[r, h, :]> [rows, H] as the kernels form it: per lane an fmaf chain of VEC products, then the butterfly."""
    r = x.shape[0]
    c = x.shape[1] // heads
    assert c % vec == 0 and c // vec <= lph
    lanes = np.zeros((2, r, heads, lph * vec), dtype=F32)
    lanes[0, :, :, :c], lanes[1, :, :, :c] = x.reshape(r, heads, c), y.reshape(r, heads, c)
    lanes = lanes.reshape(2, r, heads, lph, vec)
    p = np.zeros((r, heads, lph), dtype=F32)
    for q in range(vec):
        p = fmaf_v(lanes[0, ..., q], lanes[1, ..., q], p)
    k = 1
    while k < lph:
        p = p + p[..., np.arange(lph) ^ k]
        k <<= 1
    assert (p == p[..., :1]).all()                       # every lane of the group holds the same bits
    return p[..., 0]


def slot_terms(arrays, z, a, b, out, rec, d_out, slope, vec, lph):
    """Per slot of the transposed CSR and head: (α [E, H], g [E, H]); and g in the target CSR's slot order."""
    rowptr, col, rowptr_t, col_t, slot_t = arrays
    n, heads = rowptr.size - 1, len(a)
    pre, _ = head_scores(a, b, slope)
    flag = np.where(pre > 0, F32(1), F32(slope)).astype(F32)
    big_d = dots(d_out, out, heads, vec, lph)                                   # k_gat_rowdot
    den = rec.reshape(n, heads, 2)[:, :, 1]
    src = np.repeat(np.arange(n), np.diff(rowptr_t))
    alpha = (F32(1) / den[col_t]).astype(F32)                                   # expf(0) / den
    t = dots(d_out[col_t], z[src], heads, vec, lph)
    g = ((alpha * (t - big_d[col_t])).astype(F32) * flag[None, :]).astype(F32)
    gbuf = np.zeros_like(g)
    gbuf[slot_t] = g
    return alpha, g, gbuf


def backward(arrays, z, a, b, out, rec, d_out, slope, vec, lph, plan=plan_kernel, rows_t=None, terms=None):
    """(dZ, dS_src, dS_dst) of k_gat_rowdot, k_gat_expand and k_gat_dst_sum at unit weights.  ``rows_t``: only these rows of the
    transposed CSR (then dS_dst is not formed); ``terms``: a ``slot_terms`` result to reuse."""
    rowptr, col, rowptr_t, col_t, slot_t = arrays
    n, heads = rowptr.size - 1, len(a)
    c = z.shape[1] // heads
    alpha, g, gbuf = slot_terms(arrays, z, a, b, out, rec, d_out, slope, vec, lph) if terms is None else terms
    dz = np.zeros((n, heads * c), dtype=F32)
    ds_src = np.zeros((n, heads), dtype=F32)
    ds_dst = np.zeros((n, heads), dtype=F32)
    zero_z, zero_s = np.zeros((heads, c), dtype=F32), np.zeros(heads, dtype=F32)
    for j in (range(n) if rows_t is None else rows_t):
        e0, e1 = int(rowptr_t[j]), int(rowptr_t[j + 1])
        al, dr, gr = alpha[e0:e1, :, None], d_out[col_t[e0:e1]].reshape(e1 - e0, heads, c), g[e0:e1]
        dz[j] = row_sum(plan, e1 - e0, groups(lph), zero_z, lambda s, k: fmaf_v(al[k], dr[k], s)).reshape(-1)
        ds_src[j] = row_sum(plan, e1 - e0, groups(lph), zero_s, lambda s, k: s + gr[k])
    if rows_t is None:
        for i in range(n):
            e0, e1 = int(rowptr[i]), int(rowptr[i + 1])
            gr = gbuf[e0:e1]
            ds_dst[i] = row_sum(plan, e1 - e0, groups(DST_LPR), zero_s, lambda s, k: s + gr[k])
    return dz, ds_src, ds_dst


# ---- the fixtures both test modules use --------------------------------------------------------------------------------------
def long_lengths():
    """G·U − 1, G·U, G·U + 1 for every LPH whose G·U is above GAT_LONG (a batch of every group full, one slot short, one over)."""
    out = []
    for lph in (4, 8, 16, 32, 64):
        gu = groups(lph) * in_flight(lph)
        if gu > GAT_LONG:
            out += [gu - 1, gu, gu + 1]
    return sorted(out)


IN_LENGTHS = list(range(GAT_LONG + 2)) + [127, 128, 129] + long_lengths() + [2 * 512 + 1]
OUT_LENGTHS = list(range(GAT_LONG + 2)) + long_lengths()
HEAD_KINDS = ((0.75, 0.5), (-1.25, 0.5), (0.375, -0.375))       # (a_h, b_h): a + b > 0, < 0, = 0


def ladder(in_lengths=IN_LENGTHS, out_lengths=OUT_LENGTHS, pool=1268, seed=7, tail=None):
    """(edge_index int64 [2, E], n, targets, sources): node k of ``targets`` receives exactly in_lengths[k] columns, node k of
    ``sources`` sends exactly out_lengths[k]; the two sets are disjoint and hold no other slot, the partner endpoints come from a
    pool of further nodes (with repetition: duplicated columns; the first long target row has one for certain).  The columns are
    shuffled, so neither CSR keeps the order they were made in.  ``tail`` = k: one more node, the LAST, with k columns each way."""
    rng = np.random.default_rng(seed)
    n_t, n_s = len(in_lengths), len(out_lengths)
    targets, sources = np.arange(n_t), n_t + np.arange(n_s)
    first = n_t + n_s
    src, tgt = [], []
    forced = False
    for node, k in zip(targets, in_lengths):
        s = first + rng.integers(0, pool, k)
        if k > GAT_LONG and not forced:
            s[k // 2], forced = s[0], True
        src.append(s)
        tgt.append(np.full(k, node))
    for node, k in zip(sources, out_lengths):
        src.append(np.full(k, node))
        tgt.append(first + rng.integers(0, pool, k))
    n = first + pool
    if tail is not None:
        src += [first + rng.integers(0, pool, tail), np.full(tail, n)]
        tgt += [np.full(tail, n), first + rng.integers(0, pool, tail)]
        n += 1
    ei = np.stack([np.concatenate(src), np.concatenate(tgt)]).astype(np.int64)
    return ei[:, rng.permutation(ei.shape[1])], n, targets, sources


def reduced_lengths(lph):
    gu = groups(lph) * in_flight(lph)
    return [0, 1, 2, 7, 8, 9, GAT_LONG - 1, GAT_LONG, GAT_LONG + 1, gu - 1, gu, gu + 1]


def reduced_ladder(lph):
    """The ladder of the backward comparison: the lengths around the batch, the threshold and G·U of this LPH, in and out."""
    lengths = reduced_lengths(lph)
    return ladder(lengths, lengths, pool=200, seed=20 + lph)


def small_graph():
    """At most 250 nodes for the H = 64 shapes: target rows of 0, 1, 5, 95, 96, 97 and 130 slots, out-degrees 0, 3, 96 and 97,
    and the LAST node long both ways (100 slots in, 100 out)."""
    return ladder([0, 1, 5, GAT_LONG - 1, GAT_LONG, GAT_LONG + 1, 130], [0, 3, GAT_LONG, GAT_LONG + 1], pool=199, seed=3, tail=100)


def operands(n, heads, c, seed, kinds=HEAD_KINDS):
    """(z, a, b, d_out): random fp32 in ±1 and one head of each kind in turn."""
    rng = np.random.default_rng(seed)
    z = (rng.random((n, heads * c)) * 2 - 1).astype(F32)
    d_out = (rng.random((n, heads * c)) * 2 - 1).astype(F32)
    a = np.array([kinds[h % len(kinds)][0] for h in range(heads)], dtype=F32)
    b = np.array([kinds[h % len(kinds)][1] for h in range(heads)], dtype=F32)
    return z, a, b, d_out


# (H, C, offset of Z and O from a 16-byte boundary in floats) -> one forward comparison per LPH, LPH 64 three ways
ORDER_SHAPES = [(3, 16, 0), (3, 10, 0), (3, 36, 0), (3, 17, 0), (3, 256, 0), (3, 64, 1), (3, 128, 2)]
ORDER_INSTANTIATIONS = [(4, 4), (2, 8), (4, 16), (1, 32), (4, 64), (1, 64), (2, 64)]
# (H, C): the backward comparison, one small shape per LPH
BACKWARD_SHAPES = [(2, 8), (2, 10), (2, 36), (2, 17), (2, 33)]
BACKWARD_INSTANTIATIONS = [(4, 4), (2, 8), (4, 16), (1, 32), (1, 64)]
# (H, C, offset in floats) of the caps test
CAP_SHAPES = [(64, 1, 0), (64, 64, 0), (1, 256, 0), (2, 256, 0), (3, 128, 2), (2, 64, 1)]
CAP_INSTANTIATIONS = [(1, 4), (4, 16), (4, 64), (4, 64), (2, 64), (1, 64)]


def instantiation(heads, c, offset=0):
    return vec_lph(c, (heads * c,), (4 * offset,))
