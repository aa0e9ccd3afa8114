"""Per-slot fp64 restatement of the GAT aggregation WITH attention dropout, the host replica of its keep decisions, and the error
bounds the GPU tests apply to the DROP kernels of csrc/dcr_gat.hip.  Shares no code with models/gat.py: its own slot list (a
stable sort by target, an added self-loop last), index_add over slots, the keep matrix from tests/dropout_ref.py.  A duplicated
column is two slots with two decisions, so the dense count matrix of tests/gat_ref.py cannot carry the mask; it still carries
the bounds, which sum over slots whatever their decisions.

    k_s,h ∈ {0, scale}, scale = 1 / (1 − p)          (the kernels hold float32(scale); at the tested p that is within u of it)
    α_s,h = exp(e_s,h − m_i,h) / Σ_{slots of i} exp(e − m)                       m and the sum over EVERY slot of the row
    O[i,h,:] = Σ_{slots s of i} k_s,h·α_s,h·Z[col_s,h,:]

THE STREAM (include/dcr.h): nnz slots, S8 = nnz rounded up to a multiple of 8; slot pos under head h is element h·S8 + pos of an
(H·S8)-element tensor of the GCN dropout stream:  keep = dropout_ref.decisions(H·S8, p, seed, o).reshape(H, S8)[:, :nnz].

THE BOUNDS, from those of gat_ref (same notation: u = 2⁻²⁴, E = max |pre|, d_i and dT_j the slots of a target and a source row,
rho and rho_a the relative errors of w and α, which dropout does not touch: m, den and α are computed as without it).
* O: the kept slots are a subset, so the fmaf chain is no longer than d_i and Σ_kept|w·z| / den <= max|Z|; gat_ref's bound holds
  for acc / den, the closing multiply by float32(scale) adds one rounding u of a value <= scale·max|Z|, and float32(scale)
  itself is off by <= u relative (absorbed in the constant's slack: second-order terms had one u of it):
      |ΔO[i,h,:]| <= scale·(2·d_i + 8·E + 11)·u·max|Z[:,h,:]|
* dZ[j,h,:] = Σ_kept (α·k)·dO: each term carries one more rounding (the product α·k) and is at most scale times as large:
      |ΔdZ[j,h,:]| <= scale·((dT_j + 8·E + 11)·Σ_i α_ij,h + Σ_i α_ij,h·d_i)·u·max|dO[:,h,:]|
* g = α·(k·t − D)·(1 or slope).  |k·t| <= scale·T and |D| = |<dO_i, O_i>| <= C·max|dO|·scale·max|Z| = scale·T: every T of
  gat_ref's kappa becomes T' = scale·T, boundO becomes the one above, and the product k·t adds one rounding u·scale·T:
      kappa'(i,h) = (2·C + 9)·u·T' + C·max|dO|·boundO'(i,h) + rho_a(i)·2T'
      |ΔdS_dst[i,h]| <= kappa'(i,h) + d_i·u·2T'        |ΔdS_src[j,h]| <= Σ_i α_ij·kappa'(i,h) + dT_j·u·2T'·Σ_i α_ij
"""
import numpy as np
import torch

import dropout_ref
import gat_ref

U = gat_ref.U
SLOPE = gat_ref.SLOPE


def slots(edge_index, num_nodes, add_self_loops):
    """(rows, cols, rowptr, slot_t) int64 tensors: target and source of every slot in the order of the target CSR (the columns
    of ``edge_index`` sorted stably by target; with ``add_self_loops`` the input's self-loops dropped and one per node appended
    before the sort), and the slot of the target CSR behind each slot of the source CSR (stable sort by source)."""
    ei = torch.as_tensor(edge_index).cpu().long()
    src, tgt = ei[0], ei[1]
    if add_self_loops:
        off = src != tgt
        loops = torch.arange(num_nodes)
        src, tgt = torch.cat([src[off], loops]), torch.cat([tgt[off], loops])
    order = torch.argsort(tgt, stable=True)
    rows, cols = tgt[order], src[order]
    rowptr = torch.zeros(num_nodes + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=num_nodes), 0)
    return rows, cols, rowptr, torch.argsort(cols, stable=True)


def s8(nnz):
    return (int(nnz) + 7) // 8 * 8


def decisions(nnz, heads, p, seed, offset):
    """bool [nnz, H]: whether slot pos under head h is kept, from the stream rule above (o = ``offset``, already resolved)."""
    width = s8(nnz)
    if nnz == 0:
        return np.zeros((0, heads), dtype=np.bool_)
    return dropout_ref.decisions(heads * width, p, seed, offset).reshape(heads, width)[:, :nnz].T.copy()


def keep_weights(dec, p):
    """float64 [nnz, H]: 0 or 1 / (1 − p)."""
    return torch.from_numpy(np.asarray(dec, dtype=np.float64)) / (1.0 - float(p))


def aggregate(z, s_src, s_dst, rows, cols, keep, slope=SLOPE):
    """O [n, H·C] in float64 from float64 operands and keep [nnz, H] (0 or scale), slot by slot."""
    n, heads = s_src.shape
    pre = s_src[cols] + s_dst[rows]
    e = torch.where(pre > 0, pre, slope * pre)
    m = torch.full((n, heads), float('-inf'), dtype=torch.float64)
    m = m.scatter_reduce(0, rows[:, None].expand(-1, heads), e.detach(), 'amax', include_self=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    w = torch.exp(e - m[rows])
    den = torch.zeros((n, heads), dtype=torch.float64).index_add(0, rows, w)
    alpha = w / den[rows]
    zh = z.reshape(n, heads, -1)
    out = torch.zeros_like(zh).index_add(0, rows, (alpha * keep)[:, :, None] * zh[cols])
    return out.reshape(n, -1)


def aggregate_reference(z, s_src, s_dst, rows, cols, keep, d_out, slope=SLOPE):
    """(O, dZ, dS_src, dS_dst) in float64 for the upstream gradient ``d_out``."""
    leaves = [t.detach().cpu().double().clone().requires_grad_(True) for t in (z, s_src, s_dst)]
    out = aggregate(*leaves, rows, cols, keep.double(), slope)
    out.backward(d_out.detach().cpu().double())
    return (out.detach(),) + tuple(t.grad for t in leaves)


def bounds(z, s_src, s_dst, cnt, d_out, p, slope=SLOPE):
    """The four bounds of the docstring, shaped as gat_ref.bounds': 'O' and 'dZ' [n, H, 1], 'dS_src' and 'dS_dst' [n, H]."""
    z, s_src, s_dst, d_out = (t.detach().cpu().double() for t in (z, s_src, s_dst, d_out))
    scale = 1.0 / (1.0 - float(p))
    n, heads = s_src.shape
    c = z.shape[1] // heads
    alpha, pre = gat_ref.attention(s_src, s_dst, cnt, slope)
    big_e = float(pre[(cnt[None] > 0).expand_as(pre)].abs().max()) if bool((cnt > 0).any()) else 0.0
    d, d_t = cnt.sum(1), cnt.sum(0)
    max_z = z.reshape(n, heads, c).abs().amax((0, 2))
    max_g = d_out.reshape(n, heads, c).abs().amax((0, 2))
    b_o = scale * (2 * d[:, None] + 8 * big_e + 11) * U * max_z[None, :]
    col_alpha = alpha.sum(1).t()
    b_dz = scale * ((d_t[:, None] + 8 * big_e + 11) * col_alpha + torch.einsum('hij,i->jh', alpha, d)) * U * max_g[None, :]
    big_t = scale * c * max_g * max_z                                                     # T'
    rho_a = (d[:, None] + 8 * big_e + 9) * U
    kappa = (2 * c + 9) * U * big_t[None, :] + c * max_g[None, :] * b_o + rho_a * 2 * big_t[None, :]
    b_dst = kappa + d[:, None] * U * 2 * big_t[None, :]
    b_src = torch.einsum('hij,ih->jh', alpha, kappa) + d_t[:, None] * U * 2 * big_t[None, :] * col_alpha
    return {'O': b_o[:, :, None], 'dZ': b_dz[:, :, None], 'dS_src': b_src, 'dS_dst': b_dst}


RANDOM_PS = (0.1, 0.6, 0.9)
SEEDS = (20240607, (0xC0FFEE << 32) | 0x1234567)     # the second one has high key bits
OFFSETS = (0, 2 ** 32 + 5)                           # the second one has high counter bits


# ---- the graphs of the exact keep-set tests -------------------------------------------------------------------------------------
def block_lengths(c):
    """The in-degrees of the exact-test graph's targets for C channels per head: powers of two (den = d and every division
    exact), 1, 2, 8, 16, 128 and again in another order, capped at the largest power of two <= 24·C sources (one bit of a 24-bit
    integer per source and channel).  The rows start at positions 0, 1, 3, 11, 27, 155, 156, 284, 288, 304, 306, 314, 378
    (uncapped): from the second on no start is a multiple of 8 until 288, so one Philox call straddles two rows, the 8-slot row
    at 3 and the one at 306 cross a multiple of 8 inside, and the second 128-slot (parked) row starts at pos % 8 = 4."""
    cap = 1 << ((24 * c).bit_length() - 1)
    return [min(d, cap) for d in (1, 2, 8, 16, 128, 1, 128, 4, 16, 2, 8, 64, 32)]


def block_graph(c):
    """(edge_index, n, lengths): target i receives from sources 0 .. d_i − 1 in that order (no self-loops are added by the
    tests).  The nodes are the targets followed by nothing else: sources are the first max(d) nodes, n = max(#targets, max d)."""
    lengths = block_lengths(c)
    src = torch.cat([torch.arange(d) for d in lengths])
    tgt = torch.cat([torch.full((d,), i, dtype=torch.int64) for i, d in enumerate(lengths)])
    return torch.stack([src, tgt]), max(len(lengths), max(lengths)), lengths


def bit_values(n, heads, c):
    """Z [n, H·C] fp32: Z[j, h, ch] = 2^(j − 24·ch) for 24·ch <= j < 24·ch + 24, else 0: source j owns bit j % 24 of channel j // 24."""
    z = torch.zeros(n, heads, c)
    for j in range(min(n, 24 * c)):
        z[j, :, j // 24] = 2.0 ** (j % 24)
    return z.reshape(n, heads * c)


def bit_gradients(n, heads, c, lengths):
    """dO [n, H·C] fp32: dO[i, h, 0] = d_i·2^i for the targets (fewer than 24), else 0.  With α = 1 / d_i and k = 2 the term of
    target i in dZ[j, h, 0] is exactly 2·2^i: target i owns bit i.  (The bit is the target's own number, not its rank in source
    j's transposed row: one dO row cannot hold a rank per source, and the number orders the slots of every such row alike.)"""
    assert len(lengths) < 24
    g = torch.zeros(n, heads, c)
    for i, d in enumerate(lengths):
        g[i, :, 0] = float(d) * 2.0 ** i
    return g.reshape(n, heads * c)


def keep_sets_backward(lengths, n, heads, dec):
    """int64 [n, H]: the integer dZ[j, h, 0] / 2 must equal at p = 0.5 — bit i set where the slot (target i, source j) is kept;
    that slot sits at position start_i + j of the target CSR."""
    want = np.zeros((n, heads), dtype=np.int64)
    pos = 0
    for i, d in enumerate(lengths):
        for j in range(d):
            want[j] += dec[pos + j].astype(np.int64) << i
        pos += d
    return want


def keep_sets_forward(lengths, heads, c, dec):
    """int64 [rows, H, C]: the integer O[i, h, ch]·d_i / 2 must equal at p = 0.5 — bit (j % 24) of channel j // 24 set where the
    slot of source j is kept.  ``dec`` bool [nnz, H]."""
    want = np.zeros((len(lengths), heads, c), dtype=np.int64)
    pos = 0
    for i, d in enumerate(lengths):
        for j in range(d):
            want[i, :, j // 24] += dec[pos + j].astype(np.int64) << (j % 24)
        pos += d
    return want
