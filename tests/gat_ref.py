"""Dense fp64 restatement of the GAT layer and of a whole GAT (Veličković et al. as torch_geometric's GATConv evaluates it), from
the definition alone, and the error bounds the GPU tests apply to the fp32 kernels of csrc/dcr_gat.hip.  Shares no code with
models/gat.py: one dense n x n count matrix, a masked softmax, a duplicated column weighted by its count, no CSR.

    pre_ij,h = s_src[j,h] + s_dst[i,h]    e = pre > 0 ? pre : slope·pre    α_ij,h = cnt_ij·exp(e − m_i,h) / Σ_j cnt_ij·exp(e − m_i,h)
    O[i,h,:] = Σ_j α_ij,h·Z[j,h,:]

Gradients come from autograd on this restatement.

THE BOUNDS (derived from the kernels' operations, not fitted).  u = 2⁻²⁴ is the unit roundoff of fp32.  The kernels and the
restatement start from the same fp32 operands, so only the kernels' own roundings count.  E = max |pre| over the fixture.

* the exponent's argument: one rounding each for pre (<= u·E), the leaky product (<= u·E) and e − m (<= u·2E): <= 4·E·u absolute,
  which exp turns into a relative error of w.  expf itself: the ROCm documentation on the machine this was written on states no
  ulp figure for expf, so 2 ulp = 4u is ASSUMED (the HIP math-API table published by AMD lists 1 ulp).  So every w carries a
  relative error rho <= (4·E + 4)·u.
* O: the numerator is a chain of d_i fmaf (<= d_i·u·Σ|w·z|) of terms each off by rho; den likewise (d_i·u + rho, relative); one
  division (u).  With Σ|w·z| / den <= max|Z[:,h,:]|:      |ΔO[i,h,:]| <= (2·d_i + 8·E + 10)·u·max|Z[:,h,:]|
  (the issue's shape (d_i + 2·max|e| + c): numerator and denominator each pay d_i and rho; c = 10 holds the 8 of the two expf
  assumptions, the division and one more for the second-order terms).  A long row is summed in another order (G strided
  partial sums): its constant is below d_i.
* α (backward, from the saved m and den): rho for w, d_i·u + rho for den, u for the division: rho_a(i) = (d_i + 8·E + 9)·u.
* dZ[j,h,:] = Σ_i α_ij·dO[i,h,:], dT_j slots of the transposed pattern in a chain of fmaf:
      |ΔdZ[j,h,:]| <= ((dT_j + 8·E + 10)·Σ_i α_ij,h + Σ_i α_ij,h·d_i)·u·max|dO[:,h,:]|
* g_ij = α·(t − D_i)·(1 or slope), t = <dO_i, Z_j>, D_i = <dO_i, O_i> over C channels; T = C·max|dO|·max|Z| bounds |t| and |D|.
  A dot of C terms (fmaf chain and butterfly) is off by <= (C + 1)·u·T, D also by C·max|dO|·|ΔO_i|; the subtraction adds u·2T,
  α's error rho_a(i)·2T, the two products 2u·2T:
      kappa(i,h) = (2·C + 8)·u·T + C·max|dO|·boundO(i,h) + rho_a(i)·2T          |Δg_ij| <= α_ij·kappa(i,h)
      |ΔdS_dst[i,h]| <= kappa(i,h) + d_i·u·2T                       (Σ_j α_ij = 1, |g_ij| <= α_ij·2T)
      |ΔdS_src[j,h]| <= Σ_i α_ij·kappa(i,h) + dT_j·u·2T·Σ_i α_ij
  The flag pre > 0 is the same in fp32 and fp64: rounding a sum keeps its sign.
"""
import torch

U = 2.0 ** -24
SLOPE = 0.2


def count_matrix(edge_index, num_nodes, add_self_loops=True):
    """cnt[i, j] = the slots of row i with source j, float64 [n, n]: the columns j -> i counted, self-loops replaced by one per
    node where the layer adds them."""
    ei = torch.as_tensor(edge_index).cpu().long()
    cnt = torch.zeros(num_nodes, num_nodes, dtype=torch.float64)
    for k in range(ei.shape[1]):
        cnt[int(ei[1, k]), int(ei[0, k])] += 1.0
    if add_self_loops:
        cnt.fill_diagonal_(1.0)
    return cnt


def attention(s_src, s_dst, cnt, slope=SLOPE):
    """α [H, n, n] (target, source) and pre [H, n, n], float64; rows without a slot are zero."""
    pre = s_dst.t()[:, :, None] + s_src.t()[:, None, :]
    e = torch.where(pre > 0, pre, slope * pre).masked_fill(cnt[None] == 0, float('-inf'))
    m = e.max(2, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    w = cnt[None] * torch.exp(e - m)
    den = w.sum(2, keepdim=True)
    return torch.where(den > 0, w / den.clamp(min=1e-300), torch.zeros_like(w)), pre


def aggregate(z, s_src, s_dst, cnt, slope=SLOPE):
    """O [n, H·C] in float64 from float64 operands (z [n, H·C], scores [n, H])."""
    n, heads = s_src.shape
    alpha, _ = attention(s_src, s_dst, cnt, slope)
    return torch.einsum('hij,jhc->ihc', alpha, z.reshape(n, heads, -1)).reshape(n, -1)


def aggregate_reference(z, s_src, s_dst, cnt, d_out, slope=SLOPE):
    """(O, dZ, dS_src, dS_dst) in float64 for the upstream gradient ``d_out``."""
    leaves = [t.detach().cpu().double().clone().requires_grad_(True) for t in (z, s_src, s_dst)]
    out = aggregate(*leaves, cnt, slope)
    out.backward(d_out.detach().cpu().double())
    return (out.detach(),) + tuple(t.grad for t in leaves)


def bounds(z, s_src, s_dst, cnt, d_out, slope=SLOPE):
    """The four bounds of the docstring, float64: 'O' and 'dZ' [n, H, 1] (one per head, for all its channels), 'dS_src' and
    'dS_dst' [n, H]."""
    z, s_src, s_dst, d_out = (t.detach().cpu().double() for t in (z, s_src, s_dst, d_out))
    n, heads = s_src.shape
    c = z.shape[1] // heads
    alpha, pre = attention(s_src, s_dst, cnt, slope)
    big_e = float(pre[(cnt[None] > 0).expand_as(pre)].abs().max()) if bool((cnt > 0).any()) else 0.0
    d = cnt.sum(1)                                        # slots per target row
    d_t = cnt.sum(0)                                      # slots per source row
    max_z = z.reshape(n, heads, c).abs().amax((0, 2))     # [H]
    max_g = d_out.reshape(n, heads, c).abs().amax((0, 2))
    b_o = (2 * d[:, None] + 8 * big_e + 10) * U * max_z[None, :]                       # [n, H]
    col_alpha = alpha.sum(1).t()                                                          # Σ_i α_ij,h  [n(j), H]
    b_dz = ((d_t[:, None] + 8 * big_e + 10) * col_alpha + torch.einsum('hij,i->jh', alpha, d)) * U * max_g[None, :]
    big_t = c * max_g * max_z                                                             # [H]
    rho_a = (d[:, None] + 8 * big_e + 9) * U                                              # [n, 1]
    kappa = (2 * c + 8) * U * big_t[None, :] + c * max_g[None, :] * b_o + rho_a * 2 * big_t[None, :]
    b_dst = kappa + d[:, None] * U * 2 * big_t[None, :]
    b_src = torch.einsum('hij,ih->jh', alpha, kappa) + d_t[:, None] * U * 2 * big_t[None, :] * col_alpha
    return {'O': b_o[:, :, None], 'dZ': b_dz[:, :, None], 'dS_src': b_src, 'dS_dst': b_dst}


def worst_ratio(got, want, bound):
    """max |got − want| / bound over the elements (0 / 0 counts as 0: an element whose bound is 0 must be exact)."""
    diff = (got.double() - want).abs().reshape(bound.shape[0], bound.shape[1], -1)
    b = bound.reshape(bound.shape[0], bound.shape[1], -1).expand_as(diff)
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / b)
    return float(ratio.max()) if ratio.numel() else 0.0


# ---- the fixtures of the random-float GPU tests (shared with the guard of tests/test_gat_cpu.py) ------------------------------
def _powerlaw(n, m, seed):
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(n, m, seed=seed)
    return torch.from_numpy(ei), n


def fixture(name):
    """(edge_index, n, H, C, add_self_loops, z, s_src, s_dst, d_out), fp32 on the CPU, the same values at every call.  Scores in
    ±2 (|pre| <= 4; one source of the hub fixture at 6), so that no weight of a row underflows and the guard of the CPU tests holds."""
    g = torch.Generator().manual_seed({'powerlaw': 11, 'hub': 12, 'all hubs': 13}[name])
    if name == 'powerlaw':          # a few hundred nodes; a duplicated column, an input self-loop, an isolated last node
        ei, n = _powerlaw(299, 3, 5)
        ei = torch.cat([ei, ei[:, :7], torch.tensor([[4, 4], [4, 4]])], 1)
        n, heads, c, loops = n + 1, 8, 8, True
    elif name == 'hub':             # node 0 receives from and sends to 530 nodes (above G·U = 512 slots at H x C = 2 x 8), on a ring
        n, heads, c, loops = 550, 2, 8, True
        ring = torch.arange(n)
        spokes = torch.arange(1, 531)
        zeros = torch.zeros(530, dtype=torch.int64)
        ei = torch.cat([torch.stack([ring, (ring + 1) % n]), torch.stack([spokes, zeros]), torch.stack([zeros, spokes])], 1)
    else:                           # every row above the long-row threshold, without added self-loops; 3 heads of 6 channels
        n, heads, c, loops = 130, 3, 6, False
        src = torch.arange(n).repeat_interleave(100)
        tgt = (src + 1 + torch.arange(100).repeat(n)) % n
        ei = torch.stack([src, tgt])
    z = torch.rand(n, heads * c, generator=g) * 2 - 1
    s_src = torch.rand(n, heads, generator=g) * 4 - 2
    s_dst = torch.rand(n, heads, generator=g) * 4 - 2
    d_out = torch.rand(n, heads * c, generator=g) * 2 - 1
    if name == 'hub':   # the hub's last source stands out (|pre| <= 8): the slot the guard drops carries about a third of the row
        s_src[n - 1] = 6.0
    return ei, n, heads, c, loops, z, s_src, s_dst, d_out


FIXTURES = ('powerlaw', 'hub', 'all hubs')


# ---- the dispatch of csrc/dcr_gat.hip (pick_lph_vec), restated, and the shapes the exact-value GPU test runs ----------------
LPHS = (4, 8, 16, 32, 64)


def vec_lph(c, lds=(), byte_offsets=()):
    """(VEC, LPH) for C channels per head: the widest VEC of 4, 2, 1 that C, every leading dimension and every pointer (its
    offset from a 16-byte boundary, in bytes) allow, then the first LPH that holds the C / VEC pieces; None above 64 pieces."""
    vec = next(v for v in (4, 2, 1) if c % v == 0 and all(ld % v == 0 for ld in lds) and all(o % (4 * v) == 0 for o in byte_offsets))
    return next(((vec, lph) for lph in LPHS if c // vec <= lph), None)


# the issue's grid, then one width per (VEC, LPH) pair the grid does not reach (contiguous operands: ld = H·C)
EXACT_SHAPES = [(h, c) for h in (1, 2, 3, 8) for c in (1, 2, 3, 4, 6, 8, 16, 64, 68)] + \
               [(2, c) for c in (5, 9, 17, 33, 10, 18, 34, 66, 32, 132)]


# ---- the whole model ----------------------------------------------------------------------------------------------------------
def logits(params, x, edge_index, num_nodes, configs):
    """log_softmax of the stacked layers in float64, ELU between them (dropout 0).  ``params``: one (weight [H·C, in], att_src,
    att_dst [1, H, C], bias) per layer; ``configs``: one (heads, concat, slope, add_self_loops) per layer."""
    h = x
    for i, ((weight, att_src, att_dst, bias), (heads, concat, slope, loops)) in enumerate(zip(params, configs)):
        cnt = count_matrix(edge_index, num_nodes, loops)
        n = h.shape[0]
        z = h @ weight.t()
        zh = z.reshape(n, heads, -1)
        out = aggregate(z, (zh * att_src).sum(-1), (zh * att_dst).sum(-1), cnt, slope).reshape(n, heads, -1)
        h = out.reshape(n, -1) if concat else out.mean(1)
        if bias is not None:
            h = h + bias
        if i < len(params) - 1:
            h = torch.nn.functional.elu(h)
    return torch.log_softmax(h, dim=1)


def model_reference(model, x, edge_index, y, mask):
    """(log-probabilities, {state-dict key: gradient}) in float64 of loss = nll_loss(log_probs[mask], y[mask]) for a
    models.gat.GAT: only its parameters' VALUES and its layers' settings are read."""
    leaves = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    params = [(leaves[f'layers.{i}.lin.weight'], leaves[f'layers.{i}.att_src'], leaves[f'layers.{i}.att_dst'],
               leaves.get(f'layers.{i}.bias')) for i in range(len(model.layers))]
    configs = [(conv.heads, conv.concat, conv.negative_slope, conv.add_self_loops) for conv in model.layers]
    lp = logits(params, x.detach().cpu().double(), edge_index, x.shape[0], configs)
    mask, y = torch.as_tensor(mask).cpu(), torch.as_tensor(y).cpu()
    torch.nn.functional.nll_loss(lp[mask], y[mask]).backward()
    return lp.detach(), {k: v.grad for k, v in leaves.items()}
