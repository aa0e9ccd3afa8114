"""GAT — the attention model of Veličković et al. as torch_geometric's ``GATConv`` evaluates it (third-party; restated here,
flow source -> target as ``GCNConv``), with ``GCN``'s call surface.  H heads, C channels per head:

    Z = X·W                                  [n, H·C]
    s_src[j,h] = <Z[j,h,:], att_src[h,:]>    s_dst[i,h] = <Z[i,h,:], att_dst[h,:]>
    pre_ij,h = s_src[j,h] + s_dst[i,h]       e_ij,h = pre > 0 ? pre : slope·pre
    α_ij,h = exp(e_ij,h − m_i,h) / den_i,h   m = max over the slots of row i, den = Σ exp(e − m) over them
    O[i,h,:] = Σ_slots α_ij,h · Z[j,h,:]

The slots of row i are the columns of ``edge_index`` with target i; with ``add_self_loops`` existing self-loops are removed and
one is added per node; a duplicated column is two slots, each with its own α; a row without slots gives O = 0 and zero
gradients.  The heads are concatenated (``concat=True``) or averaged, then the bias is added.

Evaluated as ONE GEMM X·[Wᵀ | Wᵀ·att_src | Wᵀ·att_dst] (Z and both scores) and ONE sweep of the CSR by target
(``dcr_gat_gather_f32_dev``, csrc/dcr_gat.hip); the backward pass is one sweep of the CSR of the transposed pattern between a
row-local kernel and a closing sum (``dcr_gat_expand_f32_dev``).  No floating-point atomics: two runs train the same weights.

Attention dropout (``attn_dropout = p``, in training): a keep weight k_ij,h in {0, 1 / (1 − p)} multiplies α AFTER the softmax, as
torch_geometric does, so m and den still run over every slot:  O[i,h,:] = Σ_slots k_ij,h·α_ij,h·Z[j,h,:].  No mask is stored: a
keep decision is a pure function of (seed, stream offset, slot position in the target CSR, head) in the Philox stream of the
GCN dropout kernels (include/dcr.h), and the forward sweep and the transposed sweep each draw it again
(``dcr_gat_gather_drop_f32_dev``, ``dcr_gat_expand_drop_f32_dev``).
"""
from typing import List

import torch
from torch.nn import ELU, Dropout, ModuleList, Parameter

from dcr import _lib
from models import gcn as _gcn
from models.gcn import _Linear, _stream, relu_dropout
from models.rgcn import _glorot_, _slot_rows

MAX_HEADS = 64   # (GAT_MAX_HEADS in csrc/dcr_gat.hip)


class AttnCSR:
    """The pattern by target row (``rowptr`` int64, ``col`` int32 sources), the same slots by source row (``rowptr_t``,
    ``col_t`` int32 targets) and the slot map ``slot_t`` (int64): the position in the target CSR of each slot of the source CSR.
    Inside a row of either the slots keep the order of ``edge_index``'s columns, an added self-loop last."""

    def __init__(self, rowptr, col, rowptr_t, col_t, slot_t, num_nodes, nnz=None):
        self.rowptr, self.col = rowptr, col
        self.rowptr_t, self.col_t, self.slot_t = rowptr_t, col_t, slot_t
        self.num_nodes = num_nodes
        self._nnz = nnz

    @property
    def nnz(self):
        """The number of slots, ``rowptr[n]``, as a host integer (read back once where the constructor was not given it)."""
        if self._nnz is None:
            self._nnz = int(self.rowptr[-1])
        return self._nnz


def _rowptr(row, n):
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=row.device)
    torch.cumsum(torch.bincount(row, minlength=n), 0, out=rowptr[1:])
    return rowptr


def gat_csr(edge_index, num_nodes, add_self_loops=True):
    """The ``AttnCSR`` of ``edge_index = [source; target]``, built with torch ops on the tensor's device.  Without a slot the
    slot arrays hold one unused entry, so that their device pointers are never null."""
    n = int(num_nodes)
    src, tgt = edge_index[0], edge_index[1]
    if add_self_loops:
        keep = src != tgt
        loops = torch.arange(n, dtype=src.dtype, device=src.device)
        src, tgt = torch.cat([src[keep], loops]), torch.cat([tgt[keep], loops])
    perm = torch.argsort(tgt, stable=True)
    src, tgt = src[perm], tgt[perm]                      # slot k of the target CSR: src[k] -> tgt[k]
    slot_t = torch.argsort(src, stable=True)             # slot k of the source CSR is slot slot_t[k] of the target CSR
    col, col_t = src.to(torch.int32), tgt[slot_t].to(torch.int32)
    if perm.numel() == 0:
        col, col_t, slot_t = col.new_zeros(1), col_t.new_zeros(1), slot_t.new_zeros(1)
    return AttnCSR(_rowptr(tgt, n), col.contiguous(), _rowptr(src, n), col_t.contiguous(), slot_t.contiguous(), n,
                   nnz=int(perm.numel()))


def _aggregate_torch(z, s_src, s_dst, csr, slope, keep=None, p=0.0, training=False):
    """The rule in plain differentiable torch ops, any float dtype: the chain of index_select, scatter-max, exp, scatter-add,
    divide and scatter-add (the maximum is a constant of the softmax, so it is detached).  ``keep`` [nnz, H], values 0 or
    1 / (1 − p) per (slot of the target CSR, head), multiplies α.  Without one, ``training`` and 0 < p < 1 draw it with
    ``torch.rand``: the same distribution as the HIP kernels' mask, NOT their Philox stream (two backends, two masks)."""
    n, heads = csr.num_nodes, s_src.shape[1]
    e_count = int(csr.rowptr[-1])
    rows, cols = _slot_rows(csr.rowptr), csr.col[:e_count].long()
    e = torch.nn.functional.leaky_relu(s_src[cols] + s_dst[rows], slope)
    m = torch.full((n, heads), float('-inf'), dtype=z.dtype, device=z.device)
    m = m.scatter_reduce(0, rows[:, None].expand(-1, heads), e.detach(), 'amax', include_self=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    w = torch.exp(e - m[rows])
    den = torch.zeros((n, heads), dtype=z.dtype, device=z.device).index_add(0, rows, w)
    alpha = w / den[rows]
    if keep is None and training and 0.0 < p < 1.0:
        keep = (torch.rand(alpha.shape, device=z.device) >= p).to(z.dtype) / (1.0 - p)
    if keep is not None:
        alpha = alpha * keep
    zh = z.reshape(n, heads, -1)
    out = torch.zeros_like(zh).index_add(0, rows, alpha[:, :, None] * zh[cols])
    return out.reshape(n, -1)


def _require_hip(t):
    if not t.is_cuda:
        raise RuntimeError('GAT aggregation runs on the MI355X HIP kernels: move the model and data to a ROCm device '
                           '(there is no CPU fallback)')
    if t.dtype != torch.float32:
        raise TypeError('dcr_gat_gather_f32_dev is fp32')


def _row_major(t):
    return t if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def _packed(z, s_src, s_dst):
    """Whether the three are column blocks of one row-major buffer (the one GEMM of ``GATConv``): (ld, column of each)."""
    ld = z.stride(0)
    if not (s_src.stride(0) == s_dst.stride(0) == ld and z.untyped_storage().data_ptr() == s_src.untyped_storage().data_ptr()
            == s_dst.untyped_storage().data_ptr()):
        return None
    cols = [t.storage_offset() - z.storage_offset() for t in (z, s_src, s_dst)]
    if cols[1] < z.shape[1] or cols[2] < cols[1] + s_src.shape[1] or cols[2] + s_dst.shape[1] > ld:
        return None
    return ld, cols


class _GatAggregate(torch.autograd.Function):
    """O = gather(Z, s_src, s_dst); (dZ, dS_src, dS_dst) = expand(dO) on the transposed pattern.  With 0 < p < 1 both take the
    attention-dropout entry points: seed ``torch.initial_seed()``, offset 0 plus the device's dropout call counter
    (``models.gcn._dropout_counter``, stepped after the launch as ``_ReluDropoutFn`` does); the one word the gather resolves
    the stream offset into is all the backward keeps of the mask."""

    @staticmethod
    def forward(ctx, z, s_src, s_dst, csr, slope, p=0.0):
        for t in (z, s_src, s_dst):
            _require_hip(t)
        z, s_src, s_dst = _row_major(z), _row_major(s_src), _row_major(s_dst)
        if s_src.stride(0) != s_dst.stride(0):
            s_src, s_dst = s_src.contiguous(), s_dst.contiguous()
        n, heads = csr.num_nodes, s_src.shape[1]
        if z.shape[0] != n or s_src.shape != (n, heads) or s_dst.shape != (n, heads) or heads < 1 or z.shape[1] % heads:
            raise ValueError(f'Z {tuple(z.shape)}, s_src {tuple(s_src.shape)}, s_dst {tuple(s_dst.shape)} for {n} nodes')
        out = torch.empty((n, z.shape[1]), dtype=torch.float32, device=z.device)
        rec = torch.empty((max(n * heads, 1), 2), dtype=torch.float32, device=z.device)
        args = (csr.rowptr.data_ptr(), csr.col.data_ptr(), z.data_ptr(), s_src.data_ptr(), s_dst.data_ptr(), out.data_ptr(),
                rec.data_ptr(), n, heads, z.shape[1] // heads, z.stride(0), s_src.stride(0), out.stride(0), float(slope), _stream(z))
        ctx.p, ctx.seed, ctx.offset_used = float(p), 0, None
        if ctx.p > 0.0:
            ctr = _gcn._dropout_counter(z.device)
            ctx.seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
            ctx.offset_used = torch.empty(1, dtype=torch.int64, device=z.device)
            _lib.check(_lib.lib().dcr_gat_gather_drop_f32_dev(*args, csr.nnz, ctx.p, ctx.seed, 0, ctr.data_ptr(),
                                                              ctx.offset_used.data_ptr()))
            ctr.add_(1)
        else:
            _lib.check(_lib.lib().dcr_gat_gather_f32_dev(*args))
        ctx.save_for_backward(z, s_src, s_dst, out, rec)
        ctx.csr, ctx.slope = csr, float(slope)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        z, s_src, s_dst, out, rec = ctx.saved_tensors
        csr = ctx.csr
        n, heads, width = csr.num_nodes, s_src.shape[1], z.shape[1]
        grad_out = grad_out.contiguous()
        packed = _packed(z, s_src, s_dst)
        if packed:   # one gradient buffer laid out as the operand: the slices autograd joins are its column blocks
            ld, cols = packed
            buf = torch.empty((n, ld), dtype=torch.float32, device=z.device)
            dz, ds_src, ds_dst = buf[:, :width], buf[:, cols[1]:cols[1] + heads], buf[:, cols[2]:cols[2] + heads]
        else:        # (every element the kernels are asked for is written)
            dz = torch.empty((n, z.stride(0)), dtype=torch.float32, device=z.device)[:, :width]
            ds_src = torch.empty((n, s_src.stride(0)), dtype=torch.float32, device=z.device)[:, :heads]
            ds_dst = torch.empty((n, s_src.stride(0)), dtype=torch.float32, device=z.device)[:, :heads]
        work_rec = torch.empty((max(n * heads, 1), 4), dtype=torch.float32, device=z.device)
        work_g = torch.empty(max(int(csr.col_t.numel()) * heads, 1), dtype=torch.float32, device=z.device)
        args = (csr.rowptr.data_ptr(), csr.rowptr_t.data_ptr(), csr.col_t.data_ptr(), csr.slot_t.data_ptr(), z.data_ptr(),
                s_src.data_ptr(), s_dst.data_ptr(), out.data_ptr(), grad_out.data_ptr(), rec.data_ptr(), dz.data_ptr(),
                ds_src.data_ptr(), ds_dst.data_ptr(), work_rec.data_ptr(), work_g.data_ptr(), n, heads, width // heads, z.stride(0),
                s_src.stride(0), width, ctx.slope, _stream(z))
        if ctx.p > 0.0:
            _lib.check(_lib.lib().dcr_gat_expand_drop_f32_dev(*args, csr.nnz, ctx.p, ctx.seed, ctx.offset_used.data_ptr()))
        else:
            _lib.check(_lib.lib().dcr_gat_expand_f32_dev(*args))
        return dz, ds_src, ds_dst, None, None, None


def gat_aggregate(z, s_src, s_dst, csr, negative_slope=0.2, attn_dropout=0.0, training=False):
    """O [n, H·C] of the rule above from Z [n, H·C] and the scores [n, H] each, differentiable in all three.  On the 'hip'
    backend (``models.gcn.set_aggregate_backend``) the kernels of csrc/dcr_gat.hip, and a CPU tensor raises; 'torch' is the
    plain-torch path of the CPU tests (any float dtype), never chosen automatically.  ``attn_dropout`` in [0, 1) acts only
    with ``training``: on 'hip' the kernels redraw the mask from the Philox stream in both passes, on 'torch' the mask comes
    from ``torch.rand`` (another stream, the same distribution)."""
    p = float(attn_dropout)
    if not 0.0 <= p < 1.0:
        raise ValueError(f'attn_dropout must be in [0, 1), got {attn_dropout}')
    if not training:
        p = 0.0
    if _gcn._AGG_BACKEND == 'hip':
        return _GatAggregate.apply(z, s_src, s_dst, csr, negative_slope, p)
    return _aggregate_torch(z, s_src, s_dst, csr, negative_slope, p=p, training=training)


class GATConv(torch.nn.Module):
    """One attention layer.  Parameters: ``lin.weight`` [H·C, in] (glorot), ``att_src`` and ``att_dst`` [1, H, C] (glorot),
    ``bias`` [H·C], or [C] with ``concat=False`` (zeros).  These are torch_geometric's names and shapes as far as they are
    known here; torch_geometric is not installed where this was written, so the interchange of state dicts was NOT checked.
    Dropout on the attention coefficients is ``attn_dropout`` (in training, after the softmax, as torch_geometric's
    ``dropout``); the keyword ``dropout`` itself is not taken and a non-zero value raises.  ``edge_attr`` is not read: the
    layer's own learned weights take the place of edge weights."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 bias=True, attn_dropout=0.0):
        super().__init__()
        if dropout != 0.0:
            raise NotImplementedError('GATConv: dropout on the attention coefficients is the keyword attn_dropout '
                                      '(dropout= is not taken here; dropout between the layers is GAT\'s own argument)')
        if not 0.0 <= float(attn_dropout) < 1.0:
            raise ValueError(f'attn_dropout must be in [0, 1), got {attn_dropout}')
        self.attn_dropout = float(attn_dropout)
        if not 1 <= int(heads) <= MAX_HEADS:
            raise ValueError(f'heads must be in [1, {MAX_HEADS}], got {heads}')
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, int(heads)
        self.concat, self.negative_slope, self.add_self_loops = bool(concat), float(negative_slope), bool(add_self_loops)
        self.lin = _Linear(in_channels, self.heads * out_channels)
        self.att_src = Parameter(torch.empty(1, self.heads, out_channels))
        self.att_dst = Parameter(torch.empty(1, self.heads, out_channels))
        if bias:
            self.bias = Parameter(torch.zeros(self.heads * out_channels if self.concat else out_channels))
        else:
            self.register_parameter('bias', None)
        self._cache_key = self._cache_csr = self._cache_ref = None
        self.reset_parameters()

    def reset_parameters(self):
        self.lin.reset_parameters()
        _glorot_(self.att_src)
        _glorot_(self.att_dst)
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()
        self.invalidate()

    def invalidate(self):
        """Drop the cached ``AttnCSR`` (it is rebuilt at the next forward)."""
        self._cache_key = self._cache_csr = self._cache_ref = None

    def attn_csr(self, edge_index, num_nodes):
        # (keyed on the tensor's storage and version, and the tensor is held, as GCNConv.norm_csr does)
        key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), tuple(edge_index.stride()), int(num_nodes),
               str(edge_index.device))
        if key != self._cache_key:
            self._cache_csr = gat_csr(edge_index, num_nodes, self.add_self_loops)
            self._cache_key = key
            self._cache_ref = edge_index
        return self._cache_csr

    def operand(self):
        """[Wᵀ | Wᵀ·att_src | Wᵀ·att_dst | 0], [in, H·C + 2·H (+ pad to a multiple of 4)]: Z and both scores from one GEMM, and
        autograd carries the scores' gradients to ``att_*`` and ``lin.weight``."""
        h, c = self.heads, self.out_channels
        w = self.lin.weight
        wh = w.view(h, c, self.in_channels)
        parts = [w.t(), (wh * self.att_src.view(h, c, 1)).sum(1).t(), (wh * self.att_dst.view(h, c, 1)).sum(1).t()]
        pad = -(h * c + 2 * h) % 4
        if pad:
            parts.append(w.new_zeros((self.in_channels, pad)))
        return torch.cat(parts, 1)

    def forward(self, x, edge_index, edge_attr=None):
        h, c = self.heads, self.out_channels
        csr = self.attn_csr(edge_index, x.shape[0])
        zs = x @ self.operand()
        out = gat_aggregate(zs[:, :h * c], zs[:, h * c:h * c + h], zs[:, h * c + h:h * c + 2 * h], csr, self.negative_slope,
                            self.attn_dropout, self.training)
        if not self.concat:
            out = out.view(-1, h, c).mean(1)
        return out if self.bias is None else out + self.bias


class GAT(torch.nn.Module):
    """``GCN``'s surface (models/gcn.py) on ``GATConv`` layers: ``heads`` heads of each hidden width, concatenated, ELU and
    dropout between the layers; the last layer has ``output_heads`` heads, averaged.  The paper's two other dropouts are
    off by default: ``attn_dropout`` on the attention coefficients of every layer, ``input_dropout`` (a stock
    ``torch.nn.Dropout``) on the input features before the first layer; the paper trains with 0.6 for both.  Weight decay on
    the first layer only."""

    def __init__(self, dataset, hidden: List[int] = [8], heads: int = 8, output_heads: int = 1, dropout: float = 0.6,
                 attn_dropout: float = 0.0, input_dropout: float = 0.0):
        super().__init__()
        widths = [dataset.data.x.shape[1], *[w * heads for w in hidden]]
        layers = [GATConv(w_in, w_out, heads=heads, attn_dropout=attn_dropout) for w_in, w_out in zip(widths, hidden)]
        layers.append(GATConv(widths[-1], dataset.num_classes, heads=output_heads, concat=False, attn_dropout=attn_dropout))
        self.layers = ModuleList(layers)
        self.reg_params = list(self.layers[0].parameters())
        self.non_reg_params = [p for conv in list(self.layers)[1:] for p in conv.parameters()]
        self.dropout = Dropout(p=dropout)
        self.input_dropout = Dropout(p=input_dropout)
        self.act_fn = ELU()

    def reset_parameters(self):
        for conv in self.layers:
            conv.reset_parameters()

    def forward(self, data):
        x = data.x
        if self.input_dropout.p > 0.0:
            x = self.input_dropout(x)
        for i, conv in enumerate(self.layers):
            x = conv(x, data.edge_index)
            if i < len(self.layers) - 1:
                x = relu_dropout(x, self.act_fn, self.dropout)   # (ELU: the stock-module branch)
        return torch.nn.functional.log_softmax(x, dim=1)


def dense_reference_logits(model, x, edge_index, num_nodes):
    """Dense fp64 restatement of ``model`` in evaluation mode: the n x n matrix of column counts (self-loops replaced where the
    layer adds them), a masked softmax per head with a duplicated column weighted by its count, ELU between the layers — the
    build's own pin for GATConv."""
    n = num_nodes
    cnt = torch.zeros((n, n), dtype=torch.float64, device=x.device)
    cnt.index_put_((edge_index[1], edge_index[0]), torch.ones(edge_index.shape[1], dtype=torch.float64, device=x.device),
                   accumulate=True)
    h = x.double()
    for i, conv in enumerate(model.layers):
        a = cnt
        if conv.add_self_loops:
            a = cnt.clone()
            a.fill_diagonal_(1.0)
        heads, c = conv.heads, conv.out_channels
        z = (h @ conv.lin.weight.double().t()).view(n, heads, c)
        s_src, s_dst = (z * conv.att_src.double()).sum(-1), (z * conv.att_dst.double()).sum(-1)
        e = torch.nn.functional.leaky_relu(s_dst.t()[:, :, None] + s_src.t()[:, None, :], conv.negative_slope)   # [H, i, j]
        e = e.masked_fill(a[None] == 0, float('-inf'))
        m = e.max(2, keepdim=True).values
        w = a[None] * torch.exp(e - torch.where(torch.isinf(m), torch.zeros_like(m), m))
        alpha = w / w.sum(2, keepdim=True).clamp(min=1e-300)
        out = torch.einsum('hij,jhc->ihc', alpha, z)
        h = out.reshape(n, heads * c) if conv.concat else out.mean(1)
        if conv.bias is not None:
            h = h + conv.bias.double()
        if i < len(model.layers) - 1:
            h = torch.nn.functional.elu(h)
    return torch.log_softmax(h, dim=1)


def smoke_gat(edge_index, num_nodes, device='cuda:0'):
    from dcr.data import Data, Dataset
    torch.manual_seed(0)
    x = torch.randn(num_nodes, 32)
    y = torch.randint(0, 5, (num_nodes,))
    data = Data(x=x, edge_index=edge_index, y=y, num_nodes=num_nodes).to(device)
    model = GAT(Dataset(data, 5), hidden=[8], heads=8, dropout=0.6).to(device)
    model.eval()
    with torch.no_grad():
        got = model(data)
        want = dense_reference_logits(model, data.x, data.edge_index, num_nodes)
    err = (got.double() - want).abs().max().item()
    assert err < 1e-4, f'GAT logits differ from the dense reference by {err}'
    model.train()
    torch.nn.functional.nll_loss(model(data), data.y).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    return err
