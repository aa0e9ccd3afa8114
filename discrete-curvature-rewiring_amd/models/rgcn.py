"""R-GCN on typed edges — the relational model FoSR's ``edge_type`` is made for (rewiring/fosr.py: 0 on the input's entries,
1 on the added ones), with ``GCN``'s call surface.

The layer is Schlichtkrull et al. eq. 2 with c_{i,r} = |N_r(i)|, torch_geometric's ``RGCNConv`` with ``aggr='mean'``
(third-party; restated here, flow source -> target as ``GCNConv``):

    out_i = x_i·W_root + b + Σ_r (1/|N_r(i)|) Σ_{(j->i) of type r} x_j·W_r

|N_r(i)| counts the columns of ``edge_index`` with target i and type r: a duplicated column counts twice, a self-loop is an
ordinary edge of its type, a relation with no edge into i contributes nothing.  Parameters carry torch_geometric's names and
shapes (``weight`` [R, in, out], ``root`` [in, out], ``bias`` [out]), so state dicts interchange.

Evaluated transform-first: ONE GEMM gives Zall = X·[W_0 | … | W_{R-1} | W_root] and ONE sweep of a typed CSR forms the output
(``dcr_spmm_csr_typed_f32_dev``, csrc/dcr_spmm.hip); the backward pass forms the whole of dZall in one sweep of the CSR of the
transposed pattern (``dcr_spmm_csr_typed_expand_f32_dev``).  The dense products go through the GEMM library.
"""
from typing import List

import torch
from torch.nn import Dropout, ModuleList, Parameter, ReLU

from dcr import _lib
from models import gcn as _gcn
from models.gcn import _ptr, _stream, relu_dropout

MAX_RELATIONS = 8   # (SPMM_MAX_REL in csrc/dcr_spmm.hip)


class TypedCSR:
    """The typed pattern by target row (``rowptr`` int64, ``col`` int32 sources, ``val`` float32 = 1/|N_r(i)|, ``rel`` uint8) and
    the same edges by source row (``*_t``: ``col_t`` the targets, the same ``val`` and ``rel`` per edge).  Inside a row of
    either the slots are sorted by relation, stably within one: the kernels rely on it."""

    def __init__(self, rowptr, col, val, rel, rowptr_t, col_t, val_t, rel_t, num_nodes, num_relations):
        self.rowptr, self.col, self.val, self.rel = rowptr, col, val, rel
        self.rowptr_t, self.col_t, self.val_t, self.rel_t = rowptr_t, col_t, val_t, rel_t
        self.num_nodes, self.num_relations = num_nodes, num_relations


def _typed_csr_from_coo(row, other, et, val, n, n_rel):
    """CSR by ``row`` with the slots of a row sorted by relation, stably within one.  Without an edge the three slot arrays hold
    one unused entry, so that their device pointers are never null."""
    perm = torch.argsort(row * n_rel + et, stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=row.device)
    torch.cumsum(torch.bincount(row, minlength=n), 0, out=rowptr[1:])
    col, v, rel = other[perm].to(torch.int32), val[perm], et[perm].to(torch.uint8)
    if perm.numel() == 0:
        col, v, rel = col.new_zeros(1), v.new_zeros(1), rel.new_zeros(1)
    return rowptr, col.contiguous(), v.contiguous(), rel.contiguous()


def rgcn_norm_csr(edge_index, edge_type, num_nodes, num_relations):
    """The ``TypedCSR`` of ``edge_index = [source; target]`` with one ``edge_type`` in [0, num_relations) per column, built with
    torch ops on the tensors' device (one host sync, for the range check)."""
    n, n_rel = int(num_nodes), int(num_relations)
    if not 1 <= n_rel <= MAX_RELATIONS:
        raise ValueError(f'num_relations must be in [1, {MAX_RELATIONS}], got {n_rel}')
    if edge_type.dim() != 1 or edge_type.shape[0] != edge_index.shape[1]:
        raise ValueError(f'edge_type of shape {tuple(edge_type.shape)} for {edge_index.shape[1]} edges')
    if edge_type.dtype != torch.int64:
        raise TypeError('edge_type must be int64')
    src, tgt = edge_index[0], edge_index[1]
    if edge_type.numel():
        lo, hi = int(edge_type.min()), int(edge_type.max())
        if lo < 0 or hi >= n_rel:
            raise ValueError(f'edge_type outside [0, {n_rel}): [{lo}, {hi}]')
    key = tgt * n_rel + edge_type
    count = torch.bincount(key, minlength=n * n_rel)              # |N_r(i)| at i * R + r, duplicates counted
    val = count.to(torch.float32).reciprocal()[key]
    fwd = _typed_csr_from_coo(tgt, src, edge_type, val, n, n_rel)
    bwd = _typed_csr_from_coo(src, tgt, edge_type, val, n, n_rel)
    return TypedCSR(*fwd, *bwd, n, n_rel)


def _width(zall_cols, n_rel, self_block):
    blocks = n_rel + int(self_block)
    if zall_cols % blocks:
        raise ValueError(f'{zall_cols} columns are not {blocks} blocks of one width')
    return zall_cols // blocks


def _require_hip(t, name):
    if not t.is_cuda:
        raise RuntimeError('R-GCN aggregation runs on the MI355X HIP kernel: move the model and data to a ROCm device '
                           '(there is no CPU fallback)')
    if t.dtype != torch.float32:
        raise TypeError(name + ' is fp32')


def _gather_hip(csr, zall, bias, self_block):
    _require_hip(zall, 'dcr_spmm_csr_typed_f32_dev')
    zall = zall.contiguous()
    f = _width(zall.shape[1], csr.num_relations, self_block)
    out = torch.empty((csr.num_nodes, f), dtype=torch.float32, device=zall.device)
    _lib.check(_lib.lib().dcr_spmm_csr_typed_f32_dev(csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(), csr.rel.data_ptr(),
                                                     zall.data_ptr(), out.data_ptr(), csr.num_nodes, f, csr.num_relations,
                                                     zall.shape[1], f, int(self_block), _ptr(bias), 0, _stream(zall)))
    return out


def _expand_hip(csr, grad, self_block):
    _require_hip(grad, 'dcr_spmm_csr_typed_expand_f32_dev')
    grad = grad.contiguous()
    f = grad.shape[1]
    wide = (csr.num_relations + int(self_block)) * f
    out = torch.empty((csr.num_nodes, wide), dtype=torch.float32, device=grad.device)   # (every element is written)
    _lib.check(_lib.lib().dcr_spmm_csr_typed_expand_f32_dev(csr.rowptr_t.data_ptr(), csr.col_t.data_ptr(), csr.val_t.data_ptr(),
                                                            csr.rel_t.data_ptr(), grad.data_ptr(), out.data_ptr(), csr.num_nodes,
                                                            f, csr.num_relations, f, wide, int(self_block), _stream(grad)))
    return out


def _slot_rows(rowptr):
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=rowptr.device), rowptr[1:] - rowptr[:-1])


def _gather_torch(csr, zall, bias, self_block):
    n, r = csr.num_nodes, csr.num_relations
    e = int(csr.rowptr[-1])
    blocks = zall.reshape(n, r + int(self_block), -1)
    out = blocks[:, r].clone() if self_block else zall.new_zeros((n, blocks.shape[2]))
    out.index_add_(0, _slot_rows(csr.rowptr), blocks[csr.col[:e].long(), csr.rel[:e].long()] * csr.val[:e, None].to(zall.dtype))
    return out if bias is None else out + bias


def _expand_torch(csr, grad, self_block):
    n, r = csr.num_nodes, csr.num_relations
    e = int(csr.rowptr_t[-1])
    out = grad.new_zeros((n, r + int(self_block), grad.shape[1]))
    out.index_put_((_slot_rows(csr.rowptr_t), csr.rel_t[:e].long()), grad[csr.col_t[:e].long()] * csr.val_t[:e, None].to(grad.dtype),
                   accumulate=True)
    if self_block:
        out[:, r] = grad
    return out.reshape(n, -1)


class _TypedAggregate(torch.autograd.Function):
    """out = gather(Zall) + b ; dZall = expand(dout) on the transposed pattern ; db = Σ_rows dout."""

    @staticmethod
    def forward(ctx, zall, bias, csr, self_block):
        ctx.csr, ctx.self_block, ctx.has_bias = csr, self_block, bias is not None
        fn = _gather_hip if _gcn._AGG_BACKEND == 'hip' else _gather_torch
        return fn(csr, zall, bias, self_block)

    @staticmethod
    def backward(ctx, grad_out):
        need = ctx.needs_input_grad
        gz = gb = None
        if need[0]:
            fn = _expand_hip if _gcn._AGG_BACKEND == 'hip' else _expand_torch
            gz = fn(ctx.csr, grad_out, ctx.self_block)
        if ctx.has_bias and need[1]:
            gb = grad_out.sum(0)
        return gz, gb, None, None


def typed_aggregate(zall, bias, csr, self_block=True):
    """The R-GCN aggregation of Zall = [Z_0 | … | Z_{R-1} | Z_root] (``self_block=False``: no root block) over ``csr``:
    out_i = Z_root[i] + Σ_slots val·Z_rel[col] + bias.  On the 'hip' backend (``models.gcn.set_aggregate_backend``) the two
    kernels of csrc/dcr_spmm.hip, and a CPU tensor raises; 'torch' is the plain-torch path of the CPU tests, never chosen
    automatically."""
    return _TypedAggregate.apply(zall, bias, csr, bool(self_block))


def _glorot_(t):
    """torch_geometric's ``glorot``: uniform in ±sqrt(6 / (size(-2) + size(-1))), so per relation for ``weight``."""
    a = (6.0 / (t.shape[-2] + t.shape[-1])) ** 0.5
    with torch.no_grad():
        t.uniform_(-a, a)


class RGCNConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, num_relations, root_weight=True, bias=True):
        super().__init__()
        if not 1 <= int(num_relations) <= MAX_RELATIONS:
            raise ValueError(f'num_relations must be in [1, {MAX_RELATIONS}], got {num_relations}')
        self.in_channels, self.out_channels, self.num_relations = in_channels, out_channels, int(num_relations)
        self.weight = Parameter(torch.empty(self.num_relations, in_channels, out_channels))
        if root_weight:
            self.root = Parameter(torch.empty(in_channels, out_channels))
        else:
            self.register_parameter('root', None)
        if bias:
            self.bias = Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter('bias', None)
        self._cache_key = self._cache_csr = self._cache_ref = None
        self.reset_parameters()

    def reset_parameters(self):
        _glorot_(self.weight)
        if self.root is not None:
            _glorot_(self.root)
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()
        self.invalidate()

    def invalidate(self):
        """Drop the cached ``TypedCSR`` (it is rebuilt at the next forward)."""
        self._cache_key = self._cache_csr = self._cache_ref = None

    def typed_csr(self, edge_index, edge_type, num_nodes):
        # (keyed on the two tensors' storage and version, and the tensors are held, as GCNConv.norm_csr does: an equal key
        #  always means the same values)
        key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), tuple(edge_index.stride()),
               edge_type.data_ptr(), edge_type._version, tuple(edge_type.shape), int(num_nodes), str(edge_index.device))
        if key != self._cache_key:
            self._cache_csr = rgcn_norm_csr(edge_index, edge_type, num_nodes, self.num_relations)
            self._cache_key = key
            self._cache_ref = (edge_index, edge_type)
        return self._cache_csr

    def forward(self, x, edge_index, edge_type):
        csr = self.typed_csr(edge_index, edge_type, x.shape[0])
        # [W_0 | … | W_{R-1} | W_root], [in, (R + 1)·out]: one GEMM for every relation and the root
        w = self.weight.permute(1, 0, 2).reshape(self.in_channels, self.num_relations * self.out_channels)
        if self.root is not None:
            w = torch.cat([w, self.root], 1)
        return typed_aggregate(x @ w, self.bias, csr, self.root is not None)


class RGCN(torch.nn.Module):
    """``GCN``'s surface (models/gcn.py) on ``RGCNConv`` layers of widths [features] + hidden + [classes]: ReLU and dropout
    between them, log-softmax at the end, weight decay on the first layer only.  ``forward`` reads ``data.edge_type``."""

    def __init__(self, dataset, num_relations: int = 2, hidden: List[int] = [64], dropout: float = 0.5):
        super().__init__()
        widths = [dataset.data.x.shape[1], *hidden, dataset.num_classes]
        self.layers = ModuleList([RGCNConv(w_in, w_out, num_relations) for w_in, w_out in zip(widths, widths[1:])])
        self.reg_params = list(self.layers[0].parameters())
        self.non_reg_params = [p for conv in list(self.layers)[1:] for p in conv.parameters()]
        self.dropout = Dropout(p=dropout)
        self.act_fn = ReLU()

    def reset_parameters(self):
        for conv in self.layers:
            conv.reset_parameters()

    def forward(self, data):
        edge_type = getattr(data, 'edge_type', None)
        if edge_type is None:
            raise ValueError('RGCN reads data.edge_type (int64, one relation id per column of data.edge_index; '
                             'rewiring.fosr.fosr returns it): this data has none')
        x = data.x
        for i, conv in enumerate(self.layers):
            x = conv(x, data.edge_index, edge_type)
            if i < len(self.layers) - 1:
                x = relu_dropout(x, self.act_fn, self.dropout)
        return torch.nn.functional.log_softmax(x, dim=1)


def dense_reference_logits(model, x, edge_index, edge_type, num_nodes):
    """Dense fp64 restatement of ``model`` in evaluation mode: per relation the n x n matrix of column counts divided by its row
    sums, log_softmax(Σ_r M_r·(H·W_r) + H·W_root + b) with ReLU between the layers — the build's own pin for RGCNConv."""
    n, n_rel = num_nodes, model.layers[0].num_relations
    M = torch.zeros((n_rel, n, n), dtype=torch.float64, device=x.device)
    M.index_put_((edge_type, edge_index[1], edge_index[0]), torch.ones(edge_type.shape[0], dtype=torch.float64, device=x.device),
                 accumulate=True)
    M = M / M.sum(2, keepdim=True).clamp(min=1.0)
    h = x.double()
    for i, conv in enumerate(model.layers):
        h = sum(M[r] @ (h @ conv.weight[r].double()) for r in range(n_rel)) + h @ conv.root.double() + conv.bias.double()
        if i < len(model.layers) - 1:
            h = torch.relu(h)
    return torch.log_softmax(h, dim=1)


def smoke_rgcn(edge_index, num_nodes, device='cuda:0'):
    from dcr.data import Data, Dataset
    torch.manual_seed(0)
    x = torch.randn(num_nodes, 32)
    y = torch.randint(0, 5, (num_nodes,))
    edge_type = torch.arange(edge_index.shape[1]) % 2
    data = Data(x=x, edge_index=edge_index, y=y, num_nodes=num_nodes, edge_type=edge_type).to(device)
    model = RGCN(Dataset(data, 5), num_relations=2, hidden=[16], dropout=0.5).to(device)
    model.eval()
    with torch.no_grad():
        got = model(data)
        want = dense_reference_logits(model, data.x, data.edge_index, data.edge_type, num_nodes)
    err = (got.double() - want).abs().max().item()
    assert err < 1e-5, f'RGCN logits differ from the dense reference by {err}'
    model.train()
    torch.nn.functional.nll_loss(model(data), data.y).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    return err
