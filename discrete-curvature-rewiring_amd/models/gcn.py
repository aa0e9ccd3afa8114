"""GCN — call surface of the reference's models/gcn.py:12-44.

``GCN(dataset, hidden=[64], dropout=0.5)`` with ``.layers`` (a ModuleList of
GCNConv), ``.reg_params`` / ``.non_reg_params`` (gcn.py:22-23),
``.reset_parameters()`` and ``.forward(data) -> log_softmax [N, C]``.

``GCNConv`` restates torch_geometric 2.0.3's layer (third-party, not vendored
by the reference; call sites gcn.py:19,30,36): ``gcn_norm`` with self loops,
``lin`` = bias-free Linear with glorot init (state_dict key ``lin.weight``
[out, in]), aggregation at the target node, ``bias`` added after aggregation
(state_dict key ``bias``).  The dense contraction X·Wᵀ runs on the matrix cores
through the ROCm GEMM library; the sparse aggregation Â·(XWᵀ) + b is the
hand-written HIP kernel ``dcr_spmm_csr_f32_dev`` (csrc/dcr_spmm.hip), wrapped in
an autograd Function whose backward is the same kernel on Âᵀ.
"""
import ctypes
import os
import math
from typing import List

import torch
from torch.nn import Dropout, ModuleList, Parameter, ReLU

from dcr import _lib   # (the loader only: the library itself is opened at the first call of _lib.lib())

# 'hip': the product path (ROCm tensors only, raises otherwise).
# 'torch': plain-torch aggregation; selected explicitly by CPU-only tests (gloo) — never automatically.
_AGG_BACKEND = 'hip'


def set_aggregate_backend(name):
    global _AGG_BACKEND
    if name not in ('hip', 'torch'):
        raise ValueError(name)
    _AGG_BACKEND = name


def _stream(t):
    """The current stream of ``t``'s device, as the kernels' stream argument."""
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


class NormCSR:
    """Â = D^-1/2 (A + I) D^-1/2 as CSR by target row, plus the CSR of Âᵀ for the backward pass."""

    def __init__(self, rowptr, col, val, rowptr_t, col_t, val_t, n_rows, n_cols):
        self.rowptr, self.col, self.val = rowptr, col, val
        self.rowptr_t, self.col_t, self.val_t = rowptr_t, col_t, val_t
        self.n_rows, self.n_cols = n_rows, n_cols


def _csr_from_coo(target, source, w, n_rows):
    perm = torch.argsort(target, stable=True)
    counts = torch.bincount(target, minlength=n_rows)
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=target.device)
    torch.cumsum(counts, 0, out=rowptr[1:])
    return rowptr, source[perm].to(torch.int32).contiguous(), w[perm].contiguous()


def _weighted_degree(source, target, w, n):
    """deg = scatter_add(w, target), float32, the same bits on every run.  On the GPU a scatter of float32 atomics adds in the
    order the threads arrive: weights that are not small integers then gave another Â, and other trained weights, from one
    run to the next.  There the weights are grouped by target (the CSR of Â's pattern) and each row is summed by the
    aggregation kernel against a column of ones, which adds a row's entries in a fixed order (csrc/dcr_spmm.hip, k_spmm_csr).
    Unit weights give exact integer sums either way, the degrees of the published formula.  On the CPU, ``scatter_add_``
    adds in index order."""
    if _AGG_BACKEND == 'hip' and w.is_cuda:
        rowptr, cols, vals = _csr_from_coo(target, source, w, n)
        return _spmm_hip(rowptr, cols, vals, torch.ones((n, 1), dtype=torch.float32, device=w.device), n)[:, 0]
    return torch.zeros(n, dtype=torch.float32, device=w.device).scatter_add_(0, target, w)


def gcn_norm_csr(edge_index, edge_weight=None, num_nodes=None, add_self_loops=True, row_range=None):
    """PyG 2.0.3 ``gcn_norm`` (flow source_to_target): weights 1 if None;
    ``add_remaining_self_loops(fill_value=1)``; deg = scatter_add(w, target);
    norm = deg^-1/2[source] * w * deg^-1/2[target] (inf -> 0).

    ``row_range=(r0, r1)`` keeps only target rows r0..r1-1 (row-partitioned Â for data parallelism);
    normalisation always uses the full graph's degrees.
    """
    row, col = edge_index[0], edge_index[1]
    n = int(num_nodes)
    dev = edge_index.device
    w = torch.ones(row.shape[0], dtype=torch.float32, device=dev) if edge_weight is None else edge_weight.float()
    if add_self_loops:
        keep = row != col
        loop_w = torch.ones(n, dtype=torch.float32, device=dev)
        if (~keep).any():
            loop_w[row[~keep]] = w[~keep]
        ar = torch.arange(n, dtype=row.dtype, device=dev)
        row = torch.cat([row[keep], ar])
        col = torch.cat([col[keep], ar])
        w = torch.cat([w[keep], loop_w])
    deg = _weighted_degree(row, col, w, n)
    dinv = deg.pow(-0.5)
    dinv[torch.isinf(dinv)] = 0
    norm = dinv[row] * w * dinv[col]
    if row_range is not None:
        r0, r1 = row_range
        sel = (col >= r0) & (col < r1)
        row, col, norm = row[sel], col[sel] - r0, norm[sel]
        n_rows = r1 - r0
    else:
        n_rows = n
    rowptr, cidx, val = _csr_from_coo(col, row, norm, n_rows)          # Â: rows = targets
    rowptr_t, cidx_t, val_t = _csr_from_coo(row, col, norm, n)          # Âᵀ: rows = sources
    return NormCSR(rowptr, cidx, val, rowptr_t, cidx_t, val_t, n_rows, n)


def _spmm_hip(rowptr, col, val, B, n_rows, bias=None, relu=False):
    if not B.is_cuda:
        raise RuntimeError('GCN aggregation runs on the MI355X HIP kernel: move the model and data to a ROCm '
                           'device (there is no CPU fallback)')
    B = B.contiguous()
    if B.dtype != torch.float32:
        raise TypeError('dcr_spmm_csr_f32_dev is fp32')
    F = B.shape[1]
    C = torch.empty((n_rows, F), dtype=torch.float32, device=B.device)
    _lib.check(_lib.lib().dcr_spmm_csr_f32_dev(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), B.data_ptr(), C.data_ptr(),
                                               n_rows, F, F, F, _ptr(bias), int(relu), _stream(B)))
    return C


def _spmm_torch(rowptr, col, val, B, n_rows, bias=None, relu=False):
    counts = rowptr[1:] - rowptr[:-1]
    tgt = torch.repeat_interleave(torch.arange(n_rows, device=B.device), counts)
    out = torch.zeros((n_rows, B.shape[1]), dtype=B.dtype, device=B.device)
    out.index_add_(0, tgt, B[col.long()] * val[:, None])
    if bias is not None:
        out = out + bias
    return torch.relu(out) if relu else out


def spmm(rowptr, col, val, B, n_rows, bias=None, relu=False):
    fn = _spmm_hip if _AGG_BACKEND == 'hip' else _spmm_torch
    return fn(rowptr, col, val, B, n_rows, bias, relu)


def spmm_pair(rowptr, col, val, B2, n_rows, n_feat, bias=None, split=False):
    """[Â·B0 + bias | Â·B1 + bias] for B2 = [B0 | B1] (two blocks of ``n_feat`` columns) in ONE sweep of the indices
    (``dcr_spmm_csr_f32_pair_dev``): every block bit-identical to a ``spmm`` call of its own.  ``split``: the two blocks
    as two contiguous matrices (written there by the kernel: no copies afterwards)."""
    if _AGG_BACKEND != 'hip':
        a, b = (_spmm_torch(rowptr, col, val, B2[:, :n_feat], n_rows, bias), _spmm_torch(rowptr, col, val, B2[:, n_feat:], n_rows, bias))
        return (a, b) if split else torch.cat([a, b], 1)
    if not B2.is_cuda:
        raise RuntimeError('GCN aggregation runs on the MI355X HIP kernel (there is no CPU fallback)')
    B2 = B2.contiguous()
    if split and n_feat % 4 == 0:
        C = torch.empty((2, n_rows, n_feat), dtype=torch.float32, device=B2.device)
        _lib.check(_lib.lib().dcr_spmm_csr_f32_pair_split_dev(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), B2.data_ptr(),
                                                              C[0].data_ptr(), C[1].data_ptr(), n_rows, n_feat, 2 * n_feat, n_feat,
                                                              _ptr(bias), 0, _stream(B2)))
        return C[0], C[1]
    C = torch.empty((n_rows, 2 * n_feat), dtype=torch.float32, device=B2.device)
    _lib.check(_lib.lib().dcr_spmm_csr_f32_pair_dev(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), B2.data_ptr(), C.data_ptr(),
                                                    n_rows, n_feat, 2 * n_feat, 2 * n_feat, _ptr(bias), 0, _stream(B2)))
    return (C[:, :n_feat].contiguous(), C[:, n_feat:].contiguous()) if split else C


def _aggregate_backward(csr, sel, grad, z_shape, need_z, need_b):
    """(dZ, db) of out = (Â·Z + b)[sel.idx] (``sel`` None: every row) from ``grad``, the gradient of out: dZ = Âᵀ[:, sel.idx]·grad,
    zeros of ``z_shape`` for an empty selection; db = Σ_rows grad.  Either is None when not needed."""
    grad = grad.contiguous()
    gz = None
    if need_z:
        if sel is None:
            gz = spmm(csr.rowptr_t, csr.col_t, csr.val_t, grad, csr.n_cols)
        elif sel.n == 0:
            gz = grad.new_zeros(z_shape)
        else:
            gz = spmm(*sel.transposed(), grad, csr.n_cols)
    return gz, (grad.sum(0) if need_b else None)


def _halves_of_one_buffer(z_train, z_eval):
    """Whether the two operands are the column blocks [z_train | z_eval] of ONE fp32 matrix on the GPU: act_then_linear and the
    one-kernel first layer write them that way, and the pair aggregations then read both without a concatenation."""
    f = z_train.shape[1]
    return (z_train.is_cuda and z_train.dtype == torch.float32 and z_train.stride() == (2 * f, 1) and z_eval.stride() == (2 * f, 1)
            and z_eval.data_ptr() == z_train.data_ptr() + 4 * f)


class _Aggregate(torch.autograd.Function):
    """out = Â·Z + b ; dZ = Âᵀ·dout ; db = Σ_rows dout."""

    @staticmethod
    def forward(ctx, z, bias, csr):
        ctx.csr = csr
        ctx.has_bias = bias is not None
        return spmm(csr.rowptr, csr.col, csr.val, z, csr.n_rows, bias=bias)

    @staticmethod
    def backward(ctx, grad_out):
        need = ctx.needs_input_grad
        return _aggregate_backward(ctx.csr, None, grad_out, None, need[0], ctx.has_bias and need[1]) + (None,)


def aggregate(z, bias, csr):
    return _Aggregate.apply(z, bias, csr)


class _AggregatePair(torch.autograd.Function):
    """(Â·Z_train + b, Â·Z_eval + b) in one pass over the graph; only the training operand carries a gradient."""

    @staticmethod
    def forward(ctx, z_train, z_eval, bias, csr):
        ctx.csr = csr
        ctx.has_bias = bias is not None
        f = z_train.shape[1]
        if _halves_of_one_buffer(z_train, z_eval):
            b2 = torch.as_strided(z_train, (z_train.shape[0], 2 * f), (2 * f, 1))
        else:
            b2 = torch.cat([z_train, z_eval], 1)
        return spmm_pair(csr.rowptr, csr.col, csr.val, b2, csr.n_rows, f, bias=bias, split=True)

    @staticmethod
    def backward(ctx, grad_train, grad_eval):
        need = ctx.needs_input_grad
        gz, gb = _aggregate_backward(ctx.csr, None, grad_train, None, need[0], ctx.has_bias and need[2])
        return gz, None, gb, None


def _aggregate_wanted(z_train, z_eval, bias, csr):
    """(Â·Z_train + b, Â·Z_eval + b) at every row for the operands wanted (None: not wanted), both in one sweep of the graph."""
    if z_train is not None and z_eval is not None:
        return _AggregatePair.apply(z_train, z_eval, bias, csr)
    if z_train is not None:
        return aggregate(z_train, bias, csr), None
    return None, aggregate(z_eval, bias, csr)


class RowSelection:
    """The rows of the last aggregation an epoch reads — the nodes of a split (experiment/training_loop.py:50-51,64-71 index
    the model's output with the split masks and use nothing else) — and, for the backward pass, Âᵀ restricted to those
    columns: the gradient of the loss is zero outside them, so dZ = Âᵀ·dOut needs the selected columns only."""

    def __init__(self, csr, rows):
        # ``expand``: None, or the positions in ``idx`` of the caller's entries when its index tensor repeats a node:
        # the kernels (and ``transposed``, whose column map holds one position per node) then work on the distinct nodes and
        # the callers gather ``out.index_select(0, expand)``, whose backward ADDS the gradients of the repeats — what
        # ``model(data)[rows].backward()`` does.  Checked once per selection (one host sync; selections are cached).
        self.expand = None
        if rows.dtype == torch.bool:
            if rows.dim() != 1 or rows.numel() != csr.n_rows:
                raise IndexError(f'row mask of shape {tuple(rows.shape)} for {csr.n_rows} nodes')
            idx = rows.nonzero().squeeze(1)
        else:
            if rows.dim() != 1 or rows.dtype not in (torch.int64, torch.int32):
                raise IndexError('rows must be a boolean node mask or a 1-d int64 / int32 index tensor')
            idx = rows.to(torch.int64)
            if idx.numel():
                lo, hi = int(idx.min()), int(idx.max())
                if lo < -csr.n_rows or hi >= csr.n_rows:
                    raise IndexError(f'row index out of range for {csr.n_rows} nodes: [{lo}, {hi}]')
                if lo < 0:
                    idx = torch.where(idx < 0, idx + csr.n_rows, idx)     # as tensor indexing reads them
                uniq, inverse = torch.unique(idx, return_inverse=True)
                if uniq.numel() != idx.numel():
                    idx, self.expand = uniq, inverse.contiguous()
        self.idx = idx.contiguous()
        self.n = int(self.idx.numel())
        self._csr = csr
        self._t = None

    def expanded(self, out):
        """``out`` (one row per distinct selected node) in the caller's index order, repeats included."""
        return out if self.expand is None else out.index_select(0, self.expand)

    def joined_with(self, other):
        """[idx | other.idx] as one tensor (the row list of ``dcr_spmm_csr_rows2_f32_dev``); built once per pair."""
        cache = self.__dict__.setdefault('_joined', {})
        hit = cache.get(id(other))
        if hit is None or hit[0] is not other:
            hit = cache[id(other)] = (other, torch.cat([self.idx, other.idx]).contiguous())
        return hit[1]

    def transposed(self):
        """(rowptr, col, val) of Âᵀ[:, idx] with the columns renumbered 0..n-1 (positions in ``idx``); built once."""
        if self._t is None:
            csr, dev = self._csr, self.idx.device
            pos = torch.full((csr.n_rows,), -1, dtype=torch.int32, device=dev)
            pos[self.idx] = torch.arange(self.n, dtype=torch.int32, device=dev)
            p = pos[csr.col_t.long()]
            keep = p >= 0
            cs = torch.zeros(keep.numel() + 1, dtype=torch.int64, device=dev)
            torch.cumsum(keep, 0, out=cs[1:])
            self._t = (cs[csr.rowptr_t].contiguous(), p[keep].contiguous(), csr.val_t[keep].contiguous())
        return self._t


def spmm_rows(csr, sel, B, bias=None):
    """Rows ``sel.idx`` of Â·B + bias (``dcr_spmm_csr_rows_f32_dev``): [sel.n, F], every row bit-identical to that row of
    ``spmm``.  ``B`` may be a column block of a wider matrix (stride (ld, 1))."""
    F = B.shape[1]
    if _AGG_BACKEND != 'hip':
        return _spmm_torch(csr.rowptr, csr.col, csr.val, B, csr.n_rows, bias).index_select(0, sel.idx)
    if not B.is_cuda:
        raise RuntimeError('GCN aggregation runs on the MI355X HIP kernel (there is no CPU fallback)')
    if B.dtype != torch.float32:
        raise TypeError('dcr_spmm_csr_rows_f32_dev is fp32')
    if B.dim() != 2 or B.stride(1) != 1 or B.stride(0) < F:
        B = B.contiguous()
    C = torch.empty((sel.n, F), dtype=torch.float32, device=B.device)
    if sel.n == 0:
        return C
    _lib.check(_lib.lib().dcr_spmm_csr_rows_f32_dev(csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(),
                                                    sel.idx.data_ptr(), sel.n, B.data_ptr(), C.data_ptr(), F, B.stride(0), F,
                                                    _ptr(bias), 0, _stream(B)))
    return C


def _spmm_rows_pair(csr, sel_train, sel_eval, z_train, z_eval, bias):
    """(rows ``sel_train`` of Â·Z_train + b, rows ``sel_eval`` of Â·Z_eval + b): ONE launch (``dcr_spmm_csr_rows2_f32_dev``) when
    the two operands are the halves of one buffer, two ``spmm_rows`` calls otherwise; every row as ``spmm_rows`` computes it."""
    f = z_train.shape[1]
    if not (_AGG_BACKEND == 'hip' and f % 4 == 0 and sel_train.n > 0 and sel_eval.n > 0 and _halves_of_one_buffer(z_train, z_eval)):
        out_ev = spmm_rows(csr, sel_eval, z_eval, bias)
        return spmm_rows(csr, sel_train, z_train, bias), out_ev
    both = sel_train.joined_with(sel_eval)
    C = torch.empty((sel_train.n + sel_eval.n, f), dtype=torch.float32, device=z_train.device)
    _lib.check(_lib.lib().dcr_spmm_csr_rows2_f32_dev(csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(), both.data_ptr(),
                                                     sel_train.n, sel_train.n + sel_eval.n, z_train.data_ptr(), f, C.data_ptr(), f,
                                                     2 * f, f, _ptr(bias), 0, _stream(z_train)))
    return C[:sel_train.n], C[sel_train.n:]


class _AggregateRows(torch.autograd.Function):
    """out = (Â·Z + b)[rows] ; dZ = Âᵀ[:, rows]·dout ; db = Σ dout."""

    @staticmethod
    def forward(ctx, z, bias, csr, sel):
        ctx.csr, ctx.sel = csr, sel
        ctx.has_bias = bias is not None
        ctx.z_shape = z.shape
        return spmm_rows(csr, sel, z, bias)

    @staticmethod
    def backward(ctx, grad_out):
        need = ctx.needs_input_grad
        return _aggregate_backward(ctx.csr, ctx.sel, grad_out, ctx.z_shape, need[0], ctx.has_bias and need[1]) + (None, None)


def aggregate_rows(z, bias, csr, sel):
    return _AggregateRows.apply(z, bias, csr, sel)


class _AggregateRowsPair(torch.autograd.Function):
    """((Â·Z_train + b)[rows_train], (Â·Z_eval + b)[rows_eval]) in ONE launch when the two operands are the halves of one
    buffer (act_then_linear writes them that way): ``dcr_spmm_csr_rows2_f32_dev``, every row as ``spmm_rows`` computes it.
    Only the training operand carries a gradient (as ``_AggregateRows``)."""

    @staticmethod
    def forward(ctx, z_train, z_eval, bias, csr, sel_train, sel_eval):
        ctx.csr, ctx.sel = csr, sel_train
        ctx.has_bias = bias is not None
        ctx.z_shape = z_train.shape
        out_tr, out_ev = _spmm_rows_pair(csr, sel_train, sel_eval, z_train, z_eval, bias)
        ctx.mark_non_differentiable(out_ev)
        return out_tr, out_ev

    @staticmethod
    def backward(ctx, grad_train, grad_eval):
        need = ctx.needs_input_grad
        gz, gb = _aggregate_backward(ctx.csr, ctx.sel, grad_train, ctx.z_shape, need[0], ctx.has_bias and need[2])
        return gz, None, gb, None, None, None


_WORKSPACES = {}


def _workspace(kind, device, stream, *shape):
    """Partials + tickets of the kernels whose last workgroup closes a reduction: 'head' (dcr_head_*, the picked-mean loss)
    or 'first' (the K-chunked first layer; shape = (n, feats, hidden), None where W1 stays resident in LDS).  The tickets are
    zero before the first launch and every launch leaves them zero, so a buffer is zero-filled once, on creation, and needs
    no fill launch per call.  One buffer per (kind, device, stream, shape), never evicted: a captured epoch replays on the
    raw pointers it was captured with."""
    stream = getattr(stream, 'value', stream) or 0          # (an integer handle, or what ``_stream`` gives)
    key = (kind, str(device), int(stream)) + tuple(int(v) for v in shape)
    if key not in _WORKSPACES:
        need = ctypes.c_int64()
        if kind == 'head':
            _lib.check(_lib.lib().dcr_head_workspace(ctypes.byref(need)))
            _WORKSPACES[key] = torch.zeros((need.value + 7) // 8, dtype=torch.int64, device=device)
        else:
            _lib.check(_lib.lib().dcr_first_layer_fwd_workspace(*key[3:], ctypes.byref(need)))
            _WORKSPACES[key] = torch.zeros(need.value, dtype=torch.float32, device=device) if need.value else None
    return _WORKSPACES[key]


def _head_workspace(device, stream):
    return _workspace('head', device, stream)


def _first_layer_workspace(device, stream, n, feats, hidden):
    return _workspace('first', device, stream, n, feats, hidden)


HEAD_MAX_CLASSES = 32   # (dcr_head_*: HEAD_MAXC in csrc/dcr_gcn.hip)


def head_ok(z, sel_train, sel_eval, n_classes):
    """Whether the one-kernel head takes outputs of ``z``'s device and dtype: fp32 on the GPU, at most 32 classes, row
    selections without repeats."""
    return (_AGG_BACKEND == 'hip' and z.is_cuda and z.dtype == torch.float32 and 1 <= n_classes <= HEAD_MAX_CLASSES
            and (sel_train is None or sel_train.expand is None) and (sel_eval is None or sel_eval.expand is None)
            and os.environ.get('DCR_FUSED_HEAD', '1') != '0')


class _AggregateRowsHead(torch.autograd.Function):
    """The last aggregation at the rows an epoch reads AND what the epoch does with them, without the log-probabilities in
    between (models/gcn.py:44 + experiment/training_loop.py:51 and :64-71):
        loss    = F.nll_loss(log_softmax((Â·Z_train + b)[rows_train]), y_train)      (float32 0-dim; None without training rows)
        correct = ((Â·Z_eval + b)[rows_eval].argmax(1) == y_eval).sum()             (int64 0-dim; None without evaluated rows)
    One aggregation launch (``dcr_spmm_csr_rows2_f32_dev`` when both operands are the halves of one buffer) and one head kernel
    (``dcr_head_fwd_f32_dev``); backward: ``dcr_head_bwd_f32_dev`` (gradient of the selected outputs and its column sums = the
    bias gradient), then dZ = Âᵀ[:, rows]·dOut.  Every selected output row is what ``spmm_rows`` computes."""

    @staticmethod
    def forward(ctx, z_train, z_eval, bias, csr, sel_train, sel_eval, y_train, y_eval):
        have_tr, have_ev = z_train is not None, z_eval is not None
        ref = z_train if have_tr else z_eval
        f = ref.shape[1]
        out_tr = out_ev = None
        if have_tr and have_ev:
            out_tr, out_ev = _spmm_rows_pair(csr, sel_train, sel_eval, z_train, z_eval, bias)
        elif have_tr:
            out_tr = spmm_rows(csr, sel_train, z_train, bias)
        else:
            out_ev = spmm_rows(csr, sel_eval, z_eval, bias)
        stream = _stream(ref)
        ws = _head_workspace(ref.device, stream)
        loss = torch.empty((), dtype=torch.float32, device=ref.device) if have_tr else None
        correct = torch.empty((), dtype=torch.int64, device=ref.device) if have_ev else None
        m_tr = out_tr.shape[0] if have_tr else 0
        m_ev = out_ev.shape[0] if have_ev else 0
        if m_tr + m_ev > 0:
            _lib.check(_lib.lib().dcr_head_fwd_f32_dev(
                out_tr.data_ptr() if m_tr else None, out_tr.stride(0) if m_tr else f, y_train.data_ptr() if m_tr else None, m_tr,
                out_ev.data_ptr() if m_ev else None, out_ev.stride(0) if m_ev else f, y_eval.data_ptr() if m_ev else None, m_ev, f,
                _ptr(loss), _ptr(correct), ws.data_ptr(), ws.numel() * 8, stream))
        if have_tr and not m_tr:
            loss.fill_(float('nan'))          # (the mean over no rows, as F.nll_loss gives it)
        if have_ev and not m_ev:
            correct.zero_()
        ctx.csr, ctx.sel, ctx.has_bias, ctx.out_tr, ctx.y_train = csr, sel_train, bias is not None, out_tr, y_train
        ctx.z_shape = z_train.shape if have_tr else None
        if correct is not None:
            ctx.mark_non_differentiable(correct)
        ctx.set_materialize_grads(False)   # (no zero-filled "gradient" of the count: a fill launch per step)
        return loss, correct

    @staticmethod
    def backward(ctx, g_loss, _g_correct):
        out_tr, need = ctx.out_tr, ctx.needs_input_grad
        if g_loss is None or out_tr is None:
            return (None,) * 8
        m, f = out_tr.shape
        need_b = ctx.has_bias and need[2]
        if m == 0:   # (no training rows: zero gradients, no head kernel)
            gz, _ = _aggregate_backward(ctx.csr, ctx.sel, out_tr, ctx.z_shape, need[0], False)
            return (gz, None, out_tr.new_zeros(f) if need_b else None) + (None,) * 5
        g = g_loss.contiguous().float()
        grad = torch.empty((m, f), dtype=torch.float32, device=out_tr.device)
        gb = torch.empty(f, dtype=torch.float32, device=out_tr.device)
        stream = _stream(out_tr)
        ws = _head_workspace(out_tr.device, stream)
        _lib.check(_lib.lib().dcr_head_bwd_f32_dev(out_tr.data_ptr(), out_tr.stride(0), ctx.y_train.data_ptr(), m, f, g.data_ptr(),
                                                   grad.data_ptr(), gb.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream))
        gz, _ = _aggregate_backward(ctx.csr, ctx.sel, grad, ctx.z_shape, need[0], False)   # (db came out of the head kernel)
        return (gz, None, gb if need_b else None) + (None,) * 5


def atb_hip(a, b):
    """``a.t() @ b`` for tall-skinny fp32 operands [K, M], [K, N] on the hand-written MFMA kernel
    (csrc/dcr_gemm.hip, ``dcr_atb_f32_dev``)."""
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError('dcr_atb_f32_dev runs on the MI355X (there is no CPU fallback)')
    a, b = a.contiguous(), b.contiguous()
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape[0] != b.shape[0]:
        raise TypeError('atb_hip: fp32 [K, M] and [K, N] expected')
    K, M, N = a.shape[0], a.shape[1], b.shape[1]
    need = ctypes.c_int64()
    _lib.check(_lib.lib().dcr_atb_f32_workspace(K, M, N, ctypes.byref(need)))
    ws = torch.empty(max(need.value, 1), dtype=torch.float32, device=a.device)
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().dcr_atb_f32_dev(a.data_ptr(), b.data_ptr(), out.data_ptr(), K, M, N, M, N, N, ws.data_ptr(),
                                          need.value, _stream(a)))
    return out


class _LinearFn(torch.autograd.Function):
    """y = x·Wᵀ (+ b) through the GEMM library; dW = dyᵀ·x (a reduction over all nodes) on the hand-written MFMA
    kernel."""

    colsum_handoffs = 0   # bias gradients taken from the kernel that produced grad_out (read by the tests)

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        gx = grad_out @ weight if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1]:
            # a reduction over all nodes into a small tile: the case the GEMM library splits badly (measured 2.3x
            # and 3.9x slower at 1M nodes); for wide layers on small graphs the library is as fast
            tall = x.shape[0] >= 64 * max(x.shape[1], grad_out.shape[1])
            gw = atb_hip(grad_out, x) if tall else grad_out.t() @ x
        gb = _column_sums(grad_out) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return gx, gw, gb


def _column_sums(grad):
    """``grad.sum(0)`` — a bias gradient — taken from the kernel that produced ``grad`` where it left them there
    (``_dcr_colsum``, see ``_act_linear_backward``), computed otherwise."""
    ready = getattr(grad, '_dcr_colsum', None)
    if ready is not None and ready[:2] == (grad.data_ptr(), grad._version):
        _LinearFn.colsum_handoffs += 1
        return ready[2]
    return grad.sum(0)


_dropout_ctr = {}  # per device: int64 call counter IN DEVICE MEMORY = offset of the Philox stream (one step per fused
#                    ReLU+dropout call).  On the device so that a captured hipGraph of the training step draws a new
#                    mask at every replay: the launch parameters stay constant, the counter moves.


def _dropout_counter(device):
    key = str(device)
    if key not in _dropout_ctr:
        _dropout_ctr[key] = torch.zeros(1, dtype=torch.int64, device=device)
    return _dropout_ctr[key]


def _dropout_bits(numel, device):
    """(keep bits of a tensor of ``numel`` elements, one bit each, uninitialised; the device's dropout counter)."""
    words = ctypes.c_int64()
    _lib.check(_lib.lib().dcr_relu_dropout_bits_words(numel, ctypes.byref(words)))
    return torch.empty(max(words.value, 1), dtype=torch.int64, device=device), _dropout_counter(device)


def _train_eval_outputs(n, classes, want_train, want_eval, like):
    """(z_train, z_eval, their leading dimension) of a kernel that writes either or both: both as the halves of ONE buffer
    [z_train | z_eval] — what the pair aggregations read, without a concatenation; None for the one not wanted."""
    if want_train and want_eval:
        both = torch.empty((n, 2 * classes), dtype=like.dtype, device=like.device)
        return both[:, :classes], both[:, classes:], 2 * classes
    z = torch.empty((n, classes), dtype=like.dtype, device=like.device)
    return (z, None, classes) if want_train else (None, z, classes)


class _ReluDropoutFn(torch.autograd.Function):
    """y = dropout(relu(x)) in one pass each way (csrc/dcr_gcn.hip), the keep mask packed to one bit per element."""

    @staticmethod
    def forward(ctx, x, p):
        x = x.contiguous()
        bits, ctr = _dropout_bits(x.numel(), x.device)
        y = torch.empty_like(x)
        _lib.check(_lib.lib().dcr_relu_dropout_fwd_f32_ctr_dev(x.data_ptr(), y.data_ptr(), bits.data_ptr(), x.numel(), float(p),
                                                               torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, 0,
                                                               ctr.data_ptr(), _stream(x)))
        ctr.add_(1)
        ctx.bits, ctx.p = bits, float(p)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        grad_out = grad_out.contiguous()
        gin = torch.empty_like(grad_out)
        _lib.check(_lib.lib().dcr_relu_dropout_bwd_f32_dev(grad_out.data_ptr(), gin.data_ptr(), ctx.bits.data_ptr(),
                                                           grad_out.numel(), ctx.p, _stream(grad_out)))
        return gin, None


def relu_dropout(x, act_fn, dropout):
    """``dropout(act_fn(x))`` (models/gcn.py:38-42).  Training on the MI355X with ReLU: the fused kernel; otherwise the
    two stock modules (evaluation, CPU tests, other activations)."""
    if (_AGG_BACKEND == 'hip' and x.is_cuda and x.dtype == torch.float32 and dropout.training and 0.0 < dropout.p < 1.0
            and isinstance(act_fn, ReLU) and x.data_ptr() % 16 == 0):
        return _ReluDropoutFn.apply(x, dropout.p)
    return dropout(act_fn(x))


class _ActLinearFn(torch.autograd.Function):
    """(dropout(relu(x))·Wᵀ, relu(x)·Wᵀ) in ONE pass over x (csrc/dcr_gcn.hip, dcr_act_linear_fwd_f32_dev): the activation
    between two layers fused into the next layer's dense contraction, for the training operand, the evaluation operand or
    both.  Only the training operand carries a gradient; its backward is one pass too (dcr_act_linear_bwd_f32_dev), the
    weight gradient the MFMA reduction kernel on the stored training activation."""

    @staticmethod
    def forward(ctx, x, weight, p, want_train, want_eval):
        x = x.contiguous()
        w = weight.contiguous()
        n, hidden = x.shape
        classes = w.shape[0]
        z_tr, z_ev, ldz = _train_eval_outputs(n, classes, want_train, want_eval, x)
        bits, ctr = _dropout_bits(x.numel(), x.device) if want_train else (None, None)
        # (no training activation is stored: the backward kernel rebuilds it from x and the keep bits)
        _lib.check(_lib.lib().dcr_act_linear_fwd_f32_dev(
            x.data_ptr(), w.data_ptr(), None, _ptr(z_tr), _ptr(z_ev), ldz, _ptr(bits), n, hidden, classes, float(p),
            torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, 0, _ptr(ctr), _stream(x)))
        if want_train:
            ctr.add_(1)
            ctx.save_for_backward(x, w)
            ctx.bits, ctx.p = bits, float(p)
        if want_eval:
            ctx.mark_non_differentiable(z_ev)
        return z_tr, z_ev

    @staticmethod
    def backward(ctx, g_tr, g_ev):
        x, w = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None, None
        gx, gw, colsum = _act_linear_backward(g_tr.contiguous(), w, ctx.bits, x, ctx.p)
        # (the column sums of dx are the bias gradient of the layer that produced x: _column_sums picks them up there instead of
        #  reading the N x H gradient once more)
        gx._dcr_colsum = (gx.data_ptr(), gx._version, colsum)
        return (gx if ctx.needs_input_grad[0] else None), (gw if ctx.needs_input_grad[1] else None), None, None, None


def _act_linear_backward(g, w, bits, x, p):
    """(dx, dW, column sums of dx) of z = dropout(relu(x))·Wᵀ from dz = ``g`` in one pass over x
    (``dcr_act_linear_bwd_fused_f32_dev``): the activation is rebuilt from x and the keep bits."""
    n, hidden = x.shape
    gx = torch.empty_like(x)
    gw = torch.empty_like(w)
    colsum = torch.empty(hidden, dtype=torch.float32, device=x.device)
    need = ctypes.c_int64()
    _lib.check(_lib.lib().dcr_act_linear_bwd_fused_workspace(n, hidden, ctypes.byref(need)))
    ws = torch.empty(max(need.value, 1), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dcr_act_linear_bwd_fused_f32_dev(g.data_ptr(), w.data_ptr(), bits.data_ptr(), x.data_ptr(), gx.data_ptr(),
                                                           gw.data_ptr(), colsum.data_ptr(), ws.data_ptr(), need.value, n, hidden,
                                                           w.shape[0], p, _stream(g)))
    return gx, gw, colsum


def act_then_linear(x, act_fn, dropout, lin, want_train=True, want_eval=False):
    """(lin(dropout(act_fn(x))), lin(act_fn(x))) — the part of models/gcn.py:36-42 between one layer's aggregation and the
    next one's (either may be None when not wanted).  Fused into one pass on the MI355X for ReLU, hidden width 64 / 128 and
    at most 16 classes; the stock modules otherwise (CPU tests, other shapes, other activations)."""
    w = lin.weight
    can = (_AGG_BACKEND == 'hip' and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and isinstance(act_fn, ReLU)
           and x.shape[1] in (64, 128) and w.shape[0] <= 16 and x.data_ptr() % 16 == 0)
    train_ok = can and dropout.training and 0.0 < dropout.p < 1.0
    # (each operand takes the same route whatever else is asked for in the same call: the evaluation output of the one-pass
    #  epoch equals an evaluation-mode forward bit for bit, the training output a training-mode forward)
    if want_train and want_eval and train_ok:
        return _ActLinearFn.apply(x, w, dropout.p, True, True)
    z_tr = z_ev = None
    if want_train:
        z_tr = _ActLinearFn.apply(x, w, dropout.p, True, False)[0] if train_ok else lin(relu_dropout(x, act_fn, dropout))
    if want_eval:
        with torch.no_grad():
            z_ev = _ActLinearFn.apply(x.detach(), w.detach(), 0.0, False, True)[1] if can else lin(act_fn(x.detach()))
    return z_tr, z_ev


def _act_then_linear_pair(o_train, o_eval, act_fn, dropout, lin, eval_grad=False):
    """``act_then_linear`` for the training and the evaluation operand of one layer (None: not wanted), which call for which:
    ONE pass for both exactly when the evaluation operand is the detached training tensor (the first hidden layer); from
    the second hidden layer on the two differ (dropout), so training first, then evaluation.  ``eval_grad`` (an evaluation
    operand that may carry a gradient — not on the training path): the stock modules when it does."""
    if o_train is not None and o_eval is not None and o_eval.data_ptr() == o_train.data_ptr():
        return act_then_linear(o_train, act_fn, dropout, lin, want_train=True, want_eval=True)
    z_train = z_eval = None
    if o_train is not None:
        z_train, _ = act_then_linear(o_train, act_fn, dropout, lin, want_train=True, want_eval=False)
    if o_eval is not None and eval_grad and torch.is_grad_enabled() and o_eval.requires_grad:
        z_eval = lin(dropout(act_fn(o_eval)))
    elif o_eval is not None:
        _, z_eval = act_then_linear(o_eval, act_fn, dropout, lin, want_train=False, want_eval=True)
    return z_train, z_eval


class _DropoutAhead:
    """The dropout decisions of the NEXT training call of the one-kernel first layer, drawn on a side stream while the rest of
    the current epoch runs (dcr_dropout_words_dev; round 5).  The Philox instructions of the decisions were most of the vector
    work of k_first_layer_fwd, and on this chip vector instructions add to the matrix cores' time; drawn by a kernel of their
    own they overlap the aggregations, which leave the vector units idle (they wait on their gathers).  The words carry the
    stamp of the call they were drawn for — a call with another stamp (the counter moved: a second model, a forward without
    the expected successor) draws in line, so the result never depends on this object, only the time does.

    One per (device, rows, hidden, p); the side stream forks after the forward kernel and is joined before the next use of the
    words: at the start of the layer's backward, or by ``join_dropout_ahead()`` (the epoch drivers call it before a capture
    ends), or at the next forward."""

    def __init__(self, device, n, hidden, p):
        words = ctypes.c_int64()
        _lib.check(_lib.lib().dcr_dropout_words_count(n, hidden, ctypes.byref(words)))
        self.words = torch.zeros(words.value, dtype=torch.int64, device=device)   # (stamp of no call: rows = 0)
        self.next_offset_ptr = self.words.data_ptr() + 8 * (words.value - 4)
        self.stream = torch.cuda.Stream(device)
        self.device, self.n, self.hidden, self.p = device, int(n), int(hidden), float(p)
        self.forked = False

    def draw(self):
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        _lib.check(_lib.lib().dcr_dropout_words_dev(self.words.data_ptr(), self.n, self.hidden, self.p,
                                                    torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, 0, self.next_offset_ptr,
                                                    ctypes.c_void_p(self.stream.cuda_stream)))
        self.forked = True

    def join(self):
        if self.forked:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
            self.forked = False


_AHEAD = {}


def _dropout_ahead(device, n, hidden, p):
    """The _DropoutAhead of this shape, or None: not switched on (``DCR_DROPOUT_AHEAD=1``; OFF by default — measured on the
    MI355X at the 1M-node shape, the forward kernel gains 23 us of its 700 inside the epoch (82 us back to back, where the
    clock is lower) and the aggregation beside the drawing kernel loses 14: 1.585 ms per epoch against 1.589, within the noise;
    profiles/r05_dropout_ahead.txt), or it would have to be created inside a stream capture (the epoch drivers run eager
    epochs first, which create it)."""
    if os.environ.get('DCR_DROPOUT_AHEAD', '0') != '1':
        return None
    key = (str(device), int(n), int(hidden), float(p))
    ahead = _AHEAD.get(key)
    if ahead is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        if len(_AHEAD) >= 4:
            old = _AHEAD.pop(next(iter(_AHEAD)))
            old.join()
        ahead = _AHEAD[key] = _DropoutAhead(device, n, hidden, p)
    return ahead


def join_dropout_ahead():
    """Join every side stream drawing dropout decisions ahead into the current stream (before a stream capture ends)."""
    for ahead in _AHEAD.values():
        ahead.join()


class _FirstLayerFn(torch.autograd.Function):
    """The first layer's GEMM on Â·X, bias, ReLU (+ dropout) and the second layer's lin in ONE kernel on the matrix cores
    (csrc/dcr_gcn_first.hip, dcr_first_layer_fwd_f32_dev): models/gcn.py:36-42 from ``x`` of the first GCNConv to the
    second GCNConv's ``lin`` output, for the training operand, the evaluation operand or both.  The hidden activation
    never leaves the registers; the pre-activation is written once for the backward pass (training) or not at all.
    Backward: one kernel too (dcr_first_layer_bwd_f32_dev: dW1, db1, dW2 with the pre-activation's gradient in registers);
    ``DCR_FIRST_BWD_FUSED=0``: the fused MFMA pass of _ActLinearFn (dx, db1, dW2), then dW1 = dxᵀ·(Â·X)."""

    @staticmethod
    def forward(ctx, ax, w1, b1, w2, p, want_train, want_eval):
        w1, w2 = w1.contiguous(), w2.contiguous()
        # ax: Â·X, [n, feats] or (round 5) [n, feats rounded up to 16] with zero pad columns — what the K-chunked kernel for
        # input widths like Cora's 1,433 and Citeseer's 3,703 reads (GCNConv.propagated_input(..., pad16=True))
        if ax.stride(1) != 1 or ax.stride(0) % 4:
            ax = ax.contiguous()
        n = ax.shape[0]
        hidden, feats, classes = w1.shape[0], w1.shape[1], w2.shape[0]
        f16 = (feats + 15) // 16 * 16
        if ax.shape[1] < f16:                      # (a caller that did not pad: pad here, once per call)
            ax = torch.nn.functional.pad(ax, (0, f16 - ax.shape[1]))
        stream = _stream(ax)
        z_tr, z_ev, ldz = _train_eval_outputs(n, classes, want_train, want_eval, ax)
        bits = ctr = pre = None
        if want_train:
            bits, ctr = _dropout_bits(n * hidden, ax.device)
            pre = torch.empty((n, hidden), dtype=ax.dtype, device=ax.device)
        ws = _first_layer_workspace(ax.device, stream, n, feats, hidden)
        ahead = _dropout_ahead(ax.device, n, hidden, p) if (want_train and p > 0.0 and n > 0) else None
        if ahead is not None:
            ahead.join()
        _lib.check(_lib.lib().dcr_first_layer_fwd_ws_f32_dev(
            ax.data_ptr(), ax.stride(0), w1.data_ptr(), _ptr(b1), w2.data_ptr(), _ptr(pre), _ptr(z_tr), _ptr(z_ev), ldz, _ptr(bits),
            None if ahead is None else ahead.words.data_ptr(), n, feats, hidden, classes,
            float(p), torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, 0, _ptr(ctr), _ptr(ws), 0 if ws is None else ws.numel(), stream))
        ctx.ahead = ahead
        if want_train:
            ctr.add_(1)
            if ahead is not None:
                ahead.draw()   # the next call's decisions, beside whatever this stream does next
            ctx.save_for_backward(ax, w2)
            ctx.pre, ctx.bits, ctx.p, ctx.has_bias, ctx.feats = pre, bits, float(p), b1 is not None, feats
        if want_eval:
            ctx.mark_non_differentiable(z_ev)
        ctx.set_materialize_grads(False)   # (the evaluation output's zero "gradient": N x classes floats filled per step, 10 us at S1M)
        return z_tr, z_ev

    @staticmethod
    def backward(ctx, g_tr, g_ev):
        if ctx.ahead is not None:
            ctx.ahead.join()   # (inside the same capture as the fork, when there is one)
        if g_tr is None:
            return None, None, None, None, None, None, None
        ax, w2 = ctx.saved_tensors
        pre = ctx.pre
        g_tr = g_tr.contiguous()
        n, hidden = pre.shape
        aligned = all(t.data_ptr() % 16 == 0 for t in (ax, g_tr, pre, ctx.bits))   # (the kernel's stage copies move 16-byte pieces)
        feats = ctx.feats
        if os.environ.get('DCR_FIRST_BWD_FUSED', '1') != '0' and aligned:
            # one kernel (dcr_first_layer_bwd_f32_dev): the gradient of the pre-activation stays in registers between the
            # contraction with W2 that forms it and the contraction with Â·X that consumes it
            gw1 = torch.empty((hidden, feats), dtype=torch.float32, device=pre.device)
            gw2 = torch.empty_like(w2)
            gb1 = torch.empty(hidden, dtype=torch.float32, device=pre.device)
            need = ctypes.c_int64()
            _lib.check(_lib.lib().dcr_first_layer_bwd_workspace(n, feats, hidden, ctypes.byref(need)))
            ws = torch.empty(max(need.value, 1), dtype=torch.float32, device=pre.device)
            _lib.check(_lib.lib().dcr_first_layer_bwd_f32_dev(g_tr.data_ptr(), w2.data_ptr(), ctx.bits.data_ptr(), pre.data_ptr(),
                                                              ax.data_ptr(), ax.stride(0), gw1.data_ptr(), gb1.data_ptr(), gw2.data_ptr(),
                                                              ws.data_ptr(), need.value, n, feats, hidden, w2.shape[0], ctx.p,
                                                              _stream(g_tr)))
            return (None, gw1 if ctx.needs_input_grad[1] else None, gb1 if (ctx.has_bias and ctx.needs_input_grad[2]) else None,
                    gw2 if ctx.needs_input_grad[3] else None, None, None, None)
        if ax.shape[1] != feats:
            ax = ax[:, :feats].contiguous()      # (the separate kernels take the unpadded matrix)
        gx, gw2, colsum = _act_linear_backward(g_tr, w2, ctx.bits, pre, ctx.p)
        gw1 = None
        if ctx.needs_input_grad[1]:
            tall = n >= 64 * max(ax.shape[1], hidden)   # (as _LinearFn.backward)
            gw1 = atb_hip(gx, ax) if tall else gx.t() @ ax
        gb1 = colsum if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return None, gw1, gb1, (gw2 if ctx.needs_input_grad[3] else None), None, None, None


def first_layer_fused_ok(x, act_fn, first, lin2):
    """Whether the one-kernel first layer (dcr_first_layer_fwd_ws_f32_dev) takes this model: ReLU, fp32 on the MI355X, hidden
    width 64 / 128, at most 16 classes; any input width since round 5 (W1 resident in LDS where it fits, streamed through it
    in K chunks otherwise: Cora 1,433, Citeseer 3,703).  ``DCR_FIRST_FUSED=0`` switches it off."""
    if not (_AGG_BACKEND == 'hip' and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and isinstance(act_fn, ReLU)):
        return False
    if os.environ.get('DCR_FIRST_FUSED', '1') == '0':
        return False
    return bool(_lib.lib().dcr_first_layer_fits(int(first.lin.weight.shape[1]), int(first.lin.weight.shape[0]), int(lin2.weight.shape[0])))


class SparseInput:
    """The node features as a sparse operand (round 5).  Planetoid features are row-normalised bags of words, ~0.9 % dense
    (experiment/data_loader.py reads them; bench.py generates that density): X·W1ᵀ over the non-zeros is ~100 x fewer products
    than the dense contraction of the propagated Â·X (which is ~4-5 % dense), so for such inputs the first layer keeps PyG's
    order of operations — lin first, then the aggregation — with X in CSR and, for the weight gradient, Xᵀ in CSR:
        forward   pre = Â·(X·W1ᵀ) + b1            two aggregations (dcr_spmm_csr_f32_dev), the first over X's non-zeros
        backward  dW1ᵀ = Xᵀ·(Âᵀ·dpre)            two more
    Built once per (x, graph) by ``GCNConv.sparse_input``."""

    def __init__(self, x):
        n, f = x.shape
        idx = x.nonzero()                                   # row-major order
        rows, cols = idx[:, 0], idx[:, 1]
        self.n, self.f, self.nnz = n, f, int(rows.numel())
        self.val = x[rows, cols].contiguous()
        self.rowptr = torch.zeros(n + 1, dtype=torch.int64, device=x.device)
        torch.cumsum(torch.bincount(rows, minlength=n), 0, out=self.rowptr[1:])
        self.col = cols.to(torch.int32).contiguous()
        order = torch.argsort(cols * n + rows)              # Xᵀ: by column, rows ascending inside one
        self.rowptr_t = torch.zeros(f + 1, dtype=torch.int64, device=x.device)
        torch.cumsum(torch.bincount(cols, minlength=f), 0, out=self.rowptr_t[1:])
        self.col_t = rows[order].to(torch.int32).contiguous()
        self.val_t = self.val[order].contiguous()


class _SparseFirstFn(torch.autograd.Function):
    """pre = Â·(X·W1ᵀ) + b1 with X sparse (``SparseInput``); see there."""

    @staticmethod
    def forward(ctx, w1, b1, xs, csr):
        w1t = w1.t().contiguous()                           # [F, H]: the rows the non-zeros of X gather
        h = spmm(xs.rowptr, xs.col, xs.val, w1t, xs.n)
        ctx.xs, ctx.csr, ctx.has_bias = xs, csr, b1 is not None
        return spmm(csr.rowptr, csr.col, csr.val, h, csr.n_rows, bias=b1)

    @staticmethod
    def backward(ctx, g):
        xs, csr = ctx.xs, ctx.csr
        g = g.contiguous()
        gw1 = gb1 = None
        if ctx.needs_input_grad[0]:
            dh = spmm(csr.rowptr_t, csr.col_t, csr.val_t, g, csr.n_cols)
            gw1 = spmm(xs.rowptr_t, xs.col_t, xs.val_t, dh, xs.f).t()    # [H, F] as a view of the [F, H] product
        if ctx.has_bias and ctx.needs_input_grad[1]:
            gb1 = _column_sums(g)
        return gw1, gb1, None, None


def sparse_input_density():
    """Largest share of non-zeros for which the first layer takes the sparse-input route (``DCR_SPARSE_X``, default 0.1;
    0 switches it off)."""
    try:
        return float(os.environ.get('DCR_SPARSE_X', '0.1'))
    except ValueError:
        return 0.1


class _Linear(torch.nn.Module):
    """torch_geometric.nn.dense.linear.Linear(in, out, bias=False, weight_initializer='glorot')."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = Parameter(torch.empty(out_channels, in_channels))
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.in_channels + self.out_channels))  # glorot
        with torch.no_grad():
            self.weight.uniform_(-a, a)

    def forward(self, x, bias=None):
        if _AGG_BACKEND == 'hip' and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2:
            return _LinearFn.apply(x, self.weight, bias)
        return torch.nn.functional.linear(x, self.weight, bias)


class GCNConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, add_self_loops=True, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.add_self_loops = add_self_loops
        self.lin = _Linear(in_channels, out_channels)
        if bias:
            self.bias = Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter('bias', None)
        self._cache_key = None
        self._cache_csr = None
        self._cache_ref = None   # the tensors the cache is keyed on (held: their storage cannot be recycled meanwhile)
        # Â·(X·Wᵀ) = (Â·X)·Wᵀ: when the layer's input is a constant of the run (the node features, for the first layer
        # of a GCN) Â·X is computed ONCE and the layer becomes a plain GEMM: no aggregation in the forward pass, none in
        # the backward pass, and in the data-parallel model no exchange step for this layer.  GCN switches it on for
        # layers[0]; a stand-alone GCNConv keeps PyG's order of operations.
        self.propagate_input_first = False
        self._ax_key = None
        self._ax = None
        self._ax_ref = None
        self._xs_key = self._xs = self._xs_ref = None
        self._rowsel = {}

    def reset_parameters(self):
        self.lin.reset_parameters()
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()
        self.invalidate()

    def propagated_input(self, x, csr, pad16=False):
        """Â·x, cached while x (same storage, same version) and the graph stay the same.  The cache holds a reference
        to the tensor it is keyed on: its storage cannot be freed and handed to another tensor while the entry lives,
        so an equal (address, version, shape) key always means the same values.  ``pad16``: the width rounded up to a
        multiple of 16 with zero columns (what the one-kernel first layer reads: 16-column MFMA steps, 16-byte pieces)."""
        key = (x.data_ptr(), x._version, tuple(x.shape), tuple(x.stride()), str(x.device), self._cache_key, bool(pad16))
        if key != self._ax_key:
            with torch.no_grad():
                xc = x.contiguous()
                pad = (-xc.shape[1]) % 16 if pad16 else 0
                if pad:
                    xc = torch.nn.functional.pad(xc, (0, pad))
                self._ax = spmm(csr.rowptr, csr.col, csr.val, xc, csr.n_rows)
            self._ax_key = key
            self._ax_ref = x
        return self._ax

    def sparse_input(self, x):
        """``SparseInput`` of x when the first layer should take the sparse route (few non-zeros, fp32 on the GPU, HIP backend),
        else None; decided and built once per tensor (same storage, same version: the tensor is held), one host sync."""
        thr = sparse_input_density()
        if not (thr > 0 and _AGG_BACKEND == 'hip' and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] >= 64
                and not x.requires_grad):
            return None
        key = (x.data_ptr(), x._version, tuple(x.shape), tuple(x.stride()), str(x.device), thr)
        if key != self._xs_key:
            dense = int(torch.count_nonzero(x))
            self._xs = SparseInput(x) if dense <= thr * x.numel() else None
            self._xs_key, self._xs_ref = key, x
        return self._xs

    def invalidate(self):
        """Drop the cached Â and Â·x (they are rebuilt at the next forward)."""
        self._cache_key = self._cache_csr = self._cache_ref = None
        self._ax_key = self._ax = self._ax_ref = None
        self._xs_key = self._xs = self._xs_ref = None
        self._rowsel = {}

    def row_selection(self, rows, csr):
        """``RowSelection`` of a split (boolean mask or index tensor), cached while the tensor (same storage, same
        version: held here) and the graph stay the same."""
        key = (rows.data_ptr(), rows._version, tuple(rows.shape), rows.dtype, str(rows.device), self._cache_key)
        hit = self._rowsel.get(key)
        if hit is None:
            if len(self._rowsel) >= 6:
                self._rowsel.pop(next(iter(self._rowsel)))
            hit = self._rowsel[key] = (RowSelection(csr, rows), rows)
        return hit[0]

    def norm_csr(self, edge_index, edge_weight, num_nodes):
        # (PyG 2.0.3 with cached=False renormalises at every call; same result, the graph is a constant of a training
        #  run.  The keyed tensors are held, see propagated_input.)
        key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), tuple(edge_index.stride()),
               int(num_nodes),
               None if edge_weight is None else (edge_weight.data_ptr(), edge_weight._version, tuple(edge_weight.shape)),
               str(edge_index.device))
        if key != self._cache_key:
            self._cache_csr = gcn_norm_csr(edge_index, edge_weight, num_nodes, self.add_self_loops)
            self._cache_key = key
            self._cache_ref = (edge_index, edge_weight)
        return self._cache_csr

    def forward(self, x, edge_index, edge_weight=None):
        csr = self.norm_csr(edge_index, edge_weight, x.shape[0])
        if self.propagate_input_first and not x.requires_grad and x.dtype == torch.float32:
            xs = self.sparse_input(x)
            if xs is not None:                                           # Â·(X·Wᵀ) + b over X's non-zeros (SparseInput)
                return _SparseFirstFn.apply(self.lin.weight, self.bias, xs, csr)
            return self.lin(self.propagated_input(x, csr), self.bias)   # (Â·X)·Wᵀ + b: one GEMM
        z = self.lin(x)                       # dense contraction on MFMA via the GEMM library
        return aggregate(z, self.bias, csr)   # sparse aggregation + bias: HIP kernel


class GCN(torch.nn.Module):
    """The reference's model (models/gcn.py:12-44) on the kernels of this package: GCNConv layers of widths
    [features] + hidden + [classes], ReLU and dropout between them, log-softmax at the end.  Attribute names, the
    two optimiser groups (weight decay on the first layer only, save_models.py:78-82) and the ``state_dict`` keys
    (``layers.{i}.bias``, ``layers.{i}.lin.weight``) are the reference's."""

    def __init__(self, dataset, hidden: List[int] = [64], dropout: float = 0.5):
        super().__init__()
        widths = [dataset.data.x.shape[1], *hidden, dataset.num_classes]
        self.layers = ModuleList([GCNConv(w_in, w_out) for w_in, w_out in zip(widths, widths[1:])])
        first = self.layers[0]
        first.propagate_input_first = True   # its input is data.x, constant over the run
        self.reg_params = list(first.parameters())
        self.non_reg_params = [p for conv in list(self.layers)[1:] for p in conv.parameters()]
        self.dropout = Dropout(p=dropout)
        self.act_fn = ReLU()

    def reset_parameters(self):
        for conv in self.layers:
            conv.reset_parameters()

    def _fused_first(self, data, want_train, want_eval):
        """(z_train, z_eval) of the SECOND layer's lin straight from Â·X (one kernel, _FirstLayerFn), or None when the
        shapes, the mode or the backend ask for the separate kernels: each operand then takes the route it would take alone,
        so training, evaluation and the one-pass epoch see the same numbers whichever of them asks."""
        first, second = self.layers[0], self.layers[1]
        x = data.x
        if not (first.propagate_input_first and not x.requires_grad and x.dtype == torch.float32 and x.is_cuda):
            return None
        p = self.dropout.p
        if want_train and not (self.dropout.training and 0.0 < p < 1.0):
            return None
        grads = torch.is_grad_enabled() and any(q.requires_grad for q in list(first.parameters()) + [second.lin.weight])
        if want_eval and not want_train and grads:
            return None                                   # evaluation mode WITH a gradient: the stock modules
        if not first_layer_fused_ok(x, self.act_fn, first, second.lin):
            return None
        if first.sparse_input(x) is not None:
            return None                                   # few non-zeros: Â·(X·W1ᵀ) over them (GCNConv.forward), then act_then_linear
        csr = first.norm_csr(data.edge_index, data.edge_attr, x.shape[0])
        ax = first.propagated_input(x, csr, pad16=True)
        if want_train:
            return _FirstLayerFn.apply(ax, first.lin.weight, first.bias, second.lin.weight, p, True, want_eval)
        with torch.no_grad():
            return _FirstLayerFn.apply(ax, first.lin.weight.detach(), None if first.bias is None else first.bias.detach(),
                                       second.lin.weight.detach(), 0.0, False, True)

    supports_rows = True   # forward(data, rows=...) / forward_pair(data, rows_train=..., rows_eval=...)

    def _walk(self, data, want_tr, want_ev, eval_grad, finish):
        """models/gcn.py:32-44 for the training operand (dropout on, autograd graph attached), the evaluation operand, or both
        in ONE traversal of the layers: the two differ only in the dropout between the layers, so the first layer's output is
        computed once (the evaluation operand is its detached copy) and every later aggregation serves both in one sweep of
        the graph.  The activation after a layer is computed together with the next layer's lin (``_fused_first``,
        ``_act_then_linear_pair``), each operand on the route it would take alone.  ``eval_grad``: gradients attach to an
        evaluation operand asked for alone (``forward`` in evaluation mode); otherwise that walk runs under ``torch.no_grad()``.
        Returns ``finish(conv, csr, z_tr, z_ev)``: the last layer, its Â and the operands of its aggregation (None: not
        wanted).  A one-layer model's only aggregation is inside its GCNConv: ``finish(None, None, o_tr, o_ev)`` on its outputs."""
        layers = list(self.layers)
        last = len(layers) - 1
        z_first = self._fused_first(data, want_tr, want_ev) if last > 0 else None
        with torch.set_grad_enabled(torch.is_grad_enabled() and (want_tr or eval_grad)):
            conv = csr = o_tr = o_ev = None
            if z_first is None:
                o = layers[0](data.x, data.edge_index, edge_weight=data.edge_attr)
                o_tr, o_ev = (o if want_tr else None), ((o.detach() if want_tr else o) if want_ev else None)
            z_tr, z_ev = o_tr, o_ev
            for depth, conv in enumerate(layers[1:], start=1):
                if z_first is not None:          # first layer, activation and this layer's lin came out of one kernel
                    (z_tr, z_ev), z_first = z_first, None
                else:
                    z_tr, z_ev = _act_then_linear_pair(o_tr, o_ev, self.act_fn, self.dropout, conv.lin, eval_grad)
                csr = conv.norm_csr(data.edge_index, data.edge_attr, (z_ev if z_tr is None else z_tr).shape[0])
                if depth < last:
                    o_tr, o_ev = _aggregate_wanted(z_tr, z_ev, conv.bias, csr)
        return finish(conv, csr, z_tr, z_ev)

    @staticmethod
    def _log_probs(rows_tr, rows_ev):
        """The finisher of ``forward`` / ``forward_pair``: the last aggregation at every row (no rows given) or at the rows
        asked for and nowhere else, then log_softmax; (training, evaluation) log-probabilities, None where not wanted."""
        def pick(t, r):      # (one-layer model)
            return t if t is None or r is None else t[r] if r.dtype == torch.bool else t.index_select(0, r)

        def finish(conv, csr, z_tr, z_ev):
            if conv is None:
                o_tr, o_ev = pick(z_tr, rows_tr), pick(z_ev, rows_ev)
            elif rows_tr is None and rows_ev is None:
                o_tr, o_ev = _aggregate_wanted(z_tr, z_ev, conv.bias, csr)
            else:
                sel_tr = None if z_tr is None else conv.row_selection(rows_tr, csr)
                sel_ev = None if z_ev is None else conv.row_selection(rows_ev, csr)
                if z_tr is not None and z_ev is not None:
                    o_tr, o_ev = _AggregateRowsPair.apply(z_tr, z_ev, conv.bias, csr, sel_tr, sel_ev)
                else:
                    o_tr = None if z_tr is None else aggregate_rows(z_tr, conv.bias, csr, sel_tr)
                    o_ev = None if z_ev is None else aggregate_rows(z_ev, conv.bias, csr, sel_ev)
                o_tr = None if z_tr is None else sel_tr.expanded(o_tr)
                o_ev = None if z_ev is None else sel_ev.expanded(o_ev)
            return tuple(None if o is None else torch.nn.functional.log_softmax(o, dim=1) for o in (o_tr, o_ev))
        return finish

    def forward(self, data, rows=None):
        # models/gcn.py:32-44.  rows (a boolean node mask or an index tensor): return the log-probabilities of those nodes
        # only, [len, C] in index order — what ``model(data)[rows]`` holds, value for value; the last aggregation is evaluated
        # at those rows and nowhere else.
        if self.training:
            return self._walk(data, True, False, True, self._log_probs(rows, None))[0]
        return self._walk(data, False, True, True, self._log_probs(None, rows))[1]

    def forward_pair(self, data, rows_train=None, rows_eval=None):
        """(training-mode log-probabilities with their autograd graph, evaluation-mode log-probabilities) of the SAME
        weights in one pass: what ``model.train(); model(data)`` and ``model.eval(); model(data)`` return, value for
        value (``_walk`` with both operands).  The validation forward of one epoch and the training forward of the next see
        the same weights (experiment/training_loop.py:25-26: train, then evaluate, then train again), which is what
        ``LaggedGraphedEpoch`` builds on.  Call in training mode.
        ``rows_train`` / ``rows_eval`` (both or neither): only those nodes' rows of the two outputs, as ``forward(data, rows)``."""
        if (rows_train is None) != (rows_eval is None):
            raise ValueError('rows_train and rows_eval go together')
        return self._walk(data, True, True, False, self._log_probs(rows_train, rows_eval))

    def forward_head(self, data, rows_train=None, y_train=None, rows_eval=None, y_eval=None):
        """(loss, correct) of one epoch's two readings of the model in ONE pass, without the log-probabilities in between:
        ``loss = F.nll_loss(model(data)[rows_train], y_train)`` in training mode (dropout on, autograd graph attached) and
        ``correct = (model(data)[rows_eval].argmax(1) == y_eval).sum()`` in evaluation mode, of the SAME weights (see
        ``forward_pair``).  Either half may be left out (rows_* = None): the training step alone, or the evaluation alone.
        Returns None when a shape, a mode or the backend asks for the separate kernels (the caller then takes the log-probabilities
        from ``forward`` / ``forward_pair``): two or more layers, row index tensors without repeats, at most 32 classes."""
        want_tr, want_ev = rows_train is not None, rows_eval is not None
        if len(self.layers) < 2 or not (want_tr or want_ev) or (want_tr and not self.training):
            return None
        last = self.layers[-1]
        # eligibility is decided before anything runs: a forward computed and then dropped would have drawn its dropout decisions
        # (the caller's stock forward draws again, so the run would differ from DCR_FUSED_HEAD=0) and, in a capture, left dead
        # kernels in the graph.  The last layer's Â and row selections are the ones its aggregation uses below (cached).
        csr_last = last.norm_csr(data.edge_index, data.edge_attr, data.x.shape[0])
        sel_tr = last.row_selection(rows_train, csr_last) if want_tr else None
        sel_ev = last.row_selection(rows_eval, csr_last) if want_ev else None
        if data.x.dtype != torch.float32 or not head_ok(last.lin.weight, sel_tr, sel_ev, last.out_channels):
            return None
        return self._walk(data, want_tr, want_ev, False, lambda conv, csr, z_tr, z_ev: _AggregateRowsHead.apply(
            z_tr, z_ev, conv.bias, csr, sel_tr, sel_ev, y_train, y_eval))


def dense_reference_logits(model, x, edge_index, num_nodes):
    """Dense fp64 restatement Â = D^-1/2 (A+I) D^-1/2, log_softmax(Â·relu(Â·X·W1ᵀ+b1)·W2ᵀ+b2) in eval mode —
    the build's own pin for GCNConv."""
    n = num_nodes
    A = torch.zeros((n, n), dtype=torch.float64, device=x.device)
    A[edge_index[1], edge_index[0]] = 1.0
    A = A + torch.eye(n, dtype=torch.float64, device=x.device)
    dinv = A.sum(1).pow(-0.5)
    Ah = dinv[:, None] * A * dinv[None, :]
    h = x.double()
    for i, layer in enumerate(model.layers):
        h = Ah @ (h @ layer.lin.weight.double().t()) + layer.bias.double()
        if i < len(model.layers) - 1:
            h = torch.relu(h)
    return torch.log_softmax(h, dim=1)


def smoke_gcn(edge_index, num_nodes, device='cuda:0'):
    from dcr.data import Data, Dataset
    torch.manual_seed(0)
    x = torch.randn(num_nodes, 32)
    y = torch.randint(0, 5, (num_nodes,))
    data = Data(x=x, edge_index=edge_index, y=y, num_nodes=num_nodes).to(device)
    model = GCN(Dataset(data, 5), hidden=[16], dropout=0.5).to(device)
    model.eval()
    got = model(data)
    want = dense_reference_logits(model, data.x, data.edge_index, num_nodes)
    err = (got.double() - want).abs().max().item()
    assert err < 1e-5, f'GCN logits differ from the dense reference by {err}'
    model.train()
    loss = torch.nn.functional.nll_loss(model(data), data.y)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    return err
