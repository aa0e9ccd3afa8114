"""Edge weights and self-loops already in the input, through every route Â takes on the GPU (the reference's loader always
sets ``edge_attr`` and its model passes it on).  The check is the float64 restatement of PyG 2.0.3 ``gcn_norm`` in
tests/gcn_fp64.py, built from the raw edge list: the aggregation entry points at widths that select every (LPR, VEC) template of
``spmm_dispatch`` (csrc/dcr_spmm.hip), the model's logits and one training step's gradients on every first-layer and head route, the captured
epochs against the eager loop, and unit weights against no weights."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from gcn_fp64 import gcn_logits, gcn_norm_fp64, hand_built_graph, propagate, weighted_powerlaw_graph

pytestmark = pytest.mark.gpu

# VEC 1 / 2 / 4 (odd, even, multiple of 4) x LPR 4 / 8 / 16 / 32 / 64 (block widths up to 4, 8, 16, 32 and above 32 lanes)
WIDTHS = [3, 7, 15, 31, 33, 6, 14, 30, 62, 130, 16, 32, 64, 128, 256]
_GRAPHS = {}


def _graph(name):
    if name not in _GRAPHS:
        ei, w, n = hand_built_graph() if name == 'hand_built' else weighted_powerlaw_graph()
        _GRAPHS[name] = (ei.cuda(), w.cuda(), n)
    return _GRAPHS[name]


def _check(got, want, scale, what):
    """|got - want| <= 2e-6 (|Â|·|B| + |bias|) elementwise: cancellation-aware, and exact where Â's row is zero."""
    err = (got.double() - want).abs()
    bad = err > 2e-6 * scale
    assert not bool(bad.any()), (what, err.max().item(), int(bad.sum()))


@pytest.mark.parametrize('graph', ['hand_built', 'powerlaw'])
def test_every_aggregation_entry_point_against_fp64(graph):
    from dcr import _lib
    from models import gcn
    ei, w, n = _graph(graph)
    csr = gcn.gcn_norm_csr(ei, w, n)
    src, dst, val = gcn_norm_fp64(ei, w, n)
    fwd, fwd_abs = (src, dst, val), (src, dst, val.abs())
    bwd, bwd_abs = (dst, src, val), (dst, src, val.abs())
    g = torch.Generator(device='cuda').manual_seed(11)
    rows_a = torch.cat([torch.tensor([0, 100, 96, 290, 291, n - 10], device='cuda'),
                        torch.randperm(n, device='cuda', generator=g)[:n // 3]]).unique()
    rows_b = torch.randperm(n, device='cuda', generator=g)[:n // 4].sort()[0]
    sel_a, sel_b = gcn.RowSelection(csr, rows_a), gcn.RowSelection(csr, rows_b)
    st = torch.cuda.current_stream().cuda_stream
    for f in WIDTHS:
        big = torch.randn(n, 2 * f + 3, device='cuda', generator=g)
        b2 = big[:, :2 * f].contiguous()
        bias = torch.randn(f, device='cuda', generator=g)
        b0, b1 = b2[:, :f], b2[:, f:]
        want = [propagate(fwd, t, n) + bias.double() for t in (b0, b1)]
        scale = [propagate(fwd_abs, t.abs(), n) + bias.double().abs() for t in (b0, b1)]
        # spmm (forward Â and backward Âᵀ)
        _check(gcn.spmm(csr.rowptr, csr.col, csr.val, b0.contiguous(), n, bias), want[0], scale[0], ('spmm', f))
        _check(gcn.spmm(csr.rowptr_t, csr.col_t, csr.val_t, b1.contiguous(), n), propagate(bwd, b1, n),
               propagate(bwd_abs, b1.abs(), n), ('spmm_t', f))
        # pair and pair_split
        pair = gcn.spmm_pair(csr.rowptr, csr.col, csr.val, b2, n, f, bias)
        _check(pair[:, :f], want[0], scale[0], ('pair0', f))
        _check(pair[:, f:], want[1], scale[1], ('pair1', f))
        s0, s1 = gcn.spmm_pair(csr.rowptr, csr.col, csr.val, b2, n, f, bias, split=True)
        assert torch.equal(s0, pair[:, :f]) and torch.equal(s1, pair[:, f:]), ('pair_split', f)
        # rows, on a column block (stride 2f) and on a slice at an odd offset (4 bytes off 16-byte alignment: no vector loads)
        _check(gcn.spmm_rows(csr, sel_a, b1, bias), want[1][rows_a], scale[1][rows_a], ('rows', f))
        odd = big[:, 1:1 + f]
        assert odd.data_ptr() % 16 == 4 and odd.stride(0) == 2 * f + 3
        want_odd = propagate(fwd, odd, n) + bias.double()
        scale_odd = propagate(fwd_abs, odd.abs(), n) + bias.double().abs()
        _check(gcn.spmm_rows(csr, sel_a, odd, bias), want_odd[rows_a], scale_odd[rows_a], ('rows_odd', f))
        # rows2: rows_a of Â·B0, then rows_b of Â·B1, one launch
        both = torch.cat([rows_a, rows_b]).contiguous()
        out = torch.empty(both.numel(), f, device='cuda')
        _lib.check(_lib.lib().dcr_spmm_csr_rows2_f32_dev(csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(), both.data_ptr(),
                                                         rows_a.numel(), both.numel(), b2.data_ptr(), f, out.data_ptr(), f, 2 * f, f,
                                                         bias.data_ptr(), 0, ctypes.c_void_p(st)))
        _check(out[:rows_a.numel()], want[0][rows_a], scale[0][rows_a], ('rows2_a', f))
        _check(out[rows_a.numel():], want[1][rows_b], scale[1][rows_b], ('rows2_b', f))
        if f % 4:   # rows2 on the odd slice (both operands unaligned)
            out2 = torch.empty(both.numel(), f, device='cuda')
            _lib.check(_lib.lib().dcr_spmm_csr_rows2_f32_dev(csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.val.data_ptr(), both.data_ptr(),
                                                             rows_a.numel(), both.numel(), odd.data_ptr(), 1, out2.data_ptr(), f, 2 * f + 3,
                                                             f, bias.data_ptr(), 0, ctypes.c_void_p(st)))
            want_odd2 = propagate(fwd, big[:, 2:2 + f], n) + bias.double()
            _check(out2[:rows_a.numel()], want_odd[rows_a], scale_odd[rows_a], ('rows2_odd_a', f))
            _check(out2[rows_a.numel():], want_odd2[rows_b], propagate(fwd_abs, big[:, 2:2 + f].abs(), n)[rows_b] + bias.double().abs(),
                   ('rows2_odd_b', f))
    if graph == 'hand_built':   # the zero-degree node: the bias alone, exactly
        assert torch.equal(gcn.spmm(csr.rowptr, csr.col, csr.val, b0.contiguous(), n, bias)[290], bias)


@pytest.mark.parametrize('b_off2', [7, 1])
def test_rows2_second_operand_an_odd_number_of_floats_on(b_off2):
    """dcr_spmm_csr_rows2_f32_dev at a width, leading dimensions and a first operand that take 8-byte loads, the second operand
    an odd number of floats further on: only 4-byte aligned, so the call must fall back to scalar loads, not fail and not load
    float2 from it.  Small integers and dyadic weights: every fp32 operation is exact, the fp64 product bit for bit."""
    import numpy as np
    from dcr import _lib
    lib = _lib.lib()
    f, ldb, n = 6, 14, 48
    rng = np.random.default_rng(50 + b_off2)
    lengths = [int(rng.integers(0, 9)) for _ in range(n)]
    lengths[0], lengths[5], lengths[6], lengths[9] = 200, 97, 96, 0          # two hub rows, the longest short row, an empty one
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = rng.integers(0, n, rowptr[-1]).astype(np.int32)
    val = (0.5 ** rng.integers(0, 4, rowptr[-1])).astype(np.float32)
    A = np.zeros((n, n))
    np.add.at(A, (np.repeat(np.arange(n), lengths), col), val.astype(np.float64))
    Bv = np.full((n, ldb), np.nan, dtype=np.float32)                         # NaN in the columns neither operand holds
    for off in (0, b_off2):
        Bv[:, off:off + f] = rng.integers(-4, 5, (n, f))
    bias_v = rng.integers(-3, 4, f).astype(np.float32)
    rows_a = np.array([0, 3, 5, 6, 9, 20, 47], dtype=np.int64)
    rows_b = np.array([5, 0, 1, 2, 9, 6, 30, 31, 46], dtype=np.int64)
    both = np.concatenate([rows_a, rows_b])
    d_rowptr, d_col, d_val, d_B, d_bias, d_both = (torch.from_numpy(a).cuda() for a in (rowptr, col, val, Bv, bias_v, both))
    assert d_B.data_ptr() % 16 == 0 and f % 4 == 2 and ldb % 2 == 0 and b_off2 % 2 == 1 and b_off2 + f <= ldb
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rows2(n_first, n_sel, B, off2, width=f, ld=ldb):
        out = torch.full((n_sel, width), float('nan'), device='cuda')
        rc = lib.dcr_spmm_csr_rows2_f32_dev(d_rowptr.data_ptr(), d_col.data_ptr(), d_val.data_ptr(), d_both.data_ptr(), n_first, n_sel,
                                            B.data_ptr(), off2, out.data_ptr(), width, ld, width, d_bias.data_ptr(), 0, st)
        return rc, out

    rc, out = rows2(rows_a.size, both.size, d_B, b_off2)
    assert rc == 0, rc
    want = np.concatenate([(A @ Bv[:, :f].astype(np.float64))[rows_a], (A @ Bv[:, b_off2:b_off2 + f].astype(np.float64))[rows_b]]) + bias_v
    assert out.cpu().numpy().tobytes() == (want + 0.0).astype(np.float32).tobytes()
    # the second list empty: the second operand is never read, the call is dcr_spmm_csr_rows_f32_dev (random floats)
    R = torch.randn(n, ldb, device='cuda', generator=torch.Generator(device='cuda').manual_seed(b_off2))
    rc, out = rows2(both.size, both.size, R, b_off2)
    assert rc == 0, rc
    one = torch.full((both.size, f), float('nan'), device='cuda')
    rc = lib.dcr_spmm_csr_rows_f32_dev(d_rowptr.data_ptr(), d_col.data_ptr(), d_val.data_ptr(), d_both.data_ptr(), both.size, R.data_ptr(),
                                       one.data_ptr(), f, ldb, f, d_bias.data_ptr(), 0, st)
    assert rc == 0 and bool(torch.isfinite(one).all()) and torch.equal(out, one)
    # a width that takes 16-byte loads still refuses a second operand that breaks them
    rc, out = rows2(rows_a.size, both.size, R, b_off2, width=4)
    assert rc == -1 and b'16 bytes' in lib.dcr_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def _model_case(ei, w, n, seed=3):
    from dcr.data import Data, Dataset
    from models.gcn import GCN
    g = torch.Generator(device='cuda').manual_seed(5)
    x = torch.rand(n, 96, device='cuda', generator=g)
    x = x * (x < 0.06)                     # ~6 % non-zeros: the sparse-input route where DCR_SPARSE_X allows it
    y = torch.randint(0, 7, (n,), device='cuda', generator=g)
    train_rows = torch.nonzero(torch.rand(n, device='cuda', generator=g) < 0.4).flatten()
    data = Data(x=x, edge_index=ei, edge_attr=w, y=y, num_nodes=n)
    torch.manual_seed(seed)
    model = GCN(Dataset(data, 7), hidden=[64], dropout=0.5).cuda()
    with torch.no_grad():
        model.layers[0].bias.uniform_(-0.1, 0.1)
        model.layers[1].bias.uniform_(-0.1, 0.1)
    return model, data, train_rows


def _eval_and_step(ei, w, n):
    """(eval logits, training-step loss, {name: grad}, the activation pattern of the step) of a fresh model."""
    from models import gcn
    from models.gcn import _ReluDropoutFn
    model, data, rows = _model_case(ei, w, n)
    model.eval()
    with torch.no_grad():
        logits = model(data)
    model.train()
    ctr = gcn._dropout_counter(data.x.device)
    c0 = ctr.clone()
    y_tr = data.y[rows].contiguous()
    head = model.forward_head(data, rows_train=rows, y_train=y_tr)
    assert (head is not None) == (os.environ.get('DCR_FUSED_HEAD', '1') != '0')
    loss = head[0] if head is not None else F.nll_loss(model(data, rows=rows), y_tr)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    # the product's activation pattern: the sign of its float32 pre-activation, the keep mask of dropout call c0
    with torch.no_grad():
        pre = model.layers[0](data.x, ei, edge_weight=w)
    ctr.copy_(c0)
    keep = _ReluDropoutFn.apply(torch.ones_like(pre), 0.5) != 0
    assert int(ctr.item()) == int(c0.item()) + 1
    return model, data, rows, logits, loss.detach(), grads, ((pre > 0) & keep).double() / 0.5


@pytest.mark.parametrize('first_fused', ['1', '0'])
@pytest.mark.parametrize('sparse_x', ['0.1', '0'])
@pytest.mark.parametrize('fused_head', ['1', '0'])
@pytest.mark.parametrize('graph', ['hand_built', 'powerlaw'])
def test_weighted_model_logits_and_training_step_against_fp64(graph, first_fused, sparse_x, fused_head, monkeypatch):
    from models import gcn
    monkeypatch.setenv('DCR_FIRST_FUSED', first_fused)
    monkeypatch.setenv('DCR_SPARSE_X', sparse_x)
    monkeypatch.setenv('DCR_FUSED_HEAD', fused_head)
    ei, w, n = _graph(graph)
    # the first-layer route that actually ran: the sparse-input one when DCR_SPARSE_X allows it (whatever DCR_FIRST_FUSED says),
    # else the one-kernel first layer when DCR_FIRST_FUSED allows it, else the separate kernels
    calls = {gcn._FirstLayerFn: 0, gcn._SparseFirstFn: 0}
    for fn in calls:
        real = fn.apply
        monkeypatch.setattr(fn, 'apply', staticmethod(lambda *a, _fn=fn, _real=real: calls.__setitem__(_fn, calls[_fn] + 1) or _real(*a)))
    model, data, rows, logits, loss, grads, pattern = _eval_and_step(ei, w, n)
    ran = 'sparse' if calls[gcn._SparseFirstFn] else 'one-kernel' if calls[gcn._FirstLayerFn] else 'separate'
    assert ran == ('sparse' if sparse_x != '0' else 'one-kernel' if first_fused == '1' else 'separate'), (ran, calls)
    assert not (calls[gcn._SparseFirstFn] and calls[gcn._FirstLayerFn]), calls
    ref = [(l.lin.weight.detach().double().requires_grad_(), l.bias.detach().double().requires_grad_()) for l in model.layers]
    with torch.no_grad():
        want = gcn_logits(ref, data.x, ei, n, edge_weight=w)
    assert (logits.double() - want).abs().max().item() < 1e-5
    out = gcn_logits(ref, data.x, ei, n, edge_weight=w, patterns=[pattern])[rows]
    want_loss = F.nll_loss(out, data.y[rows])
    want_loss.backward()
    assert abs(loss.item() - want_loss.item()) <= 1e-5 * max(1.0, abs(want_loss.item()))
    for i, (rw, rb) in enumerate(ref):
        for name, r in ((f'layers.{i}.lin.weight', rw), (f'layers.{i}.bias', rb)):
            err, scale = (grads[name].double() - r.grad).abs().max().item(), r.grad.abs().max().item()
            assert err <= 1e-5 * scale, (name, err, scale)
    # unit weights are no weights: the same bits on this route
    ctr = gcn._dropout_counter(data.x.device)
    c0 = ctr.clone()
    a = _eval_and_step(ei, torch.ones_like(w), n)
    ctr.copy_(c0)                          # (the same dropout decisions for both)
    b = _eval_and_step(ei, None, n)
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    for k in a[5]:
        assert torch.equal(a[5][k], b[5][k]), k


def _epoch_case():
    from dcr import synthetic
    from dcr.data import Data, Dataset
    from models.gcn import GCN
    dev = torch.device('cuda')
    ei_np, n = synthetic.powerlaw_graph(1500, 3, seed=5)
    ei = torch.from_numpy(ei_np).to(dev)
    loops = torch.arange(0, n, 40, device=dev)
    ei = torch.cat([ei, torch.stack([loops, loops])], 1)
    w = 0.1 + 3.0 * torch.rand(ei.shape[1], device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(n, 96, device=dev, generator=g)
    y = torch.randint(0, 5, (n,), device=dev, generator=g)
    r = torch.rand(n, device=dev, generator=g)
    data = Data(x=x, edge_index=ei, edge_attr=w, y=y, num_nodes=n, train_mask=r < 0.3, val_mask=(r >= 0.3) & (r < 0.6))

    def build():
        torch.manual_seed(3)
        model = GCN(Dataset(data, 5), hidden=[32], dropout=0.0).to(dev)
        opt = torch.optim.Adam([{'params': model.non_reg_params, 'weight_decay': 0},
                                {'params': model.reg_params, 'weight_decay': 5e-3}], lr=0.02, capturable=True)
        return model, opt
    return data, build


def test_captured_epochs_on_a_weighted_graph_equal_eager_epochs():
    """GraphedEpoch (two graphs per epoch) and LaggedGraphedEpoch (one graph, the accuracy one step late) on a weighted graph
    with self-loops: the weights and accuracies of the eager train / evaluate loop, bit for bit (dropout off)."""
    from experiment.training_loop import GraphedEpoch, LaggedGraphedEpoch, evaluate, make_epoch, train
    data, build = _epoch_case()
    m1, o1 = build()
    accs = []
    for _ in range(10):
        train(m1, o1, data)
        accs.append(evaluate(m1, data, test=False)['val_acc'])
    m2, o2 = build()
    epoch = make_epoch(m2, o2, data)
    assert isinstance(epoch, GraphedEpoch)
    assert [epoch() for _ in range(10)] == accs
    assert epoch.train_graph is not None
    m3, o3 = build()
    lag = make_epoch(m3, o3, data, lagged=True)
    assert isinstance(lag, LaggedGraphedEpoch)
    lagged = [lag.step().item() / lag.n_val for _ in range(10)]
    assert lag.graph is not None
    assert lagged[1:] == accs[:-1] and lag.accuracy_now() == accs[-1]
    for m in (m2, m3):
        for (k1, v1), (k2, v2) in zip(m1.state_dict().items(), m.state_dict().items()):
            assert k1 == k2 and torch.equal(v1, v2), k1


def test_weighted_normalisation_is_the_same_bits_every_time():
    """gcn_norm_csr on the GPU: the degrees of a weighted graph summed in a fixed order (two calls, two models, one Â)."""
    from models.gcn import gcn_norm_csr
    ei, w, n = _graph('powerlaw')
    a, b = gcn_norm_csr(ei, w, n), gcn_norm_csr(ei, w, n)
    for k in ('rowptr', 'col', 'val', 'rowptr_t', 'col_t', 'val_t'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
