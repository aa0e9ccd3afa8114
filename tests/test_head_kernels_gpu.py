"""The loss head at its edges: dcr_head_fwd_f32_dev / dcr_head_bwd_f32_dev (through the C ABI and through _AggregateRowsHead)
and the separate kernels of the DCR_FUSED_HEAD=0 route (dcr_nll_picked_mean_*, dcr_count_argmax_equal_f32_dev) against the
float64 NLL of tests/gcn_fp64.py.  Through the C ABI the grid covers every class-count template (8 / 16 / 32) with partial
vectors, one row to ~300,000 rows (one workgroup, a full 256-workgroup grid whose threads walk several rows, and the closing
workgroup that adds up to 256 partials), contiguous, row-strided and 4-byte-misaligned operands (the scalar load path), and
train-only, eval-only and both-halves calls; through _AggregateRowsHead, every class count at up to 65,537 rows per half.
Two calls in a row give the same bits: the closing reductions run in a fixed order whoever arrives last."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from gcn_fp64 import gcn_norm_fp64, nll_fp64, propagate

pytestmark = pytest.mark.gpu

CLASSES = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32]
ROWS = [1, 255, 256, 257, 65536, 65537, 300_001]
LAYOUTS = ['contiguous', 'strided', 'misaligned']
SENTINEL = 1234.5


def _operand(m, c, layout, g, nan=True):
    """(o [m, c] view, leading dimension, the buffer it lives in) with ties (and a NaN) planted in a few rows."""
    ld = c + 3 if layout == 'strided' else c
    off = 1 if layout == 'misaligned' else 0
    buf = torch.randn(off + m * ld + 16, device='cuda', generator=g)
    o = buf[off:off + m * ld].view(m, ld)[:, :c]
    if m >= 8 and c >= 2:
        o[1, :] = o[1, 0]                           # every entry equal: the first maximum
        o[3, c - 1] = o[3, 0] = o[3].max() + 1      # a tie of the first and the last column
        if nan:
            o[5, c // 2] = float('nan')             # a NaN counts as the maximum (torch.max)
    assert o.stride(0) == ld and (o.data_ptr() % 16 == 4) == (layout == 'misaligned')
    return o, ld, buf


def _workspace():
    from models import gcn
    return gcn._head_workspace(torch.device('cuda', 0), torch.cuda.current_stream().cuda_stream)


def _fwd(o_tr, y_tr, o_ev, y_ev, c):
    from dcr import _lib
    ws = _workspace()
    loss = torch.full((), SENTINEL, device='cuda')
    cnt = torch.full((), -1, dtype=torch.int64, device='cuda')
    m_tr = 0 if o_tr is None else o_tr.shape[0]
    m_ev = 0 if o_ev is None else o_ev.shape[0]
    _lib.check(_lib.lib().dcr_head_fwd_f32_dev(
        o_tr.data_ptr() if m_tr else None, o_tr.stride(0) if m_tr else c, y_tr.data_ptr() if m_tr else None, m_tr,
        o_ev.data_ptr() if m_ev else None, o_ev.stride(0) if m_ev else c, y_ev.data_ptr() if m_ev else None, m_ev, c,
        loss.data_ptr() if m_tr else None, cnt.data_ptr() if m_ev else None, ws.data_ptr(), ws.numel() * 8,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return loss, cnt


def _bwd(o_tr, y_tr, c, g, misaligned):
    """(grad [m, c], bias gradient, the grad buffer): the buffer is m * ld + 16 floats of SENTINEL, so a write past the
    [m, c] block stays inside it and shows."""
    from dcr import _lib
    ws = _workspace()
    m, ld = o_tr.shape[0], o_tr.stride(0)
    off = 1 if misaligned else 0
    buf = torch.full((off + m * ld + 16,), SENTINEL, device='cuda')
    gb = torch.full((c,), SENTINEL, device='cuda')
    _lib.check(_lib.lib().dcr_head_bwd_f32_dev(o_tr.data_ptr(), ld, y_tr.data_ptr(), m, c, g.data_ptr(), buf[off:].data_ptr(),
                                               gb.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return buf[off:off + m * c].view(m, c), gb, (buf[:off], buf[off + m * c:])


def _expected_count(o, y):
    return int(o.max(1)[1].eq(y).sum())


@pytest.mark.parametrize('c', CLASSES)
def test_head_kernels_c_abi_against_fp64(c):
    g = torch.Generator(device='cuda').manual_seed(100 + c)
    up = torch.tensor(1.5, device='cuda')                    # d loss from above (scales the gradient)
    for layout in LAYOUTS:
        for k, m in enumerate(ROWS):
            o_tr, _, _ = _operand(m, c, layout, g, nan=False)   # (the loss of a NaN row is NaN on both sides)
            y_tr = torch.randint(0, c, (m,), device='cuda', generator=g)
            m_ev = ROWS[(k + 3) % len(ROWS)]
            o_ev, _, _ = _operand(m_ev, c, layout, g)
            y_ev = torch.randint(0, c, (m_ev,), device='cuda', generator=g)
            ctx = (c, layout, m, m_ev)
            want_loss, want_grad, want_gb = nll_fp64(o_tr, y_tr)
            want_cnt = _expected_count(o_ev, y_ev)
            loss, cnt = _fwd(o_tr, y_tr, o_ev, y_ev, c)
            assert abs(loss.item() - want_loss.item()) <= 2e-6 * max(1.0, abs(want_loss.item())), ctx
            assert cnt.item() == want_cnt, ctx
            loss2, cnt2 = _fwd(o_tr, y_tr, o_ev, y_ev, c)
            assert torch.equal(loss, loss2) and torch.equal(cnt, cnt2), ctx
            loss_tr, cnt_tr = _fwd(o_tr, y_tr, None, None, c)
            assert torch.equal(loss_tr, loss) and cnt_tr.item() == -1, ctx
            loss_ev, cnt_ev = _fwd(None, None, o_ev, y_ev, c)
            assert torch.equal(cnt_ev, cnt) and loss_ev.item() == SENTINEL, ctx
            grad, gb, tails = _bwd(o_tr, y_tr, c, up, layout == 'misaligned')
            want_grad, want_gb = want_grad * 1.5, want_gb * 1.5
            assert all(bool((t == SENTINEL).all()) for t in tails), ctx
            assert (grad.double() - want_grad).abs().max().item() <= 1e-6 * 1.5 / m, ctx
            bound = 5e-6 * want_grad.abs().sum(0) + 1e-12
            assert bool(((gb.double() - want_gb).abs() <= bound).all()), (ctx, (gb.double() - want_gb).abs().max().item())
            grad2, gb2, _ = _bwd(o_tr, y_tr, c, up, layout == 'misaligned')
            assert torch.equal(grad, grad2) and torch.equal(gb, gb2), ctx
            del o_tr, o_ev, grad, grad2, want_grad


@pytest.mark.parametrize('m', ROWS)
def test_separate_loss_and_count_kernels_against_fp64(m):
    """The DCR_FUSED_HEAD=0 route: dcr_nll_picked_mean_* on log-probabilities, dcr_count_argmax_equal_f32_dev on them."""
    from experiment.training_loop import _PickedMean, _count_correct
    g = torch.Generator(device='cuda').manual_seed(m)
    for c in (1, 3, 8, 17, 32):
        o, _, _ = _operand(m, c, 'contiguous', g)
        o = o.contiguous()
        y = torch.randint(0, c, (m,), device='cuda', generator=g)
        assert _count_correct(o, y).item() == _expected_count(o, y), (m, c)
        o = torch.where(torch.isnan(o), torch.zeros_like(o), o)
        want_loss, _, _ = nll_fp64(o, y)
        a = o.clone().requires_grad_(True)
        loss = _PickedMean.apply(F.log_softmax(a, dim=1), y)
        assert abs(loss.item() - want_loss.item()) <= 2e-6 * max(1.0, abs(want_loss.item())), (m, c)
        assert torch.equal(loss.detach(), _PickedMean.apply(F.log_softmax(o, dim=1), y))
        lp = F.log_softmax(o, dim=1).requires_grad_(True)
        _PickedMean.apply(lp, y).backward()
        lp2 = lp.detach().clone().requires_grad_(True)
        F.nll_loss(lp2, y).backward()
        assert torch.equal(lp.grad, lp2.grad), (m, c)


def _ring(n):
    i = torch.arange(n, device='cuda')
    j = (i + 1) % n
    k = (i * 7 + 3) % n
    return torch.stack([torch.cat([i, j, i]), torch.cat([j, i, k])])


@pytest.mark.parametrize('c', CLASSES)
def test_aggregate_rows_head_against_fp64(c):
    """_AggregateRowsHead (aggregation at the selected rows + the head, models/gcn.py): loss, count, dZ and the bias gradient
    against Â·Z + b and the NLL in float64, with both halves, at a training-row count past one workgroup and past 65,536."""
    from models.gcn import RowSelection, _AggregateRowsHead, gcn_norm_csr
    n = 70_000
    ei = _ring(n)
    w = 0.5 + torch.rand(ei.shape[1], device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    csr = gcn_norm_csr(ei, w, n)
    norm = gcn_norm_fp64(ei, w, n)
    g = torch.Generator(device='cuda').manual_seed(c)
    for m_tr, m_ev in ((257, 65_537), (65_537, 300)):
        perm = torch.randperm(n, device='cuda', generator=g)
        rows_tr, rows_ev = perm[:m_tr].sort()[0], perm[m_tr:m_tr + m_ev]
        s_tr, s_ev = RowSelection(csr, rows_tr), RowSelection(csr, rows_ev)
        z_tr = torch.randn(n, c, device='cuda', generator=g).requires_grad_(True)
        z_ev = torch.randn(n, c, device='cuda', generator=g)
        bias = torch.randn(c, device='cuda', generator=g).requires_grad_(True)
        y_tr = torch.randint(0, c, (m_tr,), device='cuda', generator=g)
        y_ev = torch.randint(0, c, (m_ev,), device='cuda', generator=g)
        loss, cnt = _AggregateRowsHead.apply(z_tr, z_ev, bias, csr, s_tr, s_ev, y_tr, y_ev)
        loss.backward()
        o_tr = propagate(norm, z_tr.detach(), n)[rows_tr] + bias.detach().double()
        o_ev = (propagate(norm, z_ev, n) + bias.detach().double())[rows_ev]
        want_loss, want_grad, want_gb = nll_fp64(o_tr, y_tr)
        assert abs(loss.item() - want_loss.item()) <= 2e-6 * max(1.0, abs(want_loss.item())), (c, m_tr)
        margin = o_ev.topk(min(2, c), dim=1)[0]
        clear = (margin[:, 0] - margin[:, -1] > 1e-4) if c > 1 else torch.ones(m_ev, dtype=torch.bool, device='cuda')
        # (a row whose two largest outputs are within float32 rounding of each other may go either way: the count is bounded)
        cnt_ev_only = _AggregateRowsHead.apply(None, z_ev, bias.detach(), csr, None, s_ev, None, y_ev)[1]
        assert torch.equal(cnt_ev_only, cnt)
        want_clear = int((o_ev.argmax(1).eq(y_ev) & clear).sum())
        assert want_clear <= cnt.item() <= want_clear + int((~clear).sum()), (c, m_tr)
        grad_full = torch.zeros(n, c, dtype=torch.float64, device='cuda')
        grad_full[rows_tr] = want_grad
        src, dst, val = norm
        want_dz = propagate((dst, src, val), grad_full, n)
        scale_dz = propagate((dst, src, val.abs()), grad_full.abs(), n)
        assert bool(((z_tr.grad.double() - want_dz).abs() <= 2e-6 * scale_dz + 1e-12).all()), (c, m_tr)
        assert bool(((bias.grad.double() - want_gb).abs() <= 5e-6 * want_grad.abs().sum(0) + 1e-12).all()), (c, m_tr)


def _wide_case(n_cls, dropout=0.5):
    from dcr import synthetic
    from dcr.data import Data, Dataset
    from models.gcn import GCN
    dev = torch.device('cuda')
    ei_np, n = synthetic.powerlaw_graph(1500, 3, seed=5)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(n, 96, device=dev, generator=g)
    y = torch.randint(0, n_cls, (n,), device=dev, generator=g)
    r = torch.rand(n, device=dev, generator=g)
    data = Data(x=x, edge_index=torch.from_numpy(ei_np).to(dev), y=y, num_nodes=n, train_mask=r < 0.3,
                val_mask=(r >= 0.3) & (r < 0.6))
    torch.manual_seed(3)
    model = GCN(Dataset(data, n_cls), hidden=[32], dropout=dropout).to(dev)
    opt = torch.optim.Adam([{'params': model.non_reg_params, 'weight_decay': 0},
                            {'params': model.reg_params, 'weight_decay': 5e-3}], lr=0.02, capturable=True)
    return model, opt, data


@pytest.mark.parametrize('n_cls', [33, 40])
def test_more_than_32_classes_train_as_without_the_fused_head(n_cls, monkeypatch):
    """A model wider than the head kernels decides so before anything runs: 5 epochs of train() and of GraphedEpoch give the
    parameters of DCR_FUSED_HEAD=0 bit for bit, and the dropout counter advances by the same amount (one forward per step)."""
    from experiment.training_loop import GraphedEpoch, make_epoch, train
    from models import gcn

    def run(fused, graphed):
        monkeypatch.setenv('DCR_FUSED_HEAD', fused)
        model, opt, data = _wide_case(n_cls)
        ctr = gcn._dropout_counter(data.x.device)
        ctr.zero_()
        if graphed:
            epoch = make_epoch(model, opt, data)
            assert isinstance(epoch, GraphedEpoch)
            for _ in range(5):
                epoch()
            assert epoch.train_graph is not None
        else:
            for _ in range(5):
                train(model, opt, data)
        torch.cuda.synchronize()
        return [p.detach().clone() for p in model.parameters()], int(ctr.item())
    for graphed in (False, True):
        p_on, c_on = run('1', graphed)
        p_off, c_off = run('0', graphed)
        assert c_on == c_off == 5, (graphed, c_on, c_off)
        for a, b in zip(p_on, p_off):
            assert torch.equal(a, b), graphed
    # forward_head itself: None, and nothing drawn
    monkeypatch.setenv('DCR_FUSED_HEAD', '1')
    model, _, data = _wide_case(n_cls)
    model.train()
    ctr = gcn._dropout_counter(data.x.device)
    c0 = int(ctr.item())
    rows = data.train_mask.nonzero().squeeze(1)
    assert model.forward_head(data, rows_train=rows, y_train=data.y[rows].contiguous()) is None
    assert int(ctr.item()) == c0


def test_label_check_is_not_fooled_by_another_tensor_at_the_same_address_and_version():
    """experiment/training_loop.py::_labels_in_range caches its verdict per label tensor.  A second tensor over the same memory,
    at the same version and shape, that holds ignore_index (-100) labels must be checked afresh: train()'s loss is then
    F.nll_loss's, which leaves those rows out of the mean (the head kernel would divide by all of them)."""
    from experiment.training_loop import train
    model, opt, data = _wide_case(5, dropout=0.0)
    y1 = data.y.clone()
    for _ in range(20):
        y1.add_(0)                                      # (a version the second tensor can reach)
    data.y = y1
    train(model, opt, data)                             # in range: the fused head, verdict cached
    y2 = torch.empty(0, dtype=torch.int64, device='cuda').set_(y1.untyped_storage(), 0, y1.shape)
    drop = data.train_mask & (torch.rand(y1.shape[0], device='cuda', generator=torch.Generator(device='cuda').manual_seed(2)) < 0.3)
    y2[drop] = -100
    while y2._version < y1._version:
        y2.add_(0)
    assert y2.data_ptr() == y1.data_ptr() and y2._version == y1._version and y2.shape == y1.shape and y2 is not y1
    assert int(drop.sum()) > 0 and int((y2 == -100).sum()) == int(drop.sum())
    data.y = y2
    model.train()
    with torch.no_grad():
        want = F.nll_loss(model(data, rows=data.train_mask), y2[data.train_mask]).item()
    got = train(model, opt, data)
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
