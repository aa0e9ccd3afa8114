"""Attention dropout of the GAT kernels (the DROP instantiations of csrc/dcr_gat.hip) through the raw ABI and through models/gat.py:
the p = 0 paths keep their bits, the keep set of every slot bit for bit against the host stream of tests/dropout_ref.py in both
sweeps, random floats within the derived bounds of tests/gat_dropout_ref.py, the call counter, and the model."""
import ctypes

import numpy as np
import pytest
import torch

import dropout_ref
import gat_dropout_ref as R
import gat_ref
from test_gat_gpu import NAN, _planted, _stream, _view, expand, gather

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope='module')
def lib():
    from dcr import _lib
    return _lib.lib()


def _word(value):
    return torch.tensor([value], dtype=torch.int64, device='cuda')


def gather_drop(lib, csr, z, s_src, s_dst, p, seed, offset=0, offset_dev=None, slope=0.2):
    """(O, rec, offset_used) of dcr_gat_gather_drop_f32_dev into NaN-filled buffers; ``offset_dev`` an int or None (null)."""
    n, heads = s_src.shape
    out = _view(torch.full((n, z.shape[1]), NAN))
    rec = torch.full((max(n * heads, 1), 2), NAN, dtype=torch.float32, device='cuda')
    used = _word(-1)
    ctr = None if offset_dev is None else _word(offset_dev if offset_dev < 2 ** 63 else offset_dev - 2 ** 64)
    rc = lib.dcr_gat_gather_drop_f32_dev(csr.rowptr.data_ptr(), csr.col.data_ptr(), z.data_ptr(), s_src.data_ptr(), s_dst.data_ptr(),
                                         out.data_ptr(), rec.data_ptr(), n, heads, z.shape[1] // heads, z.stride(0), s_src.stride(0),
                                         out.stride(0), slope, _stream(), csr.nnz, p, seed, offset,
                                         None if ctr is None else ctr.data_ptr(), used.data_ptr())
    assert rc == 0, lib.dcr_last_error()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(rec[:n * heads]).any())
    return out, rec, used


def expand_drop(lib, csr, z, s_src, s_dst, out, rec, d_out, p, seed, used, slope=0.2):
    n, heads = s_src.shape
    d_out = _view(d_out, out.stride(0))
    dz = _view(torch.full((n, z.shape[1]), NAN), z.stride(0))
    ds_src = _view(torch.full((n, heads), NAN), s_src.stride(0))
    ds_dst = _view(torch.full((n, heads), NAN), s_src.stride(0))
    work_rec = torch.full((max(n * heads, 1), 4), NAN, dtype=torch.float32, device='cuda')
    work_g = torch.full((max(csr.nnz * heads, 1),), NAN, dtype=torch.float32, device='cuda')
    rc = lib.dcr_gat_expand_drop_f32_dev(csr.rowptr.data_ptr(), csr.rowptr_t.data_ptr(), csr.col_t.data_ptr(), csr.slot_t.data_ptr(),
                                         z.data_ptr(), s_src.data_ptr(), s_dst.data_ptr(), out.data_ptr(), d_out.data_ptr(),
                                         rec.data_ptr(), dz.data_ptr(), ds_src.data_ptr(), ds_dst.data_ptr(), work_rec.data_ptr(),
                                         work_g.data_ptr(), n, heads, z.shape[1] // heads, z.stride(0), s_src.stride(0), out.stride(0),
                                         slope, _stream(), csr.nnz, p, seed, used.data_ptr())
    assert rc == 0, lib.dcr_last_error()
    torch.cuda.synchronize()
    for t in (dz, ds_src, ds_dst):
        assert not bool(torch.isnan(t).any())
    return dz, ds_src, ds_dst


def both_drop(lib, csr, z, s_src, s_dst, d_out, p, seed, offset=0, offset_dev=None):
    zc, sc, dc = _view(z), _view(s_src), _view(s_dst)
    out, rec, used = gather_drop(lib, csr, zc, sc, dc, p, seed, offset, offset_dev)
    return (out, rec, used) + expand_drop(lib, csr, zc, sc, dc, out, rec, d_out, p, seed, used)


def _csr(ei, n, loops):
    from models.gat import gat_csr
    return gat_csr(ei.cuda(), n, loops)


_FIX = {}


def _fixture(name):
    """The fixture, its slots, count matrix and CSR, computed once."""
    if name not in _FIX:
        ei, n, heads, c, loops, z, s_src, s_dst, d_out = gat_ref.fixture(name)
        rows, cols, rowptr, slot_t = R.slots(ei, n, loops)
        _FIX[name] = dict(ei=ei, n=n, heads=heads, c=c, loops=loops, z=z, s_src=s_src, s_dst=s_dst, d_out=d_out, rows=rows, cols=cols,
                          rowptr=rowptr, cnt=gat_ref.count_matrix(ei, n, loops), csr=_csr(ei, n, loops))
    return _FIX[name]


# ---- 1, 2: the paths without a mask keep their bits ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', gat_ref.FIXTURES)
def test_not_training_takes_the_kernels_without_dropout(name):
    from models.gat import gat_aggregate
    f = _fixture(name)
    results = []
    for extra in ({}, dict(attn_dropout=0.5, training=False)):
        leaves = [t.cuda().requires_grad_(True) for t in (f['z'], f['s_src'], f['s_dst'])]
        out = gat_aggregate(*leaves, f['csr'], 0.2, **extra)
        rec = out.grad_fn.saved_tensors[4]
        grads = torch.autograd.grad(out, leaves, f['d_out'].cuda())
        results.append((out.detach(), rec) + grads)
    for a, b in zip(*results):
        assert torch.equal(a, b)


@pytest.mark.parametrize('name', gat_ref.FIXTURES)
def test_p_zero_through_the_new_entry_points_is_the_old_bits(lib, name):
    f = _fixture(name)
    csr = f['csr']
    zc, sc, dc = _view(f['z']), _view(f['s_src']), _view(f['s_dst'])
    out, rec = gather(lib, csr, zc, sc, dc)
    grads = expand(lib, csr, zc, sc, dc, out, rec, f['d_out'])
    got = both_drop(lib, csr, f['z'], f['s_src'], f['s_dst'], f['d_out'], 0.0, R.SEEDS[0], 0, 7)
    assert int(got[2]) == 7
    for a, b in zip((out, rec) + grads, got[:2] + got[3:]):
        assert torch.equal(a, b)


# ---- 3, 4: exact keep sets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', R.SEEDS)
@pytest.mark.parametrize('offset_dev', R.OFFSETS)
@pytest.mark.parametrize('heads,c', [(1, 8), (3, 6), (8, 8), (2, 5)])
def test_exact_keep_sets_forward_and_backward(lib, heads, c, offset_dev, seed):
    """p = 0.5, scores zero, power-of-two rows: O·d / 2 is the integer whose bits are the kept sources of the row, dZ / 2 the one
    whose bits are the kept targets of the source, both the host stream's, slot by slot; with Z = 0 the score gradients are 0."""
    ei, n, lengths = R.block_graph(c)
    csr = _csr(ei, n, False)
    nnz = sum(lengths)
    assert csr.nnz == nnz
    offset = 3
    dec = R.decisions(nnz, heads, 0.5, seed, dropout_ref.stream_offset(offset, offset_dev))
    zeros = torch.zeros(n, heads)
    z, d_out = R.bit_values(n, heads, c), R.bit_gradients(n, heads, c, lengths)
    out, _, used = gather_drop(lib, csr, _view(z), _view(zeros), _view(zeros), 0.5, seed, offset, offset_dev)
    assert int(used) == offset + offset_dev
    d = torch.tensor(lengths, dtype=torch.float64)
    got = out.cpu().double().view(n, heads, c)[:len(lengths)] * d[:, None, None] / 2
    assert torch.equal(got, torch.from_numpy(R.keep_sets_forward(lengths, heads, c, dec)).double())
    assert float(out.cpu()[len(lengths):].abs().max()) == 0.0                                      # rows without a slot
    z0 = torch.zeros(n, heads * c)
    got = both_drop(lib, csr, z0, zeros, zeros, d_out, 0.5, seed, offset, offset_dev)
    dz, ds_src, ds_dst = got[3:]
    want = torch.from_numpy(R.keep_sets_backward(lengths, n, heads, dec)).double()
    assert torch.equal(dz.cpu().double().view(n, heads, c)[:, :, 0] / 2, want)
    assert float(dz.cpu().view(n, heads, c)[:, :, 1:].abs().max()) == 0.0
    assert float(ds_src.abs().max()) == 0.0 and float(ds_dst.abs().max()) == 0.0


def test_null_offset_dev_and_argument_errors(lib):
    ei, n, lengths = R.block_graph(8)
    csr = _csr(ei, n, False)
    zeros = torch.zeros(n, 1)
    z = R.bit_values(n, 1, 8)
    zc, sc = _view(z), _view(zeros)
    a, _, used = gather_drop(lib, csr, zc, sc, sc, 0.5, R.SEEDS[0], 11, None)
    b, rec, _ = gather_drop(lib, csr, zc, sc, sc, 0.5, R.SEEDS[0], 5, 6)
    assert int(used) == 11 and torch.equal(a, b)
    out = torch.full((n, 8), NAN, device='cuda')
    used = _word(-1)

    def g(p=0.5, nnz=csr.nnz, used_ptr=used.data_ptr()):
        return lib.dcr_gat_gather_drop_f32_dev(csr.rowptr.data_ptr(), csr.col.data_ptr(), zc.data_ptr(), sc.data_ptr(), sc.data_ptr(),
                                               out.data_ptr(), rec.data_ptr(), n, 1, 8, 8, 1, 8, 0.2, _stream(), nnz, p, 1, 0, None, used_ptr)

    def e(p=0.5, nnz=csr.nnz, used_ptr=used.data_ptr()):
        w4, wg = torch.empty((n, 4), device='cuda'), torch.empty(csr.nnz, device='cuda')
        return lib.dcr_gat_expand_drop_f32_dev(csr.rowptr.data_ptr(), csr.rowptr_t.data_ptr(), csr.col_t.data_ptr(), csr.slot_t.data_ptr(),
                                               zc.data_ptr(), sc.data_ptr(), sc.data_ptr(), a.data_ptr(), a.data_ptr(), rec.data_ptr(),
                                               out.data_ptr(), out.data_ptr(), out.data_ptr(), w4.data_ptr(), wg.data_ptr(), n, 1, 8, 8, 1,
                                               8, 0.2, _stream(), nnz, p, 1, used_ptr)

    for call in (g, e):
        for bad in (dict(p=1.0), dict(p=-0.25), dict(p=float('nan')), dict(p=2.0), dict(nnz=-1), dict(used_ptr=None)):
            assert call(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and int(used) == -1                                        # nothing was launched


# ---- 5: random floats ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', R.RANDOM_PS)
@pytest.mark.parametrize('name', gat_ref.FIXTURES)
def test_random_floats_within_the_derived_bounds(lib, name, p):
    f = _fixture(name)
    seed, off = R.SEEDS[1], 9
    dec = R.decisions(f['csr'].nnz, f['heads'], p, seed, off)
    want = R.aggregate_reference(f['z'], f['s_src'], f['s_dst'], f['rows'], f['cols'], R.keep_weights(dec, p), f['d_out'])
    bound = R.bounds(f['z'], f['s_src'], f['s_dst'], f['cnt'], f['d_out'], p)
    got = both_drop(lib, f['csr'], f['z'], f['s_src'], f['s_dst'], f['d_out'], p, seed, 4, 5)
    assert int(got[2]) == off
    ratios = {key: gat_ref.worst_ratio(g.cpu(), w, bound[key]) for key, g, w in zip(('O', 'dZ', 'dS_src', 'dS_dst'), (got[0],) + got[3:], want)}
    print(f'GAT kernels with attention dropout {p}, fixture {name!r}: largest error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    for key, ratio in ratios.items():
        assert ratio <= 1.0, (name, p, key, ratio)


# ---- 6: determinism and the call counter ----------------------------------------------------------------------------------------
@pytest.fixture
def counter():
    from models.gcn import _dropout_counter
    ctr = _dropout_counter(torch.device('cuda', torch.cuda.current_device()))
    before = ctr.clone()
    yield ctr
    ctr.copy_(before)


def _train_call(f, p):
    from models.gat import gat_aggregate
    leaves = [t.cuda().requires_grad_(True) for t in (f['z'], f['s_src'], f['s_dst'])]
    out = gat_aggregate(*leaves, f['csr'], 0.2, attn_dropout=p, training=True)
    return (out.detach(),) + torch.autograd.grad(out, leaves, f['d_out'].cuda())


def test_same_counter_same_bits_and_every_call_steps_it(lib, counter):
    f = _fixture('all hubs')
    torch.manual_seed(77)
    counter.fill_(1000)
    first = _train_call(f, 0.5)
    assert int(counter) == 1001
    second = _train_call(f, 0.5)
    assert int(counter) == 1002
    counter.fill_(1000)
    again = _train_call(f, 0.5)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert not torch.equal(first[0], second[0]) and not torch.equal(first[1], second[1])
    # the model path draws what the raw call draws at (initial_seed, counter): the host's mask, within the bounds
    dec = R.decisions(f['csr'].nnz, f['heads'], 0.5, 77, 1000)
    want = R.aggregate_reference(f['z'], f['s_src'], f['s_dst'], f['rows'], f['cols'], R.keep_weights(dec, 0.5), f['d_out'])
    bound = R.bounds(f['z'], f['s_src'], f['s_dst'], f['cnt'], f['d_out'], 0.5)
    for key, g, w in zip(('O', 'dZ', 'dS_src', 'dS_dst'), first, want):
        assert gat_ref.worst_ratio(g.cpu(), w, bound[key]) <= 1.0, key


def test_kept_fraction_of_all_hubs(lib):
    """Z = 1 and zero scores: O[i, h, :]·d / 2 counts the kept slots of (row, head) at p = 0.5.  Per (row, head) the host's count,
    and over the 13,000 x 3 slots within 4 standard deviations of 1 − threshold / 65536."""
    f = _fixture('all hubs')
    n, heads, c = f['n'], f['heads'], f['c']
    nnz = f['csr'].nnz
    assert nnz == 13000 and heads == 3
    zeros = torch.zeros(n, heads)
    out, _, _ = gather_drop(lib, f['csr'], _view(torch.ones(n, heads * c)), _view(zeros), _view(zeros), 0.5, R.SEEDS[0], 0, 41)
    counts = (out.cpu().double().view(n, heads, c)[:, :, 0] * 100 / 2).round().long()
    dec = torch.from_numpy(R.decisions(nnz, heads, 0.5, R.SEEDS[0], 41))
    assert torch.equal(counts, torch.zeros(n, heads, dtype=torch.int64).index_add(0, f['rows'], dec.long()))
    q = 1.0 - dropout_ref.threshold(0.5) / 65536.0
    frac = float(counts.sum()) / (nnz * heads)
    assert abs(frac - q) <= 4 * (q * (1 - q) / (nnz * heads)) ** 0.5, frac


# ---- 7: the model ---------------------------------------------------------------------------------------------------------------
def _model(ds):
    from models.gat import GAT
    torch.manual_seed(3)
    return GAT(ds, hidden=[8], heads=8, output_heads=1, dropout=0.6, attn_dropout=0.6, input_dropout=0.6).cuda()


def test_model_trains_with_both_dropouts_and_repeats_from_a_seed(counter):
    from models.gat import dense_reference_logits
    data, ds = _planted()
    finals = []
    for _ in range(2):
        model = _model(ds)
        torch.manual_seed(5)
        counter.zero_()
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        for step in range(5):
            opt.zero_grad()
            torch.nn.functional.nll_loss(model(data)[data.train_mask], data.y[data.train_mask]).backward()
            if step == 0:
                assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in model.parameters())
            opt.step()
        assert int(counter) == 5 * 2                                    # one mask per layer and step, no other draw in this model
        finals.append([p.detach().clone() for p in model.parameters()])
    for a, b in zip(*finals):
        assert torch.equal(a, b)
    model.eval()
    with torch.no_grad():
        err = (model(data).double() - dense_reference_logits(model, data.x, data.edge_index, data.num_nodes)).abs().max()
    assert err < 1e-4, float(err)
