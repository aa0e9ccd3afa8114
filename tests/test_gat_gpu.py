"""The attention aggregation kernels (csrc/dcr_gat.hip) through the raw ABI, and the GAT model on them (models/gat.py), against
the dense fp64 restatement and the derived bounds of tests/gat_ref.py.  Every raw call writes into NaN-filled buffers and no NaN
may be left: every output element is written."""
import ctypes
import math
import os
import re

import pytest
import torch

import gat_ref
from conftest import PKG

pytestmark = pytest.mark.gpu

EINVAL = -1
NAN = float('nan')


def _const(name):
    src = open(os.path.join(PKG, 'csrc', 'dcr_gat.hip')).read()
    return int(re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, src).group(1))


GAT_LONG = _const('GAT_LONG')


@pytest.fixture(scope='module')
def lib():
    from dcr import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _view(t, ld=None, offset=0):
    """``t`` [n, w] copied into a row-major buffer of leading dimension ``ld`` that starts ``offset`` floats past a 256-byte
    aligned address, NaN around it."""
    n, w = t.shape
    ld = w if ld is None else ld
    buf = torch.full((n * ld + offset + 64,), NAN, dtype=torch.float32, device='cuda')
    v = buf[offset:offset + n * ld].view(n, ld)[:, :w]
    v.copy_(t)
    return v


def gather(lib, csr, z, s_src, s_dst, slope=0.2, ldo=None, off_o=0):
    n, heads = s_src.shape
    out = _view(torch.full((n, z.shape[1]), NAN), ldo, off_o)
    rec = torch.full((max(n * heads, 1), 2), NAN, dtype=torch.float32, device='cuda')
    rc = lib.dcr_gat_gather_f32_dev(csr.rowptr.data_ptr(), csr.col.data_ptr(), z.data_ptr(), s_src.data_ptr(), s_dst.data_ptr(),
                                    out.data_ptr(), rec.data_ptr(), n, heads, z.shape[1] // heads, z.stride(0), s_src.stride(0),
                                    out.stride(0), slope, _stream())
    assert rc == 0, lib.dcr_last_error()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(rec[:n * heads]).any())
    return out, rec


def expand(lib, csr, z, s_src, s_dst, out, rec, d_out, slope=0.2):
    """(dZ, dS_src, dS_dst) with the leading dimensions of z and s_src; ``d_out`` takes ``out``'s."""
    n, heads = s_src.shape
    d_out = _view(d_out, out.stride(0))
    dz = _view(torch.full((n, z.shape[1]), NAN), z.stride(0))
    ds_src = _view(torch.full((n, heads), NAN), s_src.stride(0))
    ds_dst = _view(torch.full((n, heads), NAN), s_src.stride(0))
    work_rec = torch.full((max(n * heads, 1), 4), NAN, dtype=torch.float32, device='cuda')
    work_g = torch.full((max(int(csr.rowptr[-1]) * heads, 1),), NAN, dtype=torch.float32, device='cuda')
    rc = lib.dcr_gat_expand_f32_dev(csr.rowptr.data_ptr(), csr.rowptr_t.data_ptr(), csr.col_t.data_ptr(), csr.slot_t.data_ptr(),
                                    z.data_ptr(), s_src.data_ptr(), s_dst.data_ptr(), out.data_ptr(), d_out.data_ptr(), rec.data_ptr(),
                                    dz.data_ptr(), ds_src.data_ptr(), ds_dst.data_ptr(), work_rec.data_ptr(), work_g.data_ptr(), n,
                                    heads, z.shape[1] // heads, z.stride(0), s_src.stride(0), out.stride(0), slope, _stream())
    assert rc == 0, lib.dcr_last_error()
    torch.cuda.synchronize()
    for t in (dz, ds_src, ds_dst):
        assert not bool(torch.isnan(t).any())                       # every element written, no memset needed
    return dz, ds_src, ds_dst


def both(lib, ei, n, loops, z, s_src, s_dst, d_out, slope=0.2):
    from models.gat import gat_csr
    csr = gat_csr(ei.cuda(), n, loops)
    zc, sc, dc = _view(z), _view(s_src), _view(s_dst)
    out, rec = gather(lib, csr, zc, sc, dc, slope)
    return (out,) + expand(lib, csr, zc, sc, dc, out, rec, d_out, slope)


def _int_operands(n, heads, c, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-8, 9, (n, heads * c), generator=g).float(), torch.zeros(n, heads), torch.zeros(n, heads),
            torch.randint(-4, 5, (n, heads * c), generator=g).float())


def _edge_graph():
    """Rows of GAT_LONG - 1, GAT_LONG and GAT_LONG + 1 slots with the added self-loop counted (rows 0, 1, 2), a hub above G·U
    slots (row 3: 600 sources), rows holding only their self-loop (the last ones), a duplicated column."""
    n = 640
    cols = []
    for row, k in ((0, GAT_LONG - 2), (1, GAT_LONG - 1), (2, GAT_LONG), (3, 600)):
        src = torch.arange(10, 10 + k)
        cols.append(torch.stack([src, torch.full((k,), row)]))
    cols.append(torch.tensor([[20, 21, 21], [5, 5, 5]]))
    return torch.cat(cols, 1), n


_EXACT = {}


def _exact_reference():
    if not _EXACT:
        ei, n = _edge_graph()
        _EXACT['ei'], _EXACT['n'] = ei, n
        _EXACT[True], _EXACT[False] = gat_ref.count_matrix(ei, n, True), gat_ref.count_matrix(ei, n, False)
    return _EXACT


@pytest.mark.parametrize('heads,c', gat_ref.EXACT_SHAPES)
def test_unit_weights_give_exact_quotients_and_gradients_within_bounds(lib, heads, c):
    """att_src = att_dst = 0: every weight is exp(0) = 1, O is the fp32 quotient of two exact integers, at the long-row threshold,
    on a hub, on self-loop-only rows.  The backward of the same call within the bounds."""
    ref = _exact_reference()
    ei, n, cnt = ref['ei'], ref['n'], ref[True]
    z, s_src, s_dst, d_out = _int_operands(n, heads, c, seed=heads * 1000 + c)
    assert cnt.sum(1)[:4].tolist() == [GAT_LONG - 1, GAT_LONG, GAT_LONG + 1, 601] and cnt.sum(1)[-1] == 1
    out, dz, ds_src, ds_dst = both(lib, ei, n, True, z, s_src, s_dst, d_out)
    total = (cnt @ z.double()).float()                                  # exact: integers below 2^24
    want = total.view(n, heads, c) / cnt.sum(1).float()[:, None, None]  # one correctly rounded fp32 division
    assert torch.equal(out.cpu().view(n, heads, c), want)
    assert torch.equal(out.cpu()[-1], z[-1])                            # a row holding only its self-loop
    _, w_dz, w_src, w_dst = gat_ref.aggregate_reference(z, s_src, s_dst, cnt, d_out)
    bound = gat_ref.bounds(z, s_src, s_dst, cnt, d_out)
    for key, got, wanted in (('dZ', dz, w_dz), ('dS_src', ds_src, w_src), ('dS_dst', ds_dst, w_dst)):
        assert gat_ref.worst_ratio(got.cpu(), wanted, bound[key]) <= 1.0, key


def test_empty_rows_small_n_and_one_node(lib):
    ref = _exact_reference()
    ei, n, cnt = ref['ei'], ref['n'], ref[False]
    z, s_src, s_dst, d_out = _int_operands(n, 2, 4, seed=3)
    out, dz, ds_src, ds_dst = both(lib, ei, n, False, z, s_src, s_dst, d_out)
    d = cnt.sum(1)
    assert torch.equal(out.cpu(), (cnt @ z.double()).float() / d.clamp(min=1).float()[:, None])
    empty = d == 0
    assert int(empty.sum()) > 500 and float(out.cpu()[empty].abs().max()) == 0.0 and float(ds_dst.cpu()[empty].abs().max()) == 0.0
    no_out = cnt.sum(0) == 0
    assert float(dz.cpu()[no_out].abs().max()) == 0.0 and float(ds_src.cpu()[no_out].abs().max()) == 0.0
    for nn, heads, c in ((3, 1, 4), (1, 1, 1), (1, 3, 5), (5, 8, 8)):          # n below one workgroup's units, n = 1
        ring = torch.arange(nn)
        e2 = torch.stack([ring, (ring + 1) % nn])
        z, s_src, s_dst, d_out = _int_operands(nn, heads, c, seed=nn)
        cnt2 = gat_ref.count_matrix(e2, nn, True)
        out, dz, ds_src, ds_dst = both(lib, e2, nn, True, z, s_src, s_dst, d_out)
        assert torch.equal(out.cpu(), ((cnt2 @ z.double()).float() / cnt2.sum(1).float()[:, None]))
        _, w_dz, w_src, w_dst = gat_ref.aggregate_reference(z, s_src, s_dst, cnt2, d_out)
        bound = gat_ref.bounds(z, s_src, s_dst, cnt2, d_out)
        for key, got, wanted in (('dZ', dz, w_dz), ('dS_src', ds_src, w_src), ('dS_dst', ds_dst, w_dst)):
            assert gat_ref.worst_ratio(got.cpu(), wanted, bound[key]) <= 1.0, (nn, key)


@pytest.mark.parametrize('heads,c', [(1, 4), (3, 6), (8, 8), (2, 64)])
def test_one_dominant_slot_and_the_subtracted_maximum(lib, heads, c):
    """One source of every row leads the others by 120 after the leaky step (positive pre): the others' weights underflow to
    exactly 0 and O[i] is that source's Z row; with +100 on every score the result is finite and the same bits."""
    from models.gat import gat_csr
    n_t, per = 150, 7                                                    # targets 0 .. 149, one row of 130 slots
    lead = torch.arange(n_t) + n_t                                       # sources 150 .. 299 lead (s_src = 120), 300 .. 449 do not
    rows, srcs = [], []
    for i in range(n_t):
        k = 129 if i == 7 else per
        others = 300 + (i + torch.arange(k)) % 150
        at = i % (k + 1)
        srcs.append(torch.cat([others[:at], lead[i:i + 1], others[at:]]))
        rows.append(torch.full((k + 1,), i))
    ei = torch.stack([torch.cat(srcs), torch.cat(rows)])
    n = 450
    g = torch.Generator().manual_seed(c)
    z = torch.randn(n, heads * c, generator=g)
    s_src = torch.zeros(n, heads)
    s_src[n_t:2 * n_t] = 120.0
    s_dst = torch.zeros(n, heads)
    csr = gat_csr(ei.cuda(), n, add_self_loops=False)
    out, _ = gather(lib, csr, _view(z), _view(s_src), _view(s_dst))
    assert torch.equal(out.cpu()[:n_t], z[lead])
    shifted, _ = gather(lib, csr, _view(z), _view(s_src + 100.0), _view(s_dst))
    assert bool(torch.isfinite(shifted).all()) and torch.equal(shifted, out)


@pytest.mark.parametrize('ld_pad,offset', [(0, 1), (0, 2), (1, 0), (2, 0), (2, 2)])
def test_narrowed_vec_gives_the_aligned_values(lib, ld_pad, offset):
    """Leading dimensions and pointer offsets of 4 and 8 bytes narrow VEC: the same exact quotients, gradients within twice the
    bound of the aligned call's."""
    from models.gat import gat_csr
    ref = _exact_reference()
    ei, n, cnt = ref['ei'], ref['n'], ref[True]
    heads, c = 2, 16
    z, s_src, s_dst, d_out = _int_operands(n, heads, c, seed=9)
    assert gat_ref.vec_lph(c, (heads * c + ld_pad,), (4 * offset,)) != gat_ref.vec_lph(c, (heads * c,), (0,))
    aligned = both(lib, ei, n, True, z, s_src, s_dst, d_out)
    csr = gat_csr(ei.cuda(), n, True)
    zc, sc, dc = _view(z, heads * c + ld_pad, offset), _view(s_src, heads + 1), _view(s_dst, heads + 1)
    out, rec = gather(lib, csr, zc, sc, dc, ldo=heads * c + ld_pad, off_o=offset)
    grads = expand(lib, csr, zc, sc, dc, out, rec, d_out)
    assert torch.equal(out, aligned[0])
    bound = gat_ref.bounds(z, s_src, s_dst, cnt, d_out)
    for key, got, wanted in zip(('dZ', 'dS_src', 'dS_dst'), grads, aligned[1:]):
        assert gat_ref.worst_ratio(got.cpu(), wanted.cpu().double(), 2 * bound[key]) <= 1.0, key


@pytest.mark.parametrize('name', gat_ref.FIXTURES)
def test_random_floats_within_the_derived_bounds_and_the_same_bits_twice(lib, name):
    ei, n, heads, c, loops, z, s_src, s_dst, d_out = gat_ref.fixture(name)
    cnt = gat_ref.count_matrix(ei, n, loops)
    want = gat_ref.aggregate_reference(z, s_src, s_dst, cnt, d_out)
    bound = gat_ref.bounds(z, s_src, s_dst, cnt, d_out)
    got = both(lib, ei, n, loops, z, s_src, s_dst, d_out)
    ratios = {key: gat_ref.worst_ratio(g.cpu(), w, bound[key]) for key, g, w in zip(('O', 'dZ', 'dS_src', 'dS_dst'), got, want)}
    print(f'GAT kernels, fixture {name!r}: largest error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    for key, ratio in ratios.items():
        assert ratio <= 1.0, (name, key, ratio)
    again = both(lib, ei, n, loops, z, s_src, s_dst, d_out)
    for a, b in zip(got, again):
        assert torch.equal(a, b)                                       # no atomics on floats: the same bits on every call


def test_argument_errors(lib):
    from models.gat import gat_csr
    ring = torch.arange(6)
    csr = gat_csr(torch.stack([ring, (ring + 1) % 6]).cuda(), 6)
    z, s, out, rec = (torch.full(shape, NAN, device='cuda') for shape in ((6, 8), (6, 2), (6, 8), (12, 2)))
    w4, wg = torch.full((12, 4), NAN, device='cuda'), torch.full((24,), NAN, device='cuda')

    def g(**kw):
        a = dict(rowptr=csr.rowptr.data_ptr(), col=csr.col.data_ptr(), z=z.data_ptr(), s_src=s.data_ptr(), s_dst=s.data_ptr(),
                 out=out.data_ptr(), rec=rec.data_ptr(), n=6, H=2, C=4, ldz=8, lds=2, ldo=8)
        a.update(kw)
        return lib.dcr_gat_gather_f32_dev(a['rowptr'], a['col'], a['z'], a['s_src'], a['s_dst'], a['out'], a['rec'], a['n'], a['H'],
                                          a['C'], a['ldz'], a['lds'], a['ldo'], 0.2, _stream())

    def e(**kw):
        a = dict(rowptr=csr.rowptr.data_ptr(), rowptr_t=csr.rowptr_t.data_ptr(), col_t=csr.col_t.data_ptr(), slot_t=csr.slot_t.data_ptr(),
                 z=z.data_ptr(), s_src=s.data_ptr(), s_dst=s.data_ptr(), out=out.data_ptr(), d_out=out.data_ptr(), rec=rec.data_ptr(),
                 dz=z.data_ptr(), ds_src=s.data_ptr(), ds_dst=s.data_ptr(), w4=w4.data_ptr(), wg=wg.data_ptr(), n=6, H=2, C=4, ldz=8,
                 lds=2, ldo=8)
        a.update(kw)
        return lib.dcr_gat_expand_f32_dev(a['rowptr'], a['rowptr_t'], a['col_t'], a['slot_t'], a['z'], a['s_src'], a['s_dst'], a['out'],
                                          a['d_out'], a['rec'], a['dz'], a['ds_src'], a['ds_dst'], a['w4'], a['wg'], a['n'], a['H'],
                                          a['C'], a['ldz'], a['lds'], a['ldo'], 0.2, _stream())

    for name in ('rowptr', 'col', 'z', 's_src', 's_dst', 'out', 'rec'):
        assert g(**{name: None}) == EINVAL, name
    for name in ('rowptr', 'rowptr_t', 'col_t', 'slot_t', 'z', 's_src', 's_dst', 'out', 'd_out', 'rec', 'dz', 'ds_src', 'ds_dst', 'w4', 'wg'):
        assert e(**{name: None}) == EINVAL, name
    for call in (g, e):
        for bad in (dict(n=-1), dict(H=0), dict(H=65), dict(C=0), dict(ldz=7), dict(ldo=7), dict(lds=1), dict(C=260, ldz=520, ldo=520),
                    dict(C=65, ldz=130, ldo=130)):
            assert call(**bad) == EINVAL, bad
    assert e(w4=w4.data_ptr() + 4) == EINVAL
    from dcr import _lib
    assert b'GAT' in _lib.lib().dcr_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(z).all()) and bool(torch.isnan(s).all())   # nothing was launched
    assert g(n=0) == 0 and e(n=0) == 0


# ---- the model ----------------------------------------------------------------------------------------------------------------
MODEL_TOL = 1e-5   # the project's tolerance for a two-layer model against its dense fp64 restatement (tests/test_gcn.py, test_rgcn_gpu.py)


def _planted(n=300, classes=3, seed=0):
    """A planted-partition graph: ``classes`` blocks, p_in = 0.08, p_out = 0.005, features = a noisy one-hot of the block."""
    from dcr.data import Data, Dataset
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(n) % classes
    p = torch.where(y[:, None] == y[None, :], 0.08, 0.005)
    a = torch.triu(torch.rand(n, n, generator=g) < p, 1)
    a = a | a.t()
    ei = a.nonzero().t().contiguous()
    x = torch.nn.functional.one_hot(y, classes).float() + 0.5 * torch.randn(n, classes, generator=g)
    x = torch.cat([x, torch.randn(n, 13, generator=g)], 1)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[torch.randperm(n, generator=g)[:n // 2]] = True
    data = Data(x=x, edge_index=ei, y=y, num_nodes=n, train_mask=mask, val_mask=~mask)
    return data.to('cuda'), Dataset(data, classes)


@pytest.fixture(scope='module')
def planted():
    from models.gat import GAT
    data, ds = _planted()
    torch.manual_seed(3)
    model = GAT(ds, hidden=[8], heads=8, output_heads=1, dropout=0.0).cuda()
    with torch.no_grad():
        for conv in model.layers:
            conv.bias.uniform_(-0.5, 0.5)
    return data, model


def test_model_matches_the_dense_restatement(planted):
    from models.gat import dense_reference_logits
    data, model = planted
    model.train()
    model.zero_grad()
    lp = model(data)
    torch.nn.functional.nll_loss(lp[data.train_mask], data.y[data.train_mask]).backward()
    want_lp, want_grad = gat_ref.model_reference(model, data.x, data.edge_index, data.y, data.train_mask)
    worst = max([float((lp.detach().double().cpu() - want_lp).abs().max())] +
                [float((p.grad.double().cpu() - want_grad[k]).abs().max()) for k, p in model.named_parameters()])
    print(f'GAT on the HIP kernels against the dense fp64 restatement: worst difference {worst:.3e}')
    assert (lp.detach().double().cpu() - want_lp).abs().max() < MODEL_TOL
    for k, p in model.named_parameters():
        assert (p.grad.double().cpu() - want_grad[k]).abs().max() < MODEL_TOL, k
    model.eval()
    with torch.no_grad():
        assert (dense_reference_logits(model, data.x, data.edge_index, data.num_nodes).cpu() - want_lp).abs().max() < 1e-10


def test_three_epochs_train(planted):
    import copy
    from experiment.training_loop import train, training_loop
    data, model = planted
    model = copy.deepcopy(model)
    optimizer = torch.optim.Adam([dict(params=model.reg_params, weight_decay=5e-4), dict(params=model.non_reg_params, weight_decay=0)], lr=0.01)
    losses = [float(train(model, optimizer, data)) for _ in range(3)]
    assert all(math.isfinite(v) for v in losses) and losses[0] > losses[1] > losses[2], losses
    model.dropout.p = 0.6
    assert training_loop(model, optimizer, data, 3, 10) is model
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_model_runs_on_fosr_and_digl_outputs(planted):
    from dcr.data import Dataset
    from models.gat import GAT, dense_reference_logits
    from rewiring.diffusion import digl
    from rewiring.fosr import fosr
    data, _ = planted
    for rewired in (fosr(data, 5), digl(data, alpha=0.15, k=16)):
        torch.manual_seed(4)
        model = GAT(Dataset(rewired, 3), hidden=[8], heads=4, dropout=0.0).cuda()
        model.eval()
        with torch.no_grad():
            lp = model(rewired)
            want = dense_reference_logits(model, rewired.x, rewired.edge_index, rewired.num_nodes)
        assert (lp.double() - want).abs().max() < MODEL_TOL
        model.train()
        torch.nn.functional.nll_loss(model(rewired)[rewired.train_mask], rewired.y[rewired.train_mask]).backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
