"""GAT without a GPU: the attention CSR on a hand-built graph, the plain-torch backend of models/gat.py against the dense fp64
restatement of tests/gat_ref.py, gradcheck, the state dict, the call surface, and the guard on the bounds the GPU tests apply.
The torch aggregation is selected EXPLICITLY; the product default is the HIP kernels and refuses CPU tensors."""
import os
import re

import pytest
import torch

import gat_ref
from conftest import PKG, REPO


@pytest.fixture
def torch_backend():
    from models import gcn
    gcn.set_aggregate_backend('torch')
    yield
    gcn.set_aggregate_backend('hip')


# 12 nodes: (1 -> 0) twice, an input self-loop 3 -> 3, node 11 isolated, node 10 only a source
HAND = torch.tensor([[1, 2, 1, 3, 4, 3, 5, 6, 7, 8, 9, 10, 0, 2, 5],
                     [0, 0, 0, 0, 1, 3, 4, 5, 6, 7, 8, 9, 2, 9, 0]])
N = 12


def _rows(rowptr):
    return torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr[1:] - rowptr[:-1])


def _operands(n, heads, c, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, heads * c, generator=g, dtype=dtype), torch.randn(n, heads, generator=g, dtype=dtype),
            torch.randn(n, heads, generator=g, dtype=dtype))


def test_attn_csr_slots_and_self_loop_semantics():
    from models.gat import gat_csr
    csr = gat_csr(HAND, N, add_self_loops=True)
    assert csr.rowptr.dtype == torch.int64 and csr.col.dtype == torch.int32 and csr.slot_t.dtype == torch.int64
    # row 0: the input's columns in input order (the duplicate twice), the added self-loop last
    assert csr.col[csr.rowptr[0]:csr.rowptr[1]].tolist() == [1, 2, 1, 3, 5, 0]
    # row 3: the input self-loop is removed and exactly one is added
    assert csr.col[csr.rowptr[3]:csr.rowptr[4]].tolist() == [3]
    assert csr.col[csr.rowptr[11]:csr.rowptr[12]].tolist() == [11]               # the isolated node holds its self-loop
    assert int(csr.rowptr[-1]) == HAND.shape[1] - 1 + N
    bare = gat_csr(HAND, N, add_self_loops=False)
    assert bare.col[bare.rowptr[3]:bare.rowptr[4]].tolist() == [3]               # kept as an ordinary slot
    assert int(bare.rowptr[11]) == int(bare.rowptr[12]) and int(bare.rowptr[10]) == int(bare.rowptr[11])   # empty rows
    assert int(bare.rowptr[-1]) == HAND.shape[1]
    for c in (csr, bare):
        e = int(c.rowptr[-1])
        fwd = list(zip(c.col[:e].tolist(), _rows(c.rowptr).tolist()))            # (source, target) per slot
        bwd = list(zip(_rows(c.rowptr_t).tolist(), c.col_t[:e].tolist()))
        assert [fwd[k] for k in c.slot_t[:e].tolist()] == bwd                    # the slot map
        assert sorted(c.slot_t[:e].tolist()) == list(range(e))
        assert (gat_ref.count_matrix(HAND, N, c is csr) == torch.zeros(N, N, dtype=torch.float64).index_put_(
            (_rows(c.rowptr), c.col[:e].long()), torch.ones(e, dtype=torch.float64), accumulate=True)).all()
    empty = gat_csr(torch.zeros((2, 0), dtype=torch.int64), 3, add_self_loops=False)
    assert empty.rowptr.tolist() == [0, 0, 0, 0] and empty.col.numel() == 1 and empty.col_t.numel() == 1 and empty.slot_t.numel() == 1


@pytest.mark.parametrize('loops', [True, False])
def test_torch_backend_matches_dense_restatement(torch_backend, loops):
    from models.gat import gat_aggregate, gat_csr
    z, s_src, s_dst = _operands(N, 3, 4)
    got = gat_aggregate(z, s_src, s_dst, gat_csr(HAND, N, loops))
    want = gat_ref.aggregate(z, s_src, s_dst, gat_ref.count_matrix(HAND, N, loops))
    assert (got - want).abs().max() < 1e-13
    if not loops:
        assert float(got[10].abs().max()) == 0.0 and float(got[11].abs().max()) == 0.0


def test_torch_backend_gradcheck_and_empty_rows(torch_backend):
    from models.gat import gat_aggregate, gat_csr
    csr = gat_csr(HAND, N, add_self_loops=False)
    ops = [t.requires_grad_(True) for t in _operands(N, 2, 3, seed=1)]
    assert torch.autograd.gradcheck(lambda a, b, c: gat_aggregate(a, b, c, csr), ops, eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda a, b, c: gat_aggregate(a, b, c, gat_csr(HAND, N), 0.3), ops, eps=1e-6, atol=1e-7)
    out = gat_aggregate(*ops, csr)
    out.backward(torch.ones_like(out))
    assert all(bool(torch.isfinite(t.grad).all()) for t in ops)
    assert float(ops[2].grad[11].abs().max()) == 0.0 and float(ops[2].grad[10].abs().max()) == 0.0     # rows without a slot
    assert float(ops[0].grad[11].abs().max()) == 0.0 and float(ops[1].grad[11].abs().max()) == 0.0     # the isolated node
    d_out = torch.ones_like(out)
    _, dz, dsrc, ddst = gat_ref.aggregate_reference(ops[0], ops[1], ops[2], gat_ref.count_matrix(HAND, N, False), d_out)
    for got, want in zip((t.grad for t in ops), (dz, dsrc, ddst)):
        assert (got - want).abs().max() < 1e-12


def _toy(n=40, f=10, classes=4, seed=0):
    from dcr import synthetic
    from dcr.data import Data, Dataset
    ei_np, _ = synthetic.powerlaw_graph(n - 1, 3, seed=seed)
    g = torch.Generator().manual_seed(seed)
    ei = torch.from_numpy(ei_np)
    ei = torch.cat([ei, ei[:, :5], torch.tensor([[2], [2]])], 1)
    x = torch.randn(n, f, generator=g)
    y = torch.randint(0, classes, (n,), generator=g)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[torch.randperm(n, generator=g)[:n // 2]] = True
    data = Data(x=x, edge_index=ei, y=y, num_nodes=n, train_mask=mask, val_mask=~mask)
    return data, Dataset(data, classes)


def test_model_on_torch_backend_matches_dense_restatement(torch_backend):
    from models.gat import GAT, dense_reference_logits
    data, ds = _toy()
    torch.manual_seed(1)
    model = GAT(ds, hidden=[6], heads=3, output_heads=2, dropout=0.0)
    with torch.no_grad():
        for conv in model.layers:
            conv.bias.uniform_(-0.5, 0.5)
    model.train()
    lp = model(data)
    torch.nn.functional.nll_loss(lp[data.train_mask], data.y[data.train_mask]).backward()
    want_lp, want_grad = gat_ref.model_reference(model, data.x, data.edge_index, data.y, data.train_mask)
    assert (lp.detach().double() - want_lp).abs().max() < 1e-5
    for name, p in model.named_parameters():
        assert p.grad is not None and (p.grad.double() - want_grad[name]).abs().max() < 1e-5, name
    model.eval()
    with torch.no_grad():
        assert (dense_reference_logits(model, data.x, data.edge_index, data.num_nodes) - want_lp).abs().max() < 1e-12


def test_state_dict_and_surface(torch_backend):
    from models.gat import GAT, GATConv
    data, ds = _toy()
    m = GAT(ds, hidden=[8], heads=8, output_heads=1, dropout=0.6)
    sd = m.state_dict()
    assert list(sd.keys()) == ['layers.0.att_src', 'layers.0.att_dst', 'layers.0.bias', 'layers.0.lin.weight',
                               'layers.1.att_src', 'layers.1.att_dst', 'layers.1.bias', 'layers.1.lin.weight']
    assert sd['layers.0.lin.weight'].shape == (64, 10) and sd['layers.0.att_src'].shape == (1, 8, 8) and sd['layers.0.bias'].shape == (64,)
    assert sd['layers.1.lin.weight'].shape == (4, 64) and sd['layers.1.att_dst'].shape == (1, 1, 4) and sd['layers.1.bias'].shape == (4,)
    assert {id(p) for p in m.reg_params} == {id(p) for p in m.layers[0].parameters()}
    assert {id(p) for p in m.non_reg_params} == {id(p) for p in m.layers[1].parameters()}
    a_w, a_att = (6.0 / (10 + 64)) ** 0.5, (6.0 / (8 + 8)) ** 0.5
    assert a_w / 2 < float(sd['layers.0.lin.weight'].abs().max()) <= a_w and a_att / 2 < float(sd['layers.0.att_src'].abs().max()) <= a_att
    assert float(sd['layers.0.bias'].abs().sum()) == 0.0
    m2 = GAT(ds, hidden=[8], heads=8)
    m2.load_state_dict(sd)
    m.reset_parameters()
    assert m(data).shape == (40, 4)
    assert isinstance(m.act_fn, torch.nn.ELU) and m.layers[1].concat is False and m.layers[0].concat is True
    with pytest.raises(NotImplementedError, match='attention coefficients'):
        GATConv(5, 3, heads=2, dropout=0.1)
    with pytest.raises(ValueError):
        GATConv(5, 3, heads=65)
    assert list(GATConv(5, 3, heads=2, bias=False).state_dict().keys()) == ['att_src', 'att_dst', 'lin.weight']


def test_concat_false_averages_the_heads(torch_backend):
    from models.gat import GATConv
    data, _ = _toy()
    torch.manual_seed(2)
    cat = GATConv(10, 5, heads=3, concat=True)
    mean = GATConv(10, 5, heads=3, concat=False)
    mean.load_state_dict({**cat.state_dict(), 'bias': torch.arange(5.0)})
    with torch.no_grad():
        a, b = cat(data.x, data.edge_index), mean(data.x, data.edge_index)
    assert mean.bias.shape == (5,) and b.shape == (40, 5)
    assert (b - (a.view(40, 3, 5).mean(1) + torch.arange(5.0))).abs().max() < 1e-6


def test_layer_caches_its_csr_per_graph_identity(torch_backend):
    from models.gat import GATConv
    data, _ = _toy()
    conv = GATConv(10, 4, heads=2)
    conv(data.x, data.edge_index)
    first = conv._cache_csr
    conv(data.x, data.edge_index)
    assert conv._cache_csr is first
    conv(data.x, data.edge_index.clone())
    assert conv._cache_csr is not first
    conv.invalidate()
    assert conv._cache_csr is None


def test_hip_backend_refuses_cpu_tensors():
    from models.gat import GATConv
    data, _ = _toy()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        GATConv(10, 4, heads=2)(data.x, data.edge_index)


def test_call_surface():
    from dcr import _lib
    header = open(os.path.join(REPO, 'include', 'dcr.h')).read()
    for name, count in (('dcr_gat_gather_f32_dev', 15), ('dcr_gat_expand_f32_dev', 23)):
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert m, name + ' is not declared in include/dcr.h'
        params = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
        assert len(params.split(',')) == len(_lib.SIGNATURES[name][1]) == count, name
    build = open(os.path.join(PKG, 'csrc', 'build.sh')).read()
    assert 'dcr_gat' in build.split() and 'dcr_spmm_pieces.h' in build
    spmm = open(os.path.join(PKG, 'csrc', 'dcr_spmm.hip')).read()
    gat = open(os.path.join(PKG, 'csrc', 'dcr_gat.hip')).read()
    pieces = open(os.path.join(PKG, 'csrc', 'dcr_spmm_pieces.h')).read()
    for piece in ('struct Deal {', 'inline void load_vec(', 'inline void store_vec(', 'inline void deal_rows(', 'inline void sum_groups('):
        assert piece in pieces and piece not in spmm and piece not in gat, piece   # moved, not copied
    assert '#include "dcr_spmm_pieces.h"' in spmm and '#include "dcr_spmm_pieces.h"' in gat
    from models.gat import GAT, AttnCSR, GATConv, dense_reference_logits, gat_aggregate, gat_csr, smoke_gat
    assert all(callable(f) for f in (GAT, GATConv, AttnCSR, gat_csr, gat_aggregate, dense_reference_logits, smoke_gat))


@pytest.mark.parametrize('name', gat_ref.FIXTURES)
def test_bounds_would_catch_one_dropped_slot(name):
    """A condition on the fixtures, not a measurement: with ONE slot of the longest row dropped (its last source), the
    restatement differs from the full one by more than 8 x the bound the GPU test applies, in O and in each gradient."""
    ei, n, heads, c, loops, z, s_src, s_dst, d_out = gat_ref.fixture(name)
    cnt = gat_ref.count_matrix(ei, n, loops)
    assert float((s_src.abs().max() + s_dst.abs().max())) <= 8.0 and float(cnt.sum(1).max()) <= 1100
    full = gat_ref.aggregate_reference(z, s_src, s_dst, cnt, d_out)
    bound = gat_ref.bounds(z, s_src, s_dst, cnt, d_out)
    row = int(cnt.sum(1).argmax())
    less = cnt.clone()
    less[row, int((cnt[row] > 0).nonzero()[-1])] -= 1.0
    dropped = gat_ref.aggregate_reference(z, s_src, s_dst, less, d_out)
    for key, a, b in zip(('O', 'dZ', 'dS_src', 'dS_dst'), full, dropped):
        ratio = gat_ref.worst_ratio(b, a, bound[key])
        assert ratio > 8.0, (name, key, ratio)


def test_exact_shapes_reach_every_instantiation():
    """The (H, C) grid of the exact-value GPU test launches all 15 (VEC, LPH) instantiations of the gather and the expand, no
    added width is idle, and ``vec_lph`` still is the table csrc/dcr_gat.hip has."""
    reach = lambda shapes: {gat_ref.vec_lph(c, (h * c,)) for h, c in shapes}
    assert reach(gat_ref.EXACT_SHAPES) == {(v, l) for v in (1, 2, 4) for l in gat_ref.LPHS}
    for h in (1, 2, 3, 8):
        for c in (1, 2, 3, 4, 6, 8, 16, 64, 68):
            assert (h, c) in gat_ref.EXACT_SHAPES
    for extra in gat_ref.EXACT_SHAPES[36:]:
        assert reach([s for s in gat_ref.EXACT_SHAPES if s != extra]) < reach(gat_ref.EXACT_SHAPES), extra
    assert gat_ref.vec_lph(16, (32,), (0,)) == (4, 4) and gat_ref.vec_lph(16, (32,), (8,)) == (2, 8) and gat_ref.vec_lph(16, (33,), (0,)) == (1, 16)
    assert gat_ref.vec_lph(65) is None and gat_ref.vec_lph(256) == (4, 64) and gat_ref.vec_lph(260) is None
    src = open(os.path.join(PKG, 'csrc', 'dcr_gat.hip')).read()
    m = re.search(r'static bool pick_lph_vec\(.*?\n\}\n', src, flags=re.S)
    assert m, 'pick_lph_vec not found'
    table = m.group(0)
    assert 'bool all = C % vec == 0;' in table and 'all = all && ld % vec == 0;' in table
    assert 'all = all && ((uintptr_t)p & (4 * vec - 1)) == 0;' in table
    steps = re.findall(r'if \(pieces <= (\d+)\) go\(Int<(\d+)>\{\}, vec\);', table)
    assert [tuple(int(x) for x in st) for st in steps] == [(l, l) for l in gat_ref.LPHS], steps
    assert re.search(r'if \(ok\(4\)\) return lph\(Int<4>\{\}\);\s*if \(ok\(2\)\) return lph\(Int<2>\{\}\);\s*return lph\(Int<1>\{\}\);', table)
    assert int(re.search(r'constexpr\s+int\s+GAT_LONG\s*=\s*(\d+)\s*;', src).group(1)) == 96
