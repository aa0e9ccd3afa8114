"""R-GCN without a GPU: the typed CSR on hand-built graphs, the plain-torch backend of models/rgcn.py against the dense fp64
restatement of tests/rgcn_ref.py (tolerance 1e-5, the project's GCN tolerance: tests/test_gcn.py), the state dict and the call
surface.  The torch aggregation is selected EXPLICITLY; the product default is the HIP kernel pair and refuses CPU tensors."""
import os
import re

import pytest
import torch

import rgcn_ref
from conftest import PKG, REPO

TOL = 1e-5


@pytest.fixture
def torch_backend():
    from models import gcn
    gcn.set_aggregate_backend('torch')
    yield
    gcn.set_aggregate_backend('hip')


def _rows(rowptr):
    return torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr[1:] - rowptr[:-1])


# 7 nodes, 3 relations.  Node 5 is isolated, node 6 only a source; relation 2 has no edge at all.  (1 -> 0, type 0) appears twice,
# 3 -> 3 is a self-loop of type 1, node 0 receives both relations, out of relation order.
HAND_EI = [[1, 2, 1, 3, 4, 3, 6, 0, 2], [0, 0, 0, 0, 1, 3, 4, 2, 2]]
HAND_ET = [0, 1, 0, 1, 0, 1, 1, 0, 1]


def _hand():
    from models.rgcn import rgcn_norm_csr
    ei, et = torch.tensor(HAND_EI), torch.tensor(HAND_ET)
    return ei, et, rgcn_norm_csr(ei, et, 7, 3)


def test_typed_csr_rows_sorted_by_relation_and_mean_weights():
    ei, et, csr = _hand()
    assert csr.rowptr.dtype == torch.int64 and csr.col.dtype == torch.int32 and csr.val.dtype == torch.float32 and csr.rel.dtype == torch.uint8
    assert csr.rowptr.tolist() == [0, 4, 5, 7, 8, 9, 9, 9]                       # nodes 5 and 6 receive nothing
    # row 0: the two type-0 columns (1 -> 0 twice, in input order) before the two type-1 columns (2, then 3)
    assert csr.rel[:4].tolist() == [0, 0, 1, 1] and csr.col[:4].tolist() == [1, 1, 2, 3]
    assert csr.val[:4].tolist() == [0.5, 0.5, 0.5, 0.5]                          # the duplicate counts twice
    assert csr.col[7:8].tolist() == [3] and csr.rel[7:8].tolist() == [1] and csr.val[7:8].tolist() == [1.0]   # the self-loop, kept
    for rp, rel in ((csr.rowptr, csr.rel), (csr.rowptr_t, csr.rel_t)):
        for i in range(7):
            seg = rel[rp[i]:rp[i + 1]].tolist()
            assert seg == sorted(seg)
    assert not (csr.rel == 2).any() and not (csr.rel_t == 2).any()               # a relation with no edge at all
    assert csr.rowptr_t.tolist() == [0, 1, 3, 5, 7, 8, 8, 9]                     # node 5 sends nothing either
    # val = 1 / |N_r(i)| for every slot, from the definition
    means = rgcn_ref.relation_means(ei, et, 7, 3)
    rows = _rows(csr.rowptr)
    count = (means > 0).double().clone()
    for k in range(rows.numel()):
        i, j, r = int(rows[k]), int(csr.col[k]), int(csr.rel[k])
        n_r = sum(1 for q in range(len(HAND_ET)) if HAND_EI[1][q] == i and HAND_ET[q] == r)
        assert float(csr.val[k]) == 1.0 / n_r and count[r, i, j] == 1.0


def test_transposed_csr_holds_the_same_edges():
    _, _, csr = _hand()
    fwd = sorted(zip(csr.col.tolist(), _rows(csr.rowptr).tolist(), csr.rel.tolist(), csr.val.tolist()))      # (source, target, rel, val)
    bwd = sorted(zip(_rows(csr.rowptr_t).tolist(), csr.col_t.tolist(), csr.rel_t.tolist(), csr.val_t.tolist()))
    assert fwd == bwd and len(fwd) == len(HAND_ET)
    # within one (row, relation) the slots keep the input's order, in both directions
    assert csr.col_t[csr.rowptr_t[1]:csr.rowptr_t[2]].tolist() == [0, 0]
    assert csr.col_t[csr.rowptr_t[3]:csr.rowptr_t[4]].tolist() == [0, 3]


def test_bad_edge_type_raises():
    from models.rgcn import rgcn_norm_csr
    ei = torch.tensor([[0, 1], [1, 0]])
    for bad in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError):
            rgcn_norm_csr(ei, torch.tensor(bad), 2, 2)
    with pytest.raises(ValueError):
        rgcn_norm_csr(ei, torch.tensor([0]), 2, 2)                               # one type per column
    with pytest.raises(ValueError):
        rgcn_norm_csr(ei, torch.tensor([0, 0]), 2, 9)                            # the kernels take at most 8 relations
    empty = rgcn_norm_csr(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 3, 2)
    assert empty.rowptr.tolist() == [0, 0, 0, 0] and empty.rowptr_t.tolist() == [0, 0, 0, 0]


def _typed_toy(n=60, f=12, c=4, seed=0, n_rel=3):
    """A power-law graph with random types, a few duplicated columns and self-loops, and an isolated last node."""
    from dcr import synthetic
    from dcr.data import Data, Dataset
    ei_np, _ = synthetic.powerlaw_graph(n - 1, 3, seed=seed)
    g = torch.Generator().manual_seed(seed)
    ei = torch.from_numpy(ei_np)
    loops = torch.tensor([[2, 7, 7], [2, 7, 7]])
    ei = torch.cat([ei, ei[:, :9], loops], 1)
    et = torch.randint(0, n_rel - 1, (ei.shape[1],), generator=g)               # the last relation stays empty
    x = torch.randn(n, f, generator=g)
    y = torch.randint(0, c, (n,), generator=g)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[torch.randperm(n, generator=g)[:n // 2]] = True
    data = Data(x=x, edge_index=ei, y=y, num_nodes=n, edge_type=et, train_mask=mask, val_mask=~mask)
    return data, Dataset(data, c)


def test_torch_backend_matches_dense_reference(torch_backend):
    from models.rgcn import RGCN
    data, ds = _typed_toy()
    torch.manual_seed(1)
    model = RGCN(ds, num_relations=3, hidden=[16], dropout=0.0)
    with torch.no_grad():
        for conv in model.layers:
            conv.bias.uniform_(-0.5, 0.5)
    model.train()
    lp = model(data)
    torch.nn.functional.nll_loss(lp[data.train_mask], data.y[data.train_mask]).backward()
    want_lp, want_grad = rgcn_ref.model_reference(model.state_dict(), data.x, data.edge_index, data.edge_type, 3, data.y, data.train_mask)
    assert (lp.detach().double() - want_lp).abs().max() < TOL
    for name, p in model.named_parameters():
        assert p.grad is not None and (p.grad.double() - want_grad[name]).abs().max() < TOL, name
    assert float(want_grad['layers.0.weight'][2].abs().max()) == 0.0            # the empty relation: no gradient, none invented
    assert float(model.layers[0].weight.grad[2].abs().max()) == 0.0


def test_state_dict_and_surface():
    from models.rgcn import RGCN, RGCNConv
    data, ds = _typed_toy()
    m = RGCN(ds, num_relations=2, hidden=[16], dropout=0.3)
    sd = m.state_dict()
    assert list(sd.keys()) == ['layers.0.weight', 'layers.0.root', 'layers.0.bias', 'layers.1.weight', 'layers.1.root', 'layers.1.bias']
    assert sd['layers.0.weight'].shape == (2, 12, 16) and sd['layers.0.root'].shape == (12, 16) and sd['layers.0.bias'].shape == (16,)
    assert sd['layers.1.weight'].shape == (2, 16, 4) and sd['layers.1.root'].shape == (16, 4) and sd['layers.1.bias'].shape == (4,)
    assert {id(p) for p in m.reg_params} == {id(p) for p in m.layers[0].parameters()}
    assert {id(p) for p in m.non_reg_params} == {id(p) for p in m.layers[1].parameters()}
    a = (6.0 / (12 + 16)) ** 0.5                                                 # glorot per relation
    assert float(sd['layers.0.weight'].abs().max()) <= a and float(sd['layers.0.root'].abs().max()) <= a
    assert float(sd['layers.0.weight'].abs().max()) > a / 2 and float(sd['layers.0.bias'].abs().sum()) == 0.0
    m2 = RGCN(ds, num_relations=2, hidden=[16], dropout=0.3)
    m2.load_state_dict(sd)
    m.reset_parameters()
    bare = RGCNConv(5, 3, 4, root_weight=False, bias=False)
    assert list(bare.state_dict().keys()) == ['weight'] and bare.root is None and bare.bias is None
    with pytest.raises(ValueError):
        RGCNConv(5, 3, 9)
    del data.edge_type
    with pytest.raises(ValueError, match='edge_type'):
        m(data)


def test_hip_backend_refuses_cpu_tensors():
    from models.rgcn import RGCNConv
    data, _ = _typed_toy()
    conv = RGCNConv(12, 4, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        conv(data.x, data.edge_index, data.edge_type)


def test_one_relation_without_root_is_plain_mean_aggregation(torch_backend):
    from models.rgcn import RGCNConv
    data, _ = _typed_toy()
    n = data.num_nodes
    conv = RGCNConv(12, 5, 1, root_weight=False, bias=False)
    got = conv(data.x, data.edge_index, torch.zeros_like(data.edge_type))
    z = data.x.double() @ conv.weight[0].detach().double()
    total = torch.zeros(n, 5, dtype=torch.float64).index_add_(0, data.edge_index[1], z[data.edge_index[0]])
    indeg = torch.bincount(data.edge_index[1], minlength=n).double()
    want = total / indeg.clamp(min=1.0)[:, None]
    assert (got.detach().double() - want).abs().max() < TOL
    assert float(got[n - 1].abs().max()) == 0.0                                  # the isolated node


def test_layer_caches_its_csr_per_graph_identity(torch_backend):
    from models.rgcn import RGCNConv
    data, _ = _typed_toy()
    conv = RGCNConv(12, 4, 3)
    conv(data.x, data.edge_index, data.edge_type)
    first = conv._cache_csr
    conv(data.x, data.edge_index, data.edge_type)
    assert conv._cache_csr is first
    conv(data.x, data.edge_index, data.edge_type.clone())                        # another tensor: rebuilt
    assert conv._cache_csr is not first
    conv.invalidate()
    assert conv._cache_csr is None


def test_gpu_shapes_reach_every_typed_spmm_instantiation():
    """tests/test_rgcn_gpu.py launches all 15 (LPR, VEC) instantiations of both kernels, every added width and the third pad
    is needed for that, and ``vec_lpr`` still is the dispatch csrc/dcr_spmm.hip has."""
    import rgcn_shapes as S
    picked = {S.vec_lpr(f, *S.leading_dims(f, n_rel, self_block, pad)) for f in S.N_FEATS for pad in S.PADS for n_rel in (1, 2, 3, 8)
              for self_block in (0, 1)}
    assert picked == {(v, l) for v in (1, 2, 4) for l in (4, 8, 16, 32, 64)}
    # beyond (VEC, LPR): a second trip of the f0 loop at every VEC, and VEC 2 forced by a leading dimension on 4 to 64 lanes
    # (path = (VEC, LPR, more than one trip, VEC narrowed by a leading dimension))
    reached = S.paths()
    assert {(4, 64, True, False), (2, 64, True, False), (1, 64, True, False)} <= reached
    assert {(2, 4, False, True), (2, 32, False, True), (2, 64, False, True), (2, 64, True, True)} <= reached
    # no added entry is idle: without any one of them some path is no longer run
    for f in (20, 13, 17, 10, 18, 34, 66, 130, 65):
        assert S.paths(n_feats=[w for w in S.N_FEATS if w != f]) < reached, f
    assert 2 in S.PADS and S.paths(pads=[p for p in S.PADS if p != 2]) < reached
    for f in (1, 2, 3, 4, 6, 7, 64, 68, 260):
        assert f in S.N_FEATS
    assert {0, 1} <= set(S.PADS)
    # the table itself, from the text of the source
    src = open(os.path.join(PKG, 'csrc', 'dcr_spmm.hip')).read()
    m = re.search(r'static void pick_lpr_vec\(int F, VecOk v, Go &&go\) \{(.*?)\n\}\n', src, flags=re.S)
    assert m, 'pick_lpr_vec not found'
    table = m.group(1)
    # VEC: the widest allowed, in this order; the count the LPR steps compare is the row's VEC-wide pieces
    assert re.search(r'if \(v\.v4\) lpr\(Int<4>\{\}\);\s*else if \(v\.v2\) lpr\(Int<2>\{\}\);\s*else lpr\(Int<1>\{\}\);', table)
    assert re.search(r'auto lpr = \[&\]\(auto vec\) \{\s*const int pieces = F / decltype\(vec\)::value;', table)
    steps = re.findall(r'if \(pieces <= (\d+)\) go\(Int<(\d+)>\{\}, vec\);', table)
    assert [tuple(int(x) for x in s) for s in steps] == [(l, l) for l in S.LPRS[:-1]], steps
    assert re.findall(r'else go\(Int<(\d+)>\{\}, vec\);', table) == [str(S.LPRS[-1])]
    assert len(re.findall(r'\bgo\(', table)) == len(S.LPRS)
    # what narrows VEC: the width, both leading dimensions and the pointers the entry point names
    m = re.search(r'static VecOk vec_ok\(int F, int64_t ld_in, int64_t ld_out, std::initializer_list<const void \*> ptrs\) \{(.*?)\n\}\n', src,
                  flags=re.S)
    assert m, 'vec_ok not found'
    assert 'bool all = F % vec == 0 && ld_in % vec == 0 && ld_out % vec == 0;' in m.group(1)
    assert 'for (const void *p : ptrs) all = all && ((uintptr_t)p & (4 * vec - 1)) == 0;' in m.group(1)
    assert 'return {ok(4), ok(2)};' in m.group(1)
    for name, lds, ptrs in (('dcr_spmm_csr_typed_f32_dev', ('ldb', 'ldc'), ('B',)), ('dcr_spmm_csr_typed_expand_f32_dev', ('ldg', 'ldc'), ('G', 'C'))):
        body = src[src.index('extern "C" int ' + name):]
        body = body[:body.index('\n}\n')]
        assert 'pick_lpr_vec(F, vec_ok(F, %s, %s, {%s}), [&]' % (lds + (', '.join(ptrs),)) in body, name
        assert body.count('vec_ok(') == 1 and 'v2 =' not in body and 'v4 =' not in body, name
    assert S.vec_lpr(64, 256, 64) == (4, 16) and S.vec_lpr(64, 256, 64, residues=(8,)) == (2, 32) and S.vec_lpr(64, 256, 64, residues=(0, 4)) == (1, 64)


def test_call_surface():
    from dcr import _lib
    header = open(os.path.join(REPO, 'include', 'dcr.h')).read()
    for name in ('dcr_spmm_csr_typed_f32_dev', 'dcr_spmm_csr_typed_expand_f32_dev'):
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert m, name + ' is not declared in include/dcr.h'
        params = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
        assert len(params.split(',')) == len(_lib.SIGNATURES[name][1]), name
    assert len(_lib.SIGNATURES['dcr_spmm_csr_typed_f32_dev'][1]) == 15 and len(_lib.SIGNATURES['dcr_spmm_csr_typed_expand_f32_dev'][1]) == 13
    assert 'dcr_spmm' in open(os.path.join(PKG, 'csrc', 'build.sh')).read().split()
    from models.rgcn import RGCN, RGCNConv, TypedCSR, rgcn_norm_csr, typed_aggregate
    assert all(callable(f) for f in (RGCN, RGCNConv, TypedCSR, rgcn_norm_csr, typed_aggregate))
