"""The typed aggregation kernel pair (csrc/dcr_rgcn.hip) through the raw ABI, and the R-GCN layer on them (models/rgcn.py).

Exact cases: ``val`` dyadic and small integers in the operands, so every fp32 operation is exact and the result must equal a
float64 numpy restatement bit for bit.  Random floats: the forward error bound of an fp32 ``fmaf`` sum against float64,
k·2⁻²⁴·Σ|terms| with k = (slots feeding the element) + 2 — one rounding per slot, one for the row's own block, one for the bias
(a hub row's strided sum puts no term through more additions than that).  The bound is derived, not tuned.  As measured on an
MI355X the worst element sits at 0.64 of it (gather) and 0.45 (expand), the adjointness gap at 1.7e-6 and 8.0e-6 against bounds
of 4.6e-2 and 4.3e-1, and the two-layer model at 5.5e-7 from the dense fp64 reference (tolerance 1e-5)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fosr_ref
import rgcn_ref

pytestmark = pytest.mark.gpu

EINVAL = -1
U = 2.0 ** -24
N_COLS = 80                                   # rows of the gathered operand; >= every n_rows below (the self block reads row i)
N_FEATS = [1, 2, 3, 4, 6, 7, 64, 68, 260]     # every VEC path, 260 > one group's stride of 64 lanes x 4
# row lengths, most telling first: a prefix of this list is the graph at small n_rows.  'one': every slot of one relation.
PATTERN = [(400, 'mixed'), (0, 'mixed'), (3, 'one'), (97, 'mixed'), (300, 'one'), (96, 'mixed'), (95, 'mixed'), (1, 'one'), (0, 'mixed')]
FULL_ROWS = 70                                # holds the whole pattern and more than one workgroup at every LPR


@pytest.fixture(scope='module')
def lib():
    from dcr import _lib
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def typed_csr(rows, cols, rels, vals, n_rows):
    """Typed CSR of the slots given in COO form: by row, inside a row by relation, stably within one."""
    order = np.argsort(rows * 16 + rels, kind='stable')
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=rowptr[1:])
    return rowptr, cols[order].astype(np.int32), vals[order].astype(np.float32), rels[order].astype(np.uint8)


def family(n_rows, n_rel, seed, dyadic, n_cols=N_COLS):
    """COO slots (rows, cols, rels, vals) of the test graph: PATTERN's rows first, then short rows of 0..8 slots."""
    rng = np.random.default_rng(seed)
    rows, cols, rels = [], [], []
    for i in range(n_rows):
        length, kind = PATTERN[i] if i < len(PATTERN) else (int(rng.integers(0, 9)), 'mixed')
        rows.append(np.full(length, i, dtype=np.int64))
        cols.append(rng.integers(0, n_cols, length))
        rels.append(np.full(length, min(1 + i % 2, n_rel - 1)) if kind == 'one' else rng.integers(0, n_rel, length))
    rows, cols, rels = (np.concatenate(a).astype(np.int64) for a in (rows, cols, rels))
    vals = 0.5 ** rng.integers(0, 4, rows.size) if dyadic else rng.uniform(0.05, 1.0, rows.size)
    return rows, cols, rels, vals.astype(np.float32)


def dense(rows, cols, rels, vals, n_rows, n_rel, n_cols=N_COLS):
    """A[r, i, j] = Σ val over the slots (i, j) of relation r, float64; cnt[r, i] = the number of such slots in row i."""
    A = np.zeros((n_rel, n_rows, n_cols))
    np.add.at(A, (rels, rows, cols), vals.astype(np.float64))
    cnt = np.zeros((n_rel, n_rows), dtype=np.int64)
    np.add.at(cnt, (rels, rows), 1)
    return A, cnt


def vec_lpr(n_feat, *lds):
    """(VEC, LPR) of the dispatch for 16-byte aligned operands (csrc/dcr_rgcn.hip, DCR_TYPED_PICK)."""
    vec = next((v for v in (4, 2) if n_feat % v == 0 and all(ld % v == 0 for ld in lds)), 1)
    return vec, next((lpr for lpr in (4, 8, 16, 32) if n_feat // vec <= lpr), 64)


def row_counts(n_feat, *lds):
    g = 256 // vec_lpr(n_feat, *lds)[1]
    return [g - 1, g, g + 1, FULL_ROWS]


class Graph:
    def __init__(self, n_rows, n_rel, seed, dyadic):
        coo = family(n_rows, n_rel, seed, dyadic)
        self.n_rows, self.n_rel = n_rows, n_rel
        self.A, self.cnt = dense(*coo, n_rows, n_rel)
        self.host = typed_csr(*coo, n_rows)
        self.dev = tuple(dev(a) for a in self.host)


_GRAPHS = {}


def graph(n_rows, n_rel, dyadic, seed=0):
    key = (n_rows, n_rel, dyadic, seed)
    if key not in _GRAPHS:
        _GRAPHS[key] = Graph(n_rows, n_rel, 100 * seed + 7 * n_rows + n_rel, dyadic)
    return _GRAPHS[key]


def padded(values, ld):
    """[rows, ld] float32 on the device: ``values`` in the leading columns, NaN in the padding (never to be read or written)."""
    out = np.full((values.shape[0], ld), np.nan, dtype=np.float32)
    out[:, :values.shape[1]] = values
    return dev(out)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_gather(lib, csr, B, n_rows, n_feat, n_rel, ldc, self_block, bias=None, relu=0):
    C = torch.full((n_rows, ldc), float('nan'), dtype=torch.float32, device='cuda')
    rc = lib.dcr_spmm_csr_typed_f32_dev(*(t.data_ptr() for t in csr), B.data_ptr(), C.data_ptr(), n_rows, n_feat, n_rel, B.shape[1], ldc,
                                        self_block, None if bias is None else bias.data_ptr(), relu, stream())
    assert rc == 0, rc
    out = C.cpu().numpy()
    assert np.isnan(out[:, n_feat:]).all()
    return out[:, :n_feat]


def run_expand(lib, csr, Gm, n_rows, n_feat, n_rel, ldc, self_block):
    C = torch.full((n_rows, ldc), float('nan'), dtype=torch.float32, device='cuda')   # (every block must be written over the NaN)
    rc = lib.dcr_spmm_csr_typed_expand_f32_dev(*(t.data_ptr() for t in csr), Gm.data_ptr(), C.data_ptr(), n_rows, n_feat, n_rel,
                                               Gm.shape[1], ldc, self_block, stream())
    assert rc == 0, rc
    wide = (n_rel + self_block) * n_feat
    out = C.cpu().numpy()
    assert np.isnan(out[:, wide:]).all()
    return out[:, :wide]


def gather_ref(g, Bv, n_feat, self_block):
    """(Σ_r A_r·B_r (+ the own block), Σ |A_r|·|B_r| (+ |own block|)) in float64 from the values of B."""
    B = Bv.astype(np.float64)
    blocks = [B[:, r * n_feat:(r + 1) * n_feat] for r in range(g.n_rel + self_block)]
    out = sum(g.A[r] @ blocks[r] for r in range(g.n_rel))
    mag = sum(np.abs(g.A[r]) @ np.abs(blocks[r]) for r in range(g.n_rel))
    if self_block:
        out, mag = out + blocks[g.n_rel][:g.n_rows], mag + np.abs(blocks[g.n_rel][:g.n_rows])
    return out, mag


def expand_ref(g, Gv, n_feat, self_block):
    G = Gv.astype(np.float64)
    out = [g.A[r] @ G for r in range(g.n_rel)] + ([G[:g.n_rows]] if self_block else [])
    mag = [np.abs(g.A[r]) @ np.abs(G) for r in range(g.n_rel)] + ([np.zeros((g.n_rows, n_feat))] if self_block else [])
    return np.concatenate(out, 1), np.concatenate(mag, 1)


def same_bits(got, want64):
    want = (want64 + 0.0).astype(np.float32)       # (+ 0.0: no negative zero out of the restatement; the kernels form none)
    return got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize('n_rel', [1, 2, 3, 8])
def test_exact_values(lib, n_rel):
    rng = np.random.default_rng(n_rel)
    family_covers_the_hub_path(n_rel)
    for n_feat in N_FEATS:
        for pad in (0, 1):
            for self_block in (0, 1):
                wide, narrow = (n_rel + self_block) * n_feat + pad, n_feat + pad
                Bv = rng.integers(-4, 5, (N_COLS, wide - pad)).astype(np.float32)
                Gv = rng.integers(-4, 5, (N_COLS, n_feat)).astype(np.float32)
                bias_v = rng.integers(-3, 4, n_feat).astype(np.float32)
                B, Gm, bias = padded(Bv, wide), padded(Gv, narrow), dev(bias_v)
                assert row_counts(n_feat, wide, narrow)[:3] == [256 // vec_lpr(n_feat, wide, narrow)[1] + d for d in (-1, 0, 1)]
                for n_rows in row_counts(n_feat, wide, narrow):
                    g = graph(n_rows, n_rel, True)
                    label = (n_rel, n_feat, pad, self_block, n_rows)
                    want, _ = gather_ref(g, Bv, n_feat, self_block)
                    for with_bias in (0, 1):
                        for relu in (0, 1):
                            w = want + bias_v if with_bias else want
                            w = np.maximum(w, 0.0) if relu else w
                            got = run_gather(lib, g.dev, B, n_rows, n_feat, n_rel, narrow, self_block, bias if with_bias else None, relu)
                            assert same_bits(got, w), ('gather',) + label + (with_bias, relu)
                    got = run_expand(lib, g.dev, Gm, n_rows, n_feat, n_rel, wide, self_block)
                    want, _ = expand_ref(g, Gv, n_feat, self_block)
                    assert same_bits(got, want), ('expand',) + label
                    # a block of a relation the row has no slot of is zeros, written over the NaN
                    for r in range(n_rel):
                        empty = g.cnt[r] == 0
                        assert empty.any()
                        assert not got[empty, r * n_feat:(r + 1) * n_feat].any()


def family_covers_the_hub_path(n_rel):
    """What the exact test relies on: the full graph has rows at 95, 96, 97 and hundreds of slots, empty rows, short and hub rows
    of a single relation, and sorted slots."""
    g = graph(FULL_ROWS, n_rel, True)
    lengths = np.diff(g.host[0])
    assert {0, 3, 95, 96, 97, 300, 400} <= set(lengths.tolist())
    one = [i for i in range(FULL_ROWS) if lengths[i] and (g.cnt[:, i] > 0).sum() == 1]
    assert any(lengths[i] == 300 for i in one) and any(lengths[i] == 3 for i in one)
    for i in range(FULL_ROWS):
        seg = g.host[3][g.host[0][i]:g.host[0][i + 1]].tolist()
        assert seg == sorted(seg)


def test_one_relation_is_the_plain_spmm_bit_for_bit(lib):
    rng = np.random.default_rng(11)
    g = graph(FULL_ROWS, 1, False)
    for n_feat in N_FEATS:
        for pad in (0, 1):
            ld = n_feat + pad
            B = padded(rng.standard_normal((N_COLS, n_feat)).astype(np.float32), ld)
            bias = dev(rng.standard_normal(n_feat).astype(np.float32))
            for with_bias, relu in ((0, 0), (1, 0), (1, 1)):
                b = bias if with_bias else None
                got = run_gather(lib, g.dev, B, FULL_ROWS, n_feat, 1, ld, 0, b, relu)
                C = torch.full((FULL_ROWS, ld), float('nan'), dtype=torch.float32, device='cuda')
                rowptr, col, val, _ = g.dev
                rc = lib.dcr_spmm_csr_f32_dev(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), B.data_ptr(), C.data_ptr(), FULL_ROWS,
                                              n_feat, ld, ld, None if b is None else b.data_ptr(), relu, stream())
                assert rc == 0
                assert got.tobytes() == C.cpu().numpy()[:, :n_feat].tobytes(), (n_feat, pad, with_bias, relu)


@pytest.mark.parametrize('n_rel', [2, 8])
def test_random_floats_within_the_fmaf_bound(lib, n_rel):
    rng = np.random.default_rng(20 + n_rel)
    g = graph(FULL_ROWS, n_rel, False)
    slots = g.cnt.sum(0)[:, None]
    for n_feat in (3, 64, 260):
        for self_block in (0, 1):
            wide = (n_rel + self_block) * n_feat
            Bv = rng.standard_normal((N_COLS, wide)).astype(np.float32)
            Gv = rng.standard_normal((N_COLS, n_feat)).astype(np.float32)
            bias_v = rng.standard_normal(n_feat).astype(np.float32)
            want, mag = gather_ref(g, Bv, n_feat, self_block)
            for with_bias in (0, 1):
                got = run_gather(lib, g.dev, dev(Bv), FULL_ROWS, n_feat, n_rel, n_feat, self_block, dev(bias_v) if with_bias else None, 0)
                w, m = (want + bias_v, mag + np.abs(bias_v)) if with_bias else (want, mag)
                err, bound = np.abs(got.astype(np.float64) - w), (slots + 2) * U * m
                print(f'gather R={n_rel} F={n_feat} self={self_block} bias={with_bias}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}')
                assert (err <= bound).all()
            got = run_expand(lib, g.dev, dev(Gv), FULL_ROWS, n_feat, n_rel, wide, self_block)
            want_e, mag_e = expand_ref(g, Gv, n_feat, self_block)
            k = np.concatenate([np.repeat(g.cnt[r][:, None], n_feat, 1) + 2 for r in range(n_rel)] +
                               ([np.zeros((FULL_ROWS, n_feat))] if self_block else []), 1)
            err, bound = np.abs(got.astype(np.float64) - want_e), k * U * mag_e
            print(f'expand R={n_rel} F={n_feat} self={self_block}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}')
            assert (err <= bound).all()


def test_two_calls_give_the_same_bits(lib):
    rng = np.random.default_rng(31)
    g = graph(FULL_ROWS, 3, False)
    for n_feat in (7, 64):
        B = dev(rng.standard_normal((N_COLS, 4 * n_feat)).astype(np.float32))
        Gm = dev(rng.standard_normal((N_COLS, n_feat)).astype(np.float32))
        assert run_gather(lib, g.dev, B, FULL_ROWS, n_feat, 3, n_feat, 1).tobytes() == run_gather(lib, g.dev, B, FULL_ROWS, n_feat, 3, n_feat, 1).tobytes()
        assert run_expand(lib, g.dev, Gm, FULL_ROWS, n_feat, 3, 4 * n_feat, 1).tobytes() == run_expand(lib, g.dev, Gm, FULL_ROWS, n_feat, 3, 4 * n_feat, 1).tobytes()


@pytest.mark.parametrize('n_feat', [6, 64])
def test_expand_is_the_adjoint_of_the_gather(lib, n_feat):
    """⟨gather(B), G⟩ = ⟨B, expand(G)⟩ in float64 of the returned values, within the two kernels' element bounds summed against the
    other factor: ties the backward kernel (on the transposed CSR) to the forward one."""
    n, n_rel = N_COLS, 3
    rng = np.random.default_rng(40 + n_feat)
    rows, cols, rels, vals = family(n, n_rel, 41, False, n_cols=n)
    hub = rng.integers(0, n, 250)                                    # a hub COLUMN too: a long row of the transposed pattern
    rows, cols = np.concatenate([rows, hub]), np.concatenate([cols, np.full(250, 5)])
    rels, vals = np.concatenate([rels, rng.integers(0, n_rel, 250)]), np.concatenate([vals, rng.uniform(0.05, 1.0, 250).astype(np.float32)])
    fwd, bwd = tuple(dev(a) for a in typed_csr(rows, cols, rels, vals, n)), tuple(dev(a) for a in typed_csr(cols, rows, rels, vals, n))
    assert np.diff(typed_csr(cols, rows, rels, vals, n)[0]).max() > 96
    A, cnt = dense(rows, cols, rels, vals, n, n_rel, n_cols=n)
    At, cnt_t = dense(cols, rows, rels, vals, n, n_rel, n_cols=n)
    wide = (n_rel + 1) * n_feat
    Bv = rng.standard_normal((n, wide)).astype(np.float32)
    Gv = rng.standard_normal((n, n_feat)).astype(np.float32)
    out = run_gather(lib, fwd, dev(Bv), n, n_feat, n_rel, n_feat, 1).astype(np.float64)
    back = run_expand(lib, bwd, dev(Gv), n, n_feat, n_rel, wide, 1).astype(np.float64)
    B, G = Bv.astype(np.float64), Gv.astype(np.float64)
    mag = sum(np.abs(A[r]) @ np.abs(B[:, r * n_feat:(r + 1) * n_feat]) for r in range(n_rel)) + np.abs(B[:, n_rel * n_feat:])
    bound = np.sum(np.abs(G) * (cnt.sum(0)[:, None] + 2) * U * mag)
    for r in range(n_rel):
        bound += np.sum(np.abs(B[:, r * n_feat:(r + 1) * n_feat]) * (cnt_t[r][:, None] + 2) * U * (np.abs(At[r]) @ np.abs(G)))
    lhs, rhs = np.sum(out * G), np.sum(B * back)
    print(f'adjointness F={n_feat}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}')
    assert abs(lhs - rhs) <= bound


def test_argument_errors(lib):
    g = graph(FULL_ROWS, 2, True)
    n_feat = 4
    B = dev(np.ones((N_COLS, 3 * n_feat), dtype=np.float32))
    Gm = dev(np.ones((N_COLS, n_feat), dtype=np.float32))
    C = torch.full((FULL_ROWS, 3 * n_feat), float('nan'), dtype=torch.float32, device='cuda')
    csr = [t.data_ptr() for t in g.dev]

    def gather(csr=csr, b=B.data_ptr(), c=C.data_ptr(), n_rel=2, ldb=3 * n_feat, ldc=n_feat, n_rows=FULL_ROWS, f=n_feat):
        return lib.dcr_spmm_csr_typed_f32_dev(*csr, b, c, n_rows, f, n_rel, ldb, ldc, 1, None, 0, stream())

    def expand(csr=csr, gm=Gm.data_ptr(), c=C.data_ptr(), n_rel=2, ldg=n_feat, ldc=3 * n_feat, n_rows=FULL_ROWS, f=n_feat):
        return lib.dcr_spmm_csr_typed_expand_f32_dev(*csr, gm, c, n_rows, f, n_rel, ldg, ldc, 1, stream())

    for call in (gather, expand):
        assert call(n_rel=0) == EINVAL and call(n_rel=9) == EINVAL
        assert call(n_rows=-1) == EINVAL and call(f=0) == EINVAL
        assert call(c=None) == EINVAL
        for k in range(4):
            assert call(csr=csr[:k] + [None] + csr[k + 1:]) == EINVAL, k
    assert gather(b=None) == EINVAL and expand(gm=None) == EINVAL
    assert gather(ldb=3 * n_feat - 1) == EINVAL and gather(ldc=n_feat - 1) == EINVAL      # ldb >= (n_rel + self_block) * n_feat
    assert expand(ldc=3 * n_feat - 1) == EINVAL and expand(ldg=n_feat - 1) == EINVAL
    from dcr import _lib
    assert b'typed SpMM' in _lib.lib().dcr_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(C).all())                                                      # nothing was launched
    assert gather() == 0 and expand() == 0


@pytest.fixture(scope='module')
def fosr_model():
    """Two cliques joined by a path (60 nodes) through fosr(data, 5), and a two-layer RGCN on the result."""
    from dcr.data import Data, Dataset
    from models.rgcn import RGCN
    from rewiring.fosr import fosr
    ei, n, _, _ = fosr_ref.two_cliques(28, 4)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, 12, generator=g)
    y = torch.randint(0, 4, (n,), generator=g)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[torch.randperm(n, generator=g)[:n // 2]] = True
    data = Data(x=x, edge_index=torch.from_numpy(ei), y=y, num_nodes=n, train_mask=mask, val_mask=~mask).to('cuda')
    out = fosr(data, 5)
    assert n == 60 and out.edge_type.cpu().tolist() == [0] * ei.shape[1] + [1] * 10
    torch.manual_seed(3)
    model = RGCN(Dataset(out, 4), num_relations=2, hidden=[16], dropout=0.0).cuda()
    with torch.no_grad():
        for conv in model.layers:
            conv.bias.uniform_(-0.5, 0.5)
    return out, model


def _logits_and_grads(model, data):
    model.train()
    model.zero_grad()
    lp = model(data)
    torch.nn.functional.nll_loss(lp[data.train_mask], data.y[data.train_mask]).backward()
    return lp.detach().double().cpu(), {k: p.grad.detach().double().cpu() for k, p in model.named_parameters()}


def test_model_on_a_fosr_output_matches_the_dense_reference(fosr_model):
    from models import gcn
    data, model = fosr_model
    want_lp, want_grad = rgcn_ref.model_reference(model.state_dict(), data.x, data.edge_index, data.edge_type, 2, data.y, data.train_mask)
    lp, grad = _logits_and_grads(model, data)
    worst = max([float((lp - want_lp).abs().max())] + [float((grad[k] - want_grad[k]).abs().max()) for k in grad])
    print(f'RGCN on the HIP kernels against the dense fp64 reference: worst difference {worst:.3e}')
    assert (lp - want_lp).abs().max() < 1e-5
    for k in grad:
        assert (grad[k] - want_grad[k]).abs().max() < 1e-5, k
    assert float(grad['layers.0.weight'][1].abs().max()) > 0.0                   # the added edges' relation is trained
    gcn.set_aggregate_backend('torch')
    try:
        lp_t, grad_t = _logits_and_grads(model, data)
    finally:
        gcn.set_aggregate_backend('hip')
    assert (lp - lp_t).abs().max() < 1e-5
    for k in grad:
        assert (grad[k] - grad_t[k]).abs().max() < 1e-5, k


def test_training_loop_runs_an_rgcn(fosr_model):
    import copy
    from experiment.training_loop import train, training_loop
    data, model = fosr_model
    model = copy.deepcopy(model)
    model.dropout.p = 0.5
    optimizer = torch.optim.Adam([dict(params=model.reg_params, weight_decay=5e-4), dict(params=model.non_reg_params, weight_decay=0)], lr=0.01)
    assert training_loop(model, optimizer, data, 3, 10) is model
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert math.isfinite(train(model, optimizer, data))
