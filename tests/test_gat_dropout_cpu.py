"""Attention dropout of GAT without a GPU: the call surface, the plain-torch backend of models/gat.py under an explicit keep matrix
against the per-slot fp64 restatement of tests/gat_dropout_ref.py, the model in evaluation mode, and the conditions on the fixtures
and the host stream that tests/test_gat_dropout_gpu.py relies on."""
import os
import re

import numpy as np
import pytest
import torch

import dropout_ref
import gat_dropout_ref as R
import gat_ref
from conftest import REPO


@pytest.fixture
def torch_backend():
    from models import gcn
    gcn.set_aggregate_backend('torch')
    yield
    gcn.set_aggregate_backend('hip')


def test_call_surface():
    from dcr import _lib
    header = open(os.path.join(REPO, 'include', 'dcr.h')).read()
    for name, count in (('dcr_gat_gather_drop_f32_dev', 21), ('dcr_gat_expand_drop_f32_dev', 27)):
        m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert m, name + ' is not declared in include/dcr.h'
        params = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
        assert len(params.split(',')) == len(_lib.SIGNATURES[name][1]) == count, name
    assert 'E = h * S8 + pos' in header                                   # the stream rule is stated next to the declarations
    from models.gat import GAT, GATConv
    conv = GATConv(5, 3, heads=2, attn_dropout=0.5)
    assert conv.attn_dropout == 0.5 and GATConv(5, 3).attn_dropout == 0.0
    with pytest.raises(NotImplementedError, match='attention coefficients'):
        GATConv(5, 3, heads=2, dropout=0.1)
    with pytest.raises(NotImplementedError, match='attn_dropout'):       # the message names the keyword that does it
        GATConv(5, 3, heads=2, dropout=0.1)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            GATConv(5, 3, attn_dropout=bad)
    assert 'not part of the model' not in GAT.__doc__ and 'not implemented' not in GATConv.__doc__


def _fixture_slots(name):
    ei, n, heads, c, loops, z, s_src, s_dst, d_out = gat_ref.fixture(name)
    rows, cols, rowptr, slot_t = R.slots(ei, n, loops)
    return ei, n, heads, c, loops, z, s_src, s_dst, d_out, rows, cols, rowptr, slot_t


def test_reference_slots_are_the_models_and_no_mask_is_the_dense_restatement():
    """The restatement's own slot list is the AttnCSR's (the decisions are tied to positions in it), and with every slot kept at
    weight 1 it is the dense restatement of gat_ref."""
    from models.gat import gat_csr
    for name in gat_ref.FIXTURES:
        ei, n, heads, c, loops, z, s_src, s_dst, d_out, rows, cols, rowptr, slot_t = _fixture_slots(name)
        csr = gat_csr(ei, n, loops)
        nnz = int(rowptr[-1])
        assert csr.nnz == nnz == rows.numel() and torch.equal(csr.rowptr, rowptr) and torch.equal(csr.col[:nnz].long(), cols)
        assert torch.equal(csr.slot_t[:nnz], slot_t)
        ones = torch.ones(nnz, heads, dtype=torch.float64)
        got = R.aggregate_reference(z, s_src, s_dst, rows, cols, ones, d_out)
        want = gat_ref.aggregate_reference(z, s_src, s_dst, gat_ref.count_matrix(ei, n, loops), d_out)
        for a, b in zip(got, want):
            assert (a - b).abs().max() < 1e-12


def test_torch_backend_with_an_explicit_keep_matches_the_reference():
    from models.gat import _aggregate_torch, gat_csr
    ei, n, heads, c, loops, z, s_src, s_dst, d_out, rows, cols, rowptr, _ = _fixture_slots('powerlaw')
    assert int(torch.bincount(rows * n + cols).max()) == 2 and int((rowptr[1:] - rowptr[:-1]).min()) == 1   # duplicates; the isolated node
    nnz = rows.numel()
    keep = R.keep_weights(R.decisions(nnz, heads, 0.6, R.SEEDS[0], 3), 0.6)
    assert 0 < int((keep == 0).sum()) < keep.numel()
    dup = (torch.bincount(rows * n + cols)[rows * n + cols] == 2).nonzero().flatten()
    assert bool((keep[dup[0::2]] != keep[dup[1::2]]).any())             # two slots of one column, two decisions
    want = R.aggregate_reference(z, s_src, s_dst, rows, cols, keep, d_out)
    leaves = [t.double().clone().requires_grad_(True) for t in (z, s_src, s_dst)]
    out = _aggregate_torch(*leaves, gat_csr(ei, n, loops), R.SLOPE, keep=keep)
    out.backward(d_out.double())
    for got, w in zip((out.detach(),) + tuple(t.grad for t in leaves), want):
        assert (got - w).abs().max() < 1e-12


def test_torch_backend_draws_its_own_mask_only_in_training(torch_backend):
    from models.gat import gat_aggregate, gat_csr
    ei, n, heads, c, loops, z, s_src, s_dst, *_ = _fixture_slots('powerlaw')
    csr = gat_csr(ei, n, loops)
    plain = gat_aggregate(z, s_src, s_dst, csr)
    assert torch.equal(gat_aggregate(z, s_src, s_dst, csr, 0.2, attn_dropout=0.6, training=False), plain)
    assert torch.equal(gat_aggregate(z, s_src, s_dst, csr, 0.2, attn_dropout=0.0, training=True), plain)
    torch.manual_seed(0)
    assert not torch.equal(gat_aggregate(z, s_src, s_dst, csr, 0.2, attn_dropout=0.6, training=True), plain)
    with pytest.raises(ValueError):
        gat_aggregate(z, s_src, s_dst, csr, 0.2, attn_dropout=1.0, training=True)


def test_model_in_eval_mode_ignores_both_dropouts(torch_backend):
    from test_gat_cpu import _toy
    from models.gat import GAT
    data, ds = _toy()
    torch.manual_seed(1)
    plain = GAT(ds, hidden=[6], heads=3, output_heads=2, dropout=0.6)
    both = GAT(ds, hidden=[6], heads=3, output_heads=2, dropout=0.6, attn_dropout=0.6, input_dropout=0.6)
    assert list(both.state_dict().keys()) == list(plain.state_dict().keys())
    both.load_state_dict(plain.state_dict())
    assert all(conv.attn_dropout == 0.6 for conv in both.layers) and both.input_dropout.p == 0.6 and plain.input_dropout.p == 0.0
    plain.eval()
    both.eval()
    with torch.no_grad():
        assert torch.equal(both(data), plain(data))
    both.train()
    torch.manual_seed(2)
    lp = both(data)
    with torch.no_grad():
        assert not torch.equal(lp, plain(data))
    lp.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in both.parameters())


@pytest.mark.parametrize('name', gat_ref.FIXTURES)
def test_bounds_would_catch_one_flipped_keep_decision(name):
    """A condition on the fixtures, not a measurement: at p = 0.5, with ONE keep decision of the longest row flipped (the slot
    of its last source, every head), the restatement moves by more than 8 x the bound the GPU test applies, in O and in each gradient — the
    factor of test_gat_cpu.py::test_bounds_would_catch_one_dropped_slot."""
    ei, n, heads, c, loops, z, s_src, s_dst, d_out, rows, cols, rowptr, _ = _fixture_slots(name)
    p = 0.5
    dec = R.decisions(rows.numel(), heads, p, R.SEEDS[0], 0)
    cnt = gat_ref.count_matrix(ei, n, loops)
    bound = R.bounds(z, s_src, s_dst, cnt, d_out, p)
    full = R.aggregate_reference(z, s_src, s_dst, rows, cols, R.keep_weights(dec, p), d_out)
    row = int((rowptr[1:] - rowptr[:-1]).argmax())
    flipped = dec.copy()
    lo, hi = int(rowptr[row]), int(rowptr[row + 1])
    flipped[lo + int(cols[lo:hi].argmax())] ^= True                        # the slot of its last source, as that test drops it
    moved = R.aggregate_reference(z, s_src, s_dst, rows, cols, R.keep_weights(flipped, p), d_out)
    for key, a, b in zip(('O', 'dZ', 'dS_src', 'dS_dst'), full, moved):
        ratio = gat_ref.worst_ratio(b, a, bound[key])
        assert ratio > 8.0, (name, key, ratio)
    # and the bounds are gat_ref's, widened by what the docstring derives: scale = 2 and one more u on constants of 10 and up
    plain = gat_ref.bounds(z, s_src, s_dst, cnt, d_out)
    for key in plain:
        assert bool((bound[key] >= 2 * plain[key]).all()) and bool((bound[key] <= 2.2 * plain[key]).all()), key


def test_the_host_stream_keeps_the_fraction_its_threshold_states():
    """A condition on the inputs of the GPU test's statistics: over the 13,000 slots x 3 heads of 'all hubs' the host decisions'
    kept fraction is within 4 standard deviations of 1 − threshold / 65536, for every p and seed the GPU tests use."""
    *_, rows, cols, rowptr, _ = _fixture_slots('all hubs')
    nnz, heads = rows.numel(), 3
    assert nnz == 13000
    for p in R.RANDOM_PS + (0.5,):
        q = 1.0 - dropout_ref.threshold(p) / 65536.0
        sd = (q * (1 - q) / (nnz * heads)) ** 0.5
        for seed in R.SEEDS:
            for off in R.OFFSETS:
                frac = R.decisions(nnz, heads, p, seed, off).mean()
                assert abs(frac - q) <= 4 * sd, (p, seed, off, frac, q)
    a, b = R.decisions(nnz, heads, 0.5, R.SEEDS[0], 0), R.decisions(nnz, heads, 0.5, R.SEEDS[0], 1)
    assert 0.4 < (a != b).mean() < 0.6                                    # one step of the counter: another mask


@pytest.mark.parametrize('heads,c', [(1, 8), (3, 6), (8, 8), (2, 5)])
def test_exact_graphs_reach_what_they_claim(heads, c):
    """Conditions on the graphs of the exact keep-set GPU tests: power-of-two rows, a parked row, starts off the Philox call's
    8-slot grid, the instantiation the shape is named for, decisions that differ between heads and between the two seeds."""
    ei, n, lengths = R.block_graph(c)
    rows, cols, rowptr, slot_t = R.slots(ei, n, False)
    assert (rowptr[1:] - rowptr[:-1])[:len(lengths)].tolist() == lengths and all(d & (d - 1) == 0 for d in lengths)
    assert {1, 2, 8, 16} <= set(lengths) and max(lengths) == (128 if c != 5 else 64) and max(lengths) <= 24 * c
    starts = rowptr[:len(lengths)].tolist()
    assert sum(1 for s in starts if s % 8) >= 5
    assert any(s % 8 and s // 8 != (s + d - 1) // 8 for s, d in zip(starts, lengths) if d <= 8)       # a short row across two calls
    assert c == 5 or any(s % 8 and d > 96 for s, d in zip(starts, lengths))                            # a parked row off the grid
    assert gat_ref.vec_lph(c, (heads * c,)) == {(1, 8): (4, 4), (3, 6): (2, 4), (8, 8): (4, 4), (2, 5): (1, 8)}[(heads, c)]
    for i, d in enumerate(lengths):
        assert cols[rowptr[i]:rowptr[i + 1]].tolist() == list(range(d))
    z = R.bit_values(n, heads, c)
    assert float(z.max()) == 2.0 ** 23 and int((z != 0).sum()) == min(n, 24 * c) * heads
    nnz = rows.numel()
    d0, d1 = R.decisions(nnz, heads, 0.5, R.SEEDS[0], 0), R.decisions(nnz, heads, 0.5, R.SEEDS[1], 0)
    assert (d0 != d1).mean() > 0.3 and (heads == 1 or (d0[:, 0] != d0[:, -1]).mean() > 0.3)
    want = R.keep_sets_forward(lengths, heads, c, d0)
    assert want.max() < 2 ** 24 and int(np.count_nonzero(want)) > 0
    back = R.keep_sets_backward(lengths, n, heads, d0)
    assert back.max() < 2 ** 24 and int(sum(bin(int(v)).count('1') for v in back.reshape(-1))) == int(d0.sum())
    # the transposed row of source j holds its targets in rising order: position by position through slot_t
    for j in (0, 1, 7):
        mine = slot_t[(cols[slot_t] == j)]
        assert rows[mine].tolist() == sorted(rows[mine].tolist()) and (cols[mine] == j).all()
