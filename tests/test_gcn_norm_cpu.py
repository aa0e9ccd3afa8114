"""models/gcn.py::gcn_norm_csr (torch ops, no GPU) against the float64 restatement of PyG 2.0.3 ``gcn_norm`` in
tests/gcn_fp64.py, on edge lists with weights, self-loops already in the input, a zero-degree node, duplicates and isolated
nodes: a normalisation error shows here before any kernel sees it."""
import pytest
import torch

from gcn_fp64 import dense_a_hat, hand_built_graph, weighted_powerlaw_graph


def _dense(rowptr, col, val, n_rows, n_cols):
    counts = rowptr[1:] - rowptr[:-1]
    rows = torch.repeat_interleave(torch.arange(n_rows), counts)
    a = torch.zeros((n_rows, n_cols), dtype=torch.float64)
    a.index_put_((rows, col.long()), val.double(), accumulate=True)
    return a


@pytest.mark.parametrize('case', ['hand_built', 'hand_built_unit', 'powerlaw'])
def test_gcn_norm_csr_against_fp64(case):
    from models.gcn import gcn_norm_csr
    ei, w, n = weighted_powerlaw_graph() if case == 'powerlaw' else hand_built_graph()
    if case == 'hand_built_unit':
        w = None
    csr = gcn_norm_csr(ei, w, n)
    want = dense_a_hat(ei, w, n)
    got = _dense(csr.rowptr, csr.col, csr.val, n, n)
    got_t = _dense(csr.rowptr_t, csr.col_t, csr.val_t, n, n)
    assert (got - want).abs().max().item() <= 2e-6 * want.abs().max().item()
    assert ((got - want).abs() <= 2e-6 * want.abs()).all()
    assert torch.equal(got_t, got.t())
    # one entry per (target, source) pair of the input plus one loop per node: duplicates are kept, not merged
    loops = int((ei[0] == ei[1]).sum())
    assert int(csr.rowptr[-1]) == ei.shape[1] - loops + n
    if case != 'powerlaw':
        if w is not None:
            assert want[290].abs().sum().item() == 0 and got[290].abs().sum().item() == 0      # deg 0: the row is empty in value
            assert want[203, 203].item() != 0 and abs(got[203, 203].item() - want[203, 203].item()) <= 1e-7 * want[203, 203].item()
        assert int(csr.rowptr[1] - csr.rowptr[0]) == 96 and int(csr.rowptr[101] - csr.rowptr[100]) == 97
        assert all(got[i].abs().sum().item() == got[i, i].item() == want[i, i].item() == 1.0 for i in range(291, 300))


def test_unit_weights_give_the_same_bits_as_none():
    from models.gcn import gcn_norm_csr
    ei, _, n = hand_built_graph()
    a, b = gcn_norm_csr(ei, None, n), gcn_norm_csr(ei, torch.ones(ei.shape[1]), n)
    for k in ('rowptr', 'col', 'val', 'rowptr_t', 'col_t', 'val_t'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
