"""The summation order of every CSR aggregation entry point (csrc/dcr_spmm.hip), bit for bit against its host restatement
(tests/spmm_order_ref.py): weights powers of two, random fp32 operands, so a product is exact, a fused multiply-add is one fp32
addition, and any other order of the additions shows in the bits.  One graph whose rows sit on both sides of the long-row
threshold, one width per LPR (the number of lane groups a long row is dealt to) and the benchmark's hidden width."""
import ctypes

import numpy as np
import pytest
import torch

import spmm_order_ref as ref

pytestmark = pytest.mark.gpu

WIDTHS = sorted(ref.WIDTHS)


@pytest.fixture(scope='module')
def lib():
    from dcr import _lib
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptrs(*tensors):
    return [None if t is None else t.data_ptr() for t in tensors]


def out(rows, cols):
    return torch.full((rows, cols), float('nan'), dtype=torch.float32, device='cuda')


def same_bits(got, want, label):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, label
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (label, len(bad), bad[:5].tolist())


class Case:
    """One graph per n_rel, on the host and on the device; operands and the replica's row sums per width, computed once."""

    def __init__(self, n_rel):
        self.n_rel = n_rel
        self.host = ref.typed_graph(n_rel)
        self.dev = [dev(a) for a in self.host]
        self._plain = {}

    def plain(self, n_feat):
        """(B two blocks wide, bias, the replica's sums of block 0 and of block 1)."""
        if n_feat not in self._plain:
            rng = np.random.default_rng(n_feat)
            B = rng.standard_normal((ref.N_COLS, 2 * n_feat)).astype(np.float32)
            bias = rng.standard_normal(n_feat).astype(np.float32)
            rowptr, col, val, _ = self.host
            G = ref.groups(n_feat, 2 * n_feat, n_feat)
            assert ref.vec_lpr(n_feat, 2 * n_feat, n_feat) == ref.WIDTHS[n_feat]
            self._plain[n_feat] = (B, bias, [ref.plain_sums(rowptr, col, val, np.ascontiguousarray(B[:, k * n_feat:(k + 1) * n_feat]), G)
                                             for k in (0, 1)])
        return self._plain[n_feat]


@pytest.fixture(scope='module')
def cases():
    made = {}

    def get(n_rel):
        if n_rel not in made:
            made[n_rel] = Case(n_rel)
        return made[n_rel]
    return get


@pytest.mark.parametrize('n_feat', WIDTHS)
def test_plain_and_pair_calls(lib, cases, n_feat):
    case = cases(3)
    B, bias, sums = case.plain(n_feat)
    csr = ptrs(*case.dev[:3])
    d_B, d_bias, n, ldb = dev(B), dev(bias), ref.N_ROWS, 2 * n_feat
    for with_bias, relu in ((False, 0), (True, 0), (True, 1), (False, 1)):
        b = bias if with_bias else None
        want = [ref.close(s, bias=b, relu=bool(relu)) for s in sums]
        label = (n_feat, with_bias, relu)
        C = out(n, n_feat)
        assert lib.dcr_spmm_csr_f32_dev(*csr, d_B.data_ptr(), C.data_ptr(), n, n_feat, ldb, n_feat, *ptrs(d_bias if with_bias else None), relu,
                                        stream()) == 0
        same_bits(C, want[0], ('single',) + label)
        # the second column block as an operand of its own (n_feat floats in: as aligned as the width lets VEC ask for)
        assert ref.vec_lpr(n_feat, ldb, n_feat, residues=((4 * n_feat) % 16,)) == ref.WIDTHS[n_feat]
        C = out(n, n_feat)
        assert lib.dcr_spmm_csr_f32_dev(*csr, d_B.data_ptr() + 4 * n_feat, C.data_ptr(), n, n_feat, ldb, n_feat,
                                        *ptrs(d_bias if with_bias else None), relu, stream()) == 0
        same_bits(C, want[1], ('single, block 1',) + label)
        P = out(n, 2 * n_feat)
        assert lib.dcr_spmm_csr_f32_pair_dev(*csr, d_B.data_ptr(), P.data_ptr(), n, n_feat, ldb, 2 * n_feat, *ptrs(d_bias if with_bias else None),
                                             relu, stream()) == 0
        same_bits(P, np.concatenate(want, axis=1), ('pair',) + label)
        # two outputs of their own, a multiple of four floats apart
        flat = out(1, 2 * n * n_feat + 4).view(-1)
        gap = -(-n * n_feat // 4) * 4
        C0, C1 = flat[:n * n_feat].view(n, n_feat), flat[gap:gap + n * n_feat].view(n, n_feat)
        assert lib.dcr_spmm_csr_f32_pair_split_dev(*csr, d_B.data_ptr(), C0.data_ptr(), C1.data_ptr(), n, n_feat, ldb, n_feat,
                                                   *ptrs(d_bias if with_bias else None), relu, stream()) == 0
        same_bits(C0, want[0], ('pair split, 0',) + label)
        same_bits(C1, want[1], ('pair split, 1',) + label)


@pytest.mark.parametrize('n_feat', WIDTHS)
def test_row_lists(lib, cases, n_feat):
    """Hub rows (0, 5, 6, 7) and short ones in both lists, out of order, one of them twice."""
    case = cases(3)
    B, bias, sums = case.plain(n_feat)
    csr = ptrs(*case.dev[:3])
    d_B, d_bias, ldb = dev(B), dev(bias), 2 * n_feat
    first = np.array([7, 3, 0, 69, 1, 5, 4, 6, 33, 0], dtype=np.int64)
    second = np.array([6, 5, 2, 0, 68, 7, 4, 1], dtype=np.int64)
    both = np.concatenate([first, second])
    d_rows = dev(both)
    C = out(both.size, n_feat)
    assert lib.dcr_spmm_csr_rows_f32_dev(*csr, d_rows.data_ptr(), both.size, d_B.data_ptr(), C.data_ptr(), n_feat, ldb, n_feat, d_bias.data_ptr(), 0,
                                         stream()) == 0
    same_bits(C, ref.close(sums[0][both], bias=bias), ('rows', n_feat))
    # the second list reads the second column block; b_off2 = n_feat keeps the alignment the width allows
    assert ref.vec_lpr(n_feat, ldb, n_feat, residues=((4 * n_feat) % 16,)) == ref.WIDTHS[n_feat]
    C = out(both.size, n_feat)
    assert lib.dcr_spmm_csr_rows2_f32_dev(*csr, d_rows.data_ptr(), first.size, both.size, d_B.data_ptr(), n_feat, C.data_ptr(), n_feat, ldb, n_feat,
                                          d_bias.data_ptr(), 1, stream()) == 0
    want = np.concatenate([sums[0][first], sums[1][second]])
    same_bits(C, ref.close(want, bias=bias, relu=True), ('rows2', n_feat))


@pytest.mark.parametrize('n_feat', WIDTHS)
@pytest.mark.parametrize('n_rel', (1, 3))
def test_typed_gather_and_expand(lib, cases, n_rel, n_feat):
    case = cases(n_rel)
    rowptr, col, val, rel = case.host
    csr = ptrs(*case.dev)
    rng = np.random.default_rng(100 * n_rel + n_feat)
    n = ref.N_ROWS
    for self_block in (0, 1):
        ldw = (n_rel + self_block) * n_feat
        wide = rng.standard_normal((ref.N_COLS, ldw)).astype(np.float32)
        bias = rng.standard_normal(n_feat).astype(np.float32)
        Gm = rng.standard_normal((ref.N_COLS, n_feat)).astype(np.float32)
        G = ref.groups(n_feat, ldw, n_feat)
        assert ref.vec_lpr(n_feat, ldw, n_feat) == ref.WIDTHS[n_feat]
        sums = ref.typed_gather_sums(rowptr, col, val, rel, wide, n_feat, G)
        own = wide[:n, n_rel * n_feat:] if self_block else None
        d_wide, d_bias, d_G = dev(wide), dev(bias), dev(Gm)
        for with_bias, relu in ((False, 0), (True, 1)):
            C = out(n, n_feat)
            assert lib.dcr_spmm_csr_typed_f32_dev(*csr, d_wide.data_ptr(), C.data_ptr(), n, n_feat, n_rel, ldw, n_feat, self_block,
                                                  *ptrs(d_bias if with_bias else None), relu, stream()) == 0
            same_bits(C, ref.close(sums, own=own, bias=bias if with_bias else None, relu=bool(relu)),
                      ('gather', n_rel, n_feat, self_block, with_bias, relu))
        C = out(n, ldw)
        assert lib.dcr_spmm_csr_typed_expand_f32_dev(*csr, d_G.data_ptr(), C.data_ptr(), n, n_feat, n_rel, n_feat, ldw, self_block, stream()) == 0
        same_bits(C, ref.typed_expand(rowptr, col, val, rel, Gm, n_rel, G, self_block), ('expand', n_rel, n_feat, self_block))
