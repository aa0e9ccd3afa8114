"""The typed aggregation kernel pair (csrc/dcr_spmm.hip) through the raw ABI, and the R-GCN layer on them (models/rgcn.py).

Exact cases: ``val`` dyadic and small integers in the operands, so every fp32 operation is exact and the result must equal a
float64 numpy restatement bit for bit.  Random floats: the forward error bound of an fp32 ``fmaf`` sum against float64,
k·2⁻²⁴·Σ|terms| with k = (slots feeding the element) + 2 — one rounding per slot, one for the row's own block, one for the bias
(a hub row's strided sum puts no term through more additions than that, whatever the number of lane groups).  The bound is
derived, not tuned.  As measured on an MI355X the worst element sits at 0.64 of it (gather, width 260) and 0.45 (expand, width
64); at the widths 20, 13, 17, 10, 18, 34 and 66, one per (LPR, VEC) instantiation that narrower and wider widths leave out, at
0.55 (gather, widths 13 and 66) and 0.43 (expand, width 20).  The adjointness gap is 1.7e-6 and 8.0e-6 against bounds of 4.6e-2
and 4.3e-1.  Against the dense fp64 reference (tolerance 1e-5) the two-layer model on a FoSR output is at 5.5e-7; on the
140-node graph whose node 0 is a hub row of both CSRs a single layer is at 6.3e-7 at worst over its six variants and the
two-layer model at 2.2e-6.

The shapes live in tests/rgcn_shapes.py; tests/test_rgcn_cpu.py asserts that they launch all 15 instantiations of each kernel.
Beyond widths: operands viewed off 16-byte alignment, workgroups whose every row is a hub, a CSR whose relations exceed n_rel."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fosr_ref
import rgcn_ref
from rgcn_shapes import FULL_ROWS, N_FEATS, PADS, groups, leading_dims, row_counts, vec_lpr

pytestmark = pytest.mark.gpu

EINVAL = -1
U = 2.0 ** -24
N_COLS = 80                                   # rows of the gathered operand; >= every n_rows below (the self block reads row i)
# row lengths, most telling first: a prefix of this list is the graph at small n_rows.  'one': every slot of one relation.
PATTERN = [(400, 'mixed'), (0, 'mixed'), (3, 'one'), (97, 'mixed'), (300, 'one'), (96, 'mixed'), (95, 'mixed'), (1, 'one'), (0, 'mixed')]
HUB_COLS = 136                                # the all-hub family: the next multiple of 8 above its largest n_rows (2 * 64 + 1)
HUB_LENGTHS = (97, 130, 200, 98)
RANDOM_FEATS = (3, 64, 260, 20, 13, 17, 10, 18, 34, 66)
SPMM_LONG = 96                              # (SPMM_LONG of csrc/dcr_spmm.hip) rows above it are parked and summed by the whole workgroup


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


def hub_family(n_rows, n_rel, seed, dyadic):
    """COO slots of a graph in which EVERY row is a hub: lengths cycle through HUB_LENGTHS, one row in every four (its place
    moving on from four to four) holds a single relation."""
    rng = np.random.default_rng(seed)
    rows, cols, rels = [], [], []
    for i in range(n_rows):
        length = HUB_LENGTHS[i % 4]
        rows.append(np.full(length, i, dtype=np.int64))
        cols.append(rng.integers(0, HUB_COLS, length))
        rels.append(np.full(length, (i // 4) % n_rel) if i % 4 == (i // 4) % 4 else rng.integers(0, n_rel, length))
    rows, cols, rels = (np.concatenate(a).astype(np.int64) for a in (rows, cols, rels))
    vals = 0.5 ** rng.integers(0, 4, rows.size) if dyadic else rng.uniform(0.05, 1.0, rows.size)
    return rows, cols, rels, vals.astype(np.float32)


class Graph:
    def __init__(self, coo, n_rows, n_rel, n_cols=N_COLS):
        self.n_rows, self.n_rel, self.n_cols = n_rows, n_rel, n_cols
        self.A, self.cnt = dense(*coo, n_rows, n_rel, n_cols=n_cols)
        self.host = typed_csr(*coo, n_rows)
        self.dev = tuple(dev(a) for a in self.host)


_GRAPHS = {}


def graph(n_rows, n_rel, dyadic, seed=0):
    key = (n_rows, n_rel, dyadic, seed)
    if key not in _GRAPHS:
        _GRAPHS[key] = Graph(family(n_rows, n_rel, 100 * seed + 7 * n_rows + n_rel, dyadic), n_rows, n_rel)
    return _GRAPHS[key]


def hub_graph(n_rows, n_rel, dyadic):
    key = ('hub', n_rows, n_rel, dyadic)
    if key not in _GRAPHS:
        _GRAPHS[key] = Graph(hub_family(n_rows, n_rel, 1000 + 7 * n_rows + n_rel, dyadic), n_rows, n_rel, n_cols=HUB_COLS)
    return _GRAPHS[key]


class Operand:
    """[rows, ld] float32 on the device, viewed from element ``offset`` of a flat NaN-filled buffer: ``values`` (None: nothing)
    in the leading columns, NaN before the view and in the padding — never to be read, never to be written."""

    def __init__(self, rows, ld, values=None, offset=0):
        self.offset, self.rows, self.ld = offset, rows, ld
        if values is None:
            self.host, self.flat = None, torch.full((offset + rows * ld,), float('nan'), dtype=torch.float32, device='cuda')
        else:
            self.host = np.full(offset + rows * ld, np.nan, dtype=np.float32)
            self.host[offset:].reshape(rows, ld)[:, :values.shape[1]] = values
            self.flat = dev(self.host)
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat[offset:].view(rows, ld)

    def data_ptr(self):
        return self.view.data_ptr()

    def residue(self):
        return self.view.data_ptr() % 16

    def unchanged(self):
        return self.flat.cpu().numpy().tobytes() == self.host.tobytes()

    def read(self, width):
        """The leading ``width`` columns; everything else must still be NaN."""
        got = self.flat.cpu().numpy()
        out = got[self.offset:].reshape(self.rows, self.ld)
        assert np.isnan(got[:self.offset]).all() and np.isnan(out[:, width:]).all()
        return out[:, :width]


def padded(values, ld, offset=0):
    return Operand(values.shape[0], ld, values, offset)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def run_gather(lib, csr, B, n_rows, n_feat, n_rel, ldc, self_block, bias=None, relu=0, c_offset=0):
    """``B``: an Operand or a contiguous tensor."""
    C = Operand(n_rows, ldc, offset=c_offset)
    rc = lib.dcr_spmm_csr_typed_f32_dev(*(t.data_ptr() for t in csr), B.data_ptr(), C.data_ptr(), n_rows, n_feat, n_rel,
                                        B.ld if isinstance(B, Operand) else B.shape[1], ldc, self_block, ptr(bias), relu, stream())
    assert rc == 0, rc
    return C.read(n_feat)


def run_expand(lib, csr, Gm, n_rows, n_feat, n_rel, ldc, self_block, c_offset=0):
    C = Operand(n_rows, ldc, offset=c_offset)                      # (every block must be written over the NaN)
    rc = lib.dcr_spmm_csr_typed_expand_f32_dev(*(t.data_ptr() for t in csr), Gm.data_ptr(), C.data_ptr(), n_rows, n_feat, n_rel,
                                               Gm.ld if isinstance(Gm, Operand) else Gm.shape[1], ldc, self_block, stream())
    assert rc == 0, rc
    return C.read((n_rel + self_block) * n_feat)


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
        for pad in PADS:
            for self_block in (0, 1):
                wide, narrow = leading_dims(n_feat, n_rel, self_block, pad)
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
        for pad in PADS:
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
    # (3, 64, 260 and one width for each instantiation they and narrower widths leave out)
    assert {vec_lpr(f) for f in RANDOM_FEATS[3:]} == {(4, 8), (1, 16), (1, 32), (2, 8), (2, 16), (2, 32), (2, 64)}
    for n_feat in RANDOM_FEATS:
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


@pytest.mark.parametrize('n_feat', [64, 68])
def test_dispatch_on_pointer_alignment_exact_values(lib, n_feat):
    """Widths and leading dimensions that take VEC 4, operands viewed 4, 8 or 12 bytes off 16-byte alignment: the dispatch must
    step down to VEC 2 / VEC 1 (another LPR, another hub-row summation order: exact values, so the same bits) and touch nothing
    outside the views."""
    n_rel, rng = 3, np.random.default_rng(60 + n_feat)
    g = graph(FULL_ROWS, n_rel, True)
    for self_block in (0, 1):
        wide, narrow = leading_dims(n_feat, n_rel, self_block, 0)
        assert wide % 4 == 0 and narrow % 4 == 0 and vec_lpr(n_feat, wide, narrow)[0] == 4
        Bv = rng.integers(-4, 5, (N_COLS, wide)).astype(np.float32)
        Gv = rng.integers(-4, 5, (N_COLS, n_feat)).astype(np.float32)
        bias_v = rng.integers(-3, 4, n_feat).astype(np.float32)
        bias = dev(bias_v)
        want = gather_ref(g, Bv, n_feat, self_block)[0] + bias_v
        # the gather looks at B alone (its stores are scalar): C one float off changes nothing
        for b_off, c_off, vec in ((1, 0, 1), (2, 0, 2), (3, 0, 1), (0, 1, 4), (0, 0, 4)):
            B = padded(Bv, wide, b_off)
            assert B.residue() == 4 * b_off and vec_lpr(n_feat, wide, narrow, residues=(B.residue(),))[0] == vec
            got = run_gather(lib, g.dev, B, FULL_ROWS, n_feat, n_rel, narrow, self_block, bias, 0, c_offset=c_off)
            assert same_bits(got, want), ('gather', n_feat, self_block, b_off, c_off)
            assert B.unchanged()
        want, _ = expand_ref(g, Gv, n_feat, self_block)
        for g_off, c_off, vec in ((2, 0, 2), (0, 2, 2), (0, 1, 1), (2, 2, 2), (1, 0, 1), (0, 0, 4)):
            Gm = padded(Gv, narrow, g_off)
            assert vec_lpr(n_feat, wide, narrow, residues=(Gm.residue(), 4 * c_off))[0] == vec
            got = run_expand(lib, g.dev, Gm, FULL_ROWS, n_feat, n_rel, wide, self_block, c_offset=c_off)
            assert same_bits(got, want), ('expand', n_feat, self_block, g_off, c_off)
            assert Gm.unchanged()
    assert {vec_lpr(n_feat, residues=(r,)) for r in (0, 4, 8)} == {64: {(4, 16), (1, 64), (2, 32)}, 68: {(4, 32), (1, 64), (2, 64)}}[n_feat]


# one width per LPR; n_rows = G, 2G (every workgroup's parked list full: the kernels deal row sub·grid + block to group sub) and
# 2G + 1 (three workgroups, none full)
HUB_FEATS = {4: (4, 4), 7: (1, 8), 18: (2, 16), 68: (4, 32), 65: (1, 64)}


def hub_cases():
    for n_feat, want in HUB_FEATS.items():
        assert vec_lpr(n_feat) == want
        for n_rel in (3, 8):
            for self_block in (0, 1):
                wide, narrow = leading_dims(n_feat, n_rel, self_block, 0)
                assert vec_lpr(n_feat, wide, narrow) == want
                G = groups(n_feat, wide, narrow)
                for n_rows in (G, 2 * G, 2 * G + 1):
                    assert n_rows <= HUB_COLS
                    yield n_feat, n_rel, self_block, wide, narrow, G, n_rows


def parked_per_workgroup(rowptr, n_rows, G):
    """How many rows each workgroup parks: group ``sub`` of workgroup ``b`` owns row sub·grid + b."""
    grid = (n_rows + G - 1) // G
    lengths = np.diff(rowptr)
    return [sum(1 for sub in range(G) if sub * grid + b < n_rows and lengths[sub * grid + b] > SPMM_LONG) for b in range(grid)]


def test_every_row_a_hub_exact_values(lib):
    rng = np.random.default_rng(70)
    full = set()
    for n_feat, n_rel, self_block, wide, narrow, G, n_rows in hub_cases():
        g = hub_graph(n_rows, n_rel, True)
        parked = parked_per_workgroup(g.host[0], n_rows, G)
        assert sum(parked) == n_rows and (max(parked) == G) == (n_rows in (G, 2 * G))
        full |= {G} if max(parked) == G else set()
        label = (n_feat, n_rel, self_block, n_rows)
        Bv = rng.integers(-4, 5, (HUB_COLS, wide)).astype(np.float32)
        Gv = rng.integers(-4, 5, (HUB_COLS, n_feat)).astype(np.float32)
        bias_v = rng.integers(-3, 4, n_feat).astype(np.float32)
        got = run_gather(lib, g.dev, dev(Bv), n_rows, n_feat, n_rel, narrow, self_block, dev(bias_v), 0)
        assert same_bits(got, gather_ref(g, Bv, n_feat, self_block)[0] + bias_v), ('gather',) + label
        got = run_expand(lib, g.dev, dev(Gv), n_rows, n_feat, n_rel, wide, self_block)
        assert same_bits(got, expand_ref(g, Gv, n_feat, self_block)[0]), ('expand',) + label
        empty = g.cnt == 0                                         # [n_rel, n_rows]: the single-relation rows' other blocks
        assert empty.any()
        for r in range(n_rel):
            assert not got[empty[r], r * n_feat:(r + 1) * n_feat].any()
    assert full == {64, 32, 16, 8, 4}                              # a full parked list at every G


def test_every_row_a_hub_two_calls_give_the_same_bits(lib):
    """Random floats where the order in which a workgroup's rows are parked can differ from run to run: it must not show."""
    rng = np.random.default_rng(71)
    for n_feat, n_rel, self_block, wide, narrow, G, n_rows in hub_cases():
        g = hub_graph(n_rows, n_rel, False)
        B = dev(rng.standard_normal((HUB_COLS, wide)).astype(np.float32))
        Gm = dev(rng.standard_normal((HUB_COLS, n_feat)).astype(np.float32))
        first = run_gather(lib, g.dev, B, n_rows, n_feat, n_rel, narrow, self_block)
        assert np.isfinite(first).all() and first.tobytes() == run_gather(lib, g.dev, B, n_rows, n_feat, n_rel, narrow, self_block).tobytes()
        first = run_expand(lib, g.dev, Gm, n_rows, n_feat, n_rel, wide, self_block)
        assert np.isfinite(first).all() and first.tobytes() == run_expand(lib, g.dev, Gm, n_rows, n_feat, n_rel, wide, self_block).tobytes()


@pytest.mark.parametrize('n_feat', [6, 64])
def test_relation_above_n_rel_is_read_as_the_last(lib, n_feat):
    """The header's contract for a CSR that breaks ``rel[e] < n_rel``: such a slot counts as relation n_rel - 1.  Every buffer
    holds nine column blocks, NaN past those in use, so that a read or write at the slot's own relation would stay inside it
    and show as a NaN in the result or a number in the padding."""
    rng = np.random.default_rng(80 + n_feat)
    coo = family(FULL_ROWS, 8, 8 * FULL_ROWS, True)
    rows, cols, rels, vals = coo
    csr = typed_csr(*coo, FULL_ROWS)
    lengths = np.diff(csr[0])
    assert set(csr[3].tolist()) == set(range(8)) and lengths.max() > SPMM_LONG and 0 < lengths[lengths > 0].min() < 8
    csr_dev = tuple(dev(a) for a in csr)
    ld = 9 * n_feat + (-9 * n_feat) % 4                                          # (VEC 2 at 6, VEC 4 at 64, as an aligned call)
    for n_rel in (2, 3):
        clamped = Graph((rows, cols, np.minimum(rels, n_rel - 1), vals), FULL_ROWS, n_rel)
        assert (clamped.host[3] == np.minimum(csr[3], n_rel - 1)).all()          # a clamped row is still sorted
        for self_block in (0, 1):
            used = (n_rel + self_block) * n_feat
            assert vec_lpr(n_feat, ld, n_feat)[0] == (4 if n_feat % 4 == 0 else 2)
            Bv = rng.integers(-4, 5, (N_COLS, used)).astype(np.float32)
            Gv = rng.integers(-4, 5, (N_COLS, n_feat)).astype(np.float32)
            B = padded(Bv, ld)
            got = run_gather(lib, csr_dev, B, FULL_ROWS, n_feat, n_rel, n_feat, self_block)
            assert same_bits(got, gather_ref(clamped, Bv, n_feat, self_block)[0]), ('gather', n_feat, n_rel, self_block)
            got = run_expand(lib, csr_dev, dev(Gv), FULL_ROWS, n_feat, n_rel, ld, self_block)   # (asserts C's other columns NaN)
            assert same_bits(got, expand_ref(clamped, Gv, n_feat, self_block)[0]), ('expand', n_feat, n_rel, self_block)


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


HUB_N = 140


@pytest.fixture(scope='module')
def hub_data():
    """A directed graph whose node 0 is a hub row of BOTH CSRs of ``rgcn_norm_csr`` (104 in-edges from nodes 1..104, 104
    out-edges to nodes 36..139), three relations, duplicated columns, self-loops, node 1 without an in-edge; not symmetric."""
    from dcr.data import Data
    from models.rgcn import rgcn_norm_csr
    n, rng = HUB_N, np.random.default_rng(90)
    into = np.stack([np.arange(1, 105), np.zeros(104, dtype=np.int64)])
    out_of = np.stack([np.zeros(104, dtype=np.int64), np.arange(36, 140)])
    rnd = np.stack([rng.integers(0, n, 300), rng.integers(2, n, 300)])
    dup = np.concatenate([into[:, :7], out_of[:, :5], rnd[:, :9]], 1)
    loops = np.array([[0, 7, 7, 50], [0, 7, 7, 50]])
    ei = torch.from_numpy(np.concatenate([into, out_of, rnd, dup, loops], 1))
    et = torch.from_numpy(rng.integers(0, 3, ei.shape[1]))
    csr = rgcn_norm_csr(ei, et, n, 3)
    deg_in, deg_out = (csr.rowptr[1:] - csr.rowptr[:-1]), (csr.rowptr_t[1:] - csr.rowptr_t[:-1])
    assert int(deg_in[0]) > SPMM_LONG and int(deg_out[0]) > SPMM_LONG and int(deg_in[1]) == 0
    assert not torch.equal(csr.rowptr, csr.rowptr_t) and not torch.equal(csr.col, csr.col_t)
    assert set(csr.rel[:int(deg_in[0])].tolist()) == {0, 1, 2} and set(csr.rel_t[:int(deg_out[0])].tolist()) == {0, 1, 2}
    g = torch.Generator().manual_seed(6)
    x = torch.randn(n, 10, generator=g)
    y = torch.randint(0, 3, (n,), generator=g)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[torch.randperm(n, generator=g)[:n // 2]] = True
    mask[0] = True                                                               # the hub's own row carries a gradient
    data = Data(x=x, edge_index=ei, y=y, num_nodes=n, edge_type=et, train_mask=mask, val_mask=~mask).to('cuda')
    return data, rgcn_ref.relation_means(ei, et, n, 3)


def _layer_step(conv, data):
    """Output and gradients of loss = nll_loss(log_softmax(conv(x))[train], y[train]) with respect to x and the parameters."""
    conv.zero_grad()
    x = data.x.clone().requires_grad_(True)
    out = conv(x, data.edge_index, data.edge_type)
    torch.nn.functional.nll_loss(torch.log_softmax(out, 1)[data.train_mask], data.y[data.train_mask]).backward()
    got = {'out': out, 'x': x.grad, **{k: p.grad for k, p in conv.named_parameters()}}
    return {k: v.detach().double().cpu() for k, v in got.items()}


@pytest.mark.parametrize('root_weight,bias', [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize('out_channels', [6, 3])
def test_layer_on_hub_rows_of_both_csrs_matches_the_dense_reference(hub_data, out_channels, root_weight, bias):
    """RGCNConv forward (a hub row of ``rowptr``) and backward (a hub row of ``rowptr_t``) on a graph that is not symmetric, at
    VEC 2 (6 channels) and VEC 1 (3), with and without the root block and the bias."""
    from models import gcn
    from models.rgcn import RGCNConv
    data, means = hub_data
    assert vec_lpr(out_channels, (3 + root_weight) * out_channels, out_channels)[0] == (2 if out_channels == 6 else 1)
    torch.manual_seed(7)
    conv = RGCNConv(10, out_channels, 3, root_weight=root_weight, bias=bias)
    if bias:
        with torch.no_grad():
            conv.bias.uniform_(-0.5, 0.5)
    leaves = {k: p.detach().double().clone().requires_grad_(True) for k, p in conv.named_parameters()}
    leaves['x'] = data.x.cpu().double().requires_grad_(True)
    out = rgcn_ref.layer(leaves['x'], means, leaves['weight'], leaves.get('root'), leaves.get('bias'))
    torch.nn.functional.nll_loss(torch.log_softmax(out, 1)[data.train_mask.cpu()], data.y.cpu()[data.train_mask.cpu()]).backward()
    want = {'out': out.detach(), **{k: v.grad for k, v in leaves.items()}}
    assert set(want) == {'out', 'x', 'weight'} | ({'root'} if root_weight else set()) | ({'bias'} if bias else set())
    conv = conv.cuda()
    got = _layer_step(conv, data)
    worst = max(float((got[k] - want[k]).abs().max()) for k in want)
    print(f'RGCNConv(10, {out_channels}, 3, root_weight={root_weight}, bias={bias}) on hub rows against dense fp64: worst difference {worst:.3e}')
    for k in want:
        assert got[k].shape == want[k].shape and (got[k] - want[k]).abs().max() < 1e-5, k
    assert float(want['x'][0].abs().max()) > 0.0 and float(want['x'][1].abs().max()) > 0.0
    gcn.set_aggregate_backend('torch')
    try:
        got_t = _layer_step(conv, data)
    finally:
        gcn.set_aggregate_backend('hip')
    for k in want:
        assert (got[k] - got_t[k]).abs().max() < 1e-5, k


def test_model_on_hub_rows_of_both_csrs_matches_the_dense_reference(hub_data):
    from dcr.data import Dataset
    from models import gcn
    from models.rgcn import RGCN
    data, _ = hub_data
    torch.manual_seed(8)
    model = RGCN(Dataset(data, 3), num_relations=3, hidden=[6], dropout=0.0).cuda()
    with torch.no_grad():
        for conv in model.layers:
            conv.bias.uniform_(-0.5, 0.5)
    want_lp, want_grad = rgcn_ref.model_reference(model.state_dict(), data.x, data.edge_index, data.edge_type, 3, data.y, data.train_mask)
    lp, grad = _logits_and_grads(model, data)
    worst = max([float((lp - want_lp).abs().max())] + [float((grad[k] - want_grad[k]).abs().max()) for k in grad])
    print(f'RGCN on hub rows against the dense fp64 reference: worst difference {worst:.3e}')
    assert (lp - want_lp).abs().max() < 1e-5
    assert set(grad) == set(want_grad)
    for k in grad:
        assert (grad[k] - want_grad[k]).abs().max() < 1e-5, k
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
