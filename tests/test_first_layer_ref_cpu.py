"""tests/first_layer_ref.py, the inputs of tests/test_first_layer_exact_gpu.py, checked without a GPU: fp32 emulations that add
in the groupings of csrc/dcr_gcn_first.hip's kernels, in scrambled orders, equal the int64 references bit for bit on these
operands, and each planted mistake of the kind those kernels could make — a dropped 16-row unit, a K chunk added twice, a chunk
skipped, a stage multiplying the previous stage's rows of Â·X, a keep bit taken one column on, a pad column let into dW1, b1
added once per chunk — makes at least one entry differ.  So ``==`` on the GPU means what it says.  The exactness guard (every
output entry's sum of absolute products below 2**24) is run here for every shape the GPU file uses, at the MI355X's 256 CUs and
at a smaller device's plan, so a shape that cannot be exact fails here and not on the GPU; and the plan restatements are held
against the source lines they cite."""
import os

import numpy as np
import pytest
import torch

import dropout_ref
import first_layer_ref as fr
from conftest import PKG

# (n, feats, hidden, classes): three / three / five K chunks, the last one 16 / 80 / 16 columns wide
FWD_SHAPES = [(70, 272, 128, 7), (65, 592, 64, 16), (40, 528, 128, 1)]
# (n, feats, hidden, classes, workgroups): feats no multiple of 16 (a pad column exists), 3 … 4 stages, a ragged last one
BWD_SHAPES = [(70, 23, 64, 7, 2), (100, 277, 128, 16, 3), (75, 37, 128, 1, 3)]


def eq(got, want):
    """The comparison the GPU tests make: by value, every entry."""
    return torch.equal(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(want, dtype=np.float32)))


def forward_case(n, feats, hidden, classes, p):
    ops = fr.forward_operands(n, feats, hidden, classes, seed=n + feats)
    pre = fr.forward_pre(ops)
    keep = dropout_ref.decisions(n * hidden, p, 5, 7).reshape(n, hidden) & (pre > 0)
    return ops, keep, fr.forward_reference(ops, keep, fr.scale_of(p))


@pytest.mark.parametrize('n,feats,hidden,classes', FWD_SHAPES)
def test_scrambled_fp32_forward_is_the_integer_result(n, feats, hidden, classes):
    for p in (0.0, 0.5):
        ops, keep, want = forward_case(n, feats, hidden, classes, p)
        assert (want[0] > 0).any() and (want[0] < 0).any() and (want[0] == 0).any()
        assert p == 0.0 or (keep != (want[0] > 0)).any()
        for seed in (1, 2, 3):
            got = fr.emulate_forward(ops, keep, fr.scale_of(p), seed)
            assert all(eq(g, w) for g, w in zip(got, want)), (p, seed)


@pytest.mark.parametrize('fault', fr.FORWARD_FAULTS)
@pytest.mark.parametrize('n,feats,hidden,classes', FWD_SHAPES)
def test_planted_forward_fault_is_seen(n, feats, hidden, classes, fault):
    ops, keep, want = forward_case(n, feats, hidden, classes, 0.5)
    pre, z_tr, z_ev = fr.emulate_forward(ops, keep, 2, 1, fault)
    if fault == 'keep_bit_one_column_on':
        assert eq(pre, want[0]) and eq(z_ev, want[2]) and not eq(z_tr, want[1])
    else:
        assert not eq(pre, want[0]) and not eq(z_tr, want[1]) and not eq(z_ev, want[2])


@pytest.mark.parametrize('n,feats,hidden,classes,blocks', BWD_SHAPES)
def test_scrambled_fp32_backward_is_the_integer_result(n, feats, hidden, classes, blocks):
    for p, dense_every in ((0.0, 1), (0.5, 4)):
        ops = fr.backward_operands(n, feats, hidden, classes, seed=n, dense_every=dense_every)
        _, db1, dw2, dw1 = fr.backward_reference(ops, fr.scale_of(p))
        assert (ops['keep'] & (ops['pre'] <= 0)).any() and (~ops['keep'] & (ops['pre'] > 0)).any()    # the mask is not the sign of pre
        for seed in (1, 2, 3):
            got = fr.emulate_backward(ops, fr.scale_of(p), blocks, seed)
            assert eq(got[0], db1) and eq(got[1], dw2) and eq(got[2], dw1), (p, seed)


@pytest.mark.parametrize('fault', fr.BACKWARD_FAULTS)
@pytest.mark.parametrize('n,feats,hidden,classes,blocks', BWD_SHAPES)
def test_planted_backward_fault_is_seen(n, feats, hidden, classes, blocks, fault):
    for dense_every in (1, 4):
        ops = fr.backward_operands(n, feats, hidden, classes, seed=n, dense_every=dense_every)
        _, db1, dw2, dw1 = fr.backward_reference(ops, 2)
        got = fr.emulate_backward(ops, 2, blocks, 1, fault)
        assert not eq(got[2], dw1), dense_every                        # every one of them shows in dW1
        if fault in ('unit_dropped', 'keep_bit_one_column_on'):
            assert not eq(got[0], db1) and not eq(got[1], dw2), dense_every
        else:
            assert eq(got[0], db1) and eq(got[1], dw2), dense_every


def test_thin_dz_rows_leave_no_row_out():
    rng = np.random.default_rng(0)
    dz = fr.dz_rows(200, 7, rng, dense_every=4)
    assert dz.min() == -2 and dz.max() == 2 and (np.abs(dz).sum(1) > 0).all()
    thin = np.arange(200) % 4 != 0
    assert ((dz[thin] != 0).sum(1) == 1).all() and ((dz[~thin] != 0).sum(1) > 1).any()
    one = fr.dz_rows(50, 1, rng, dense_every=4)
    assert one.shape == (50, 1) and (one[np.arange(50) % 4 != 0] != 0).all()


def test_buffers_are_zero_padded_to_16_and_nan_beyond():
    ops = fr.forward_operands(5, 23, 64, 7, seed=0)
    buf = fr.ax_buffer(ops['ax'])
    assert tuple(buf.shape) == (5 + 16, 32 + 8) and buf.dtype == torch.float32
    assert np.array_equal(buf[:5, :23].numpy(), ops['ax'].astype(np.float32)) and not buf[:5, 23:32].any()
    assert torch.isnan(buf[:, 32:]).all() and torch.isnan(buf[5:]).all()
    rows = fr.rows_buffer(ops['w2'])
    assert tuple(rows.shape) == (7 + 16, 64) and torch.isnan(rows[7:]).all() and not torch.isnan(rows[:7]).any()
    for key, lo, hi in (('ax', -2, 2), ('w1', -2, 2), ('b1', -3, 3), ('w2', -1, 1)):
        assert ops[key].dtype == np.int64 and ops[key].min() == lo and ops[key].max() == hi
    b = fr.backward_operands(40, 23, 64, 7, seed=0)
    assert b['dz'].min() == -2 and b['dz'].max() == 2 and b['pre'].min() == -4 and b['pre'].max() == 4
    words = fr.pack_keep(b['keep'])
    need = dropout_ref.bits_words(40 * 64)
    assert words.numel() == need + 4 and not words[need:].any()
    assert np.array_equal(dropout_ref.unpack_bits(words.numpy().view(np.uint64), 40 * 64), b['keep'].reshape(-1))


def test_exactness_guard_refuses_what_cannot_be_exact():
    assert fr.assert_exact('x', np.array([[2 ** 24 - 1]])) == 2 ** 24 - 1
    with pytest.raises(AssertionError):
        fr.assert_exact('x', np.array([[3, 2 ** 24]]))
    ops = fr.backward_operands(64, 16, 64, 1, seed=0)
    ops['pre'] = ops['pre'] * 2 ** 20                                   # dW2 would add products of 2**21 and more
    with pytest.raises(AssertionError):
        fr.backward_reference(ops, 2)
    ops = fr.forward_operands(4, 16, 64, 1, seed=0)
    with pytest.raises(AssertionError):                                # a keep bit on an entry that is not positive
        fr.forward_reference(ops, np.ones((4, 64), dtype=bool), 1)


# ---- the guard at every shape of the GPU file ----------------------------------------------------------------------------------
def guard_forward(n, feats, hidden, classes):
    ops = fr.forward_case_operands(n, feats, hidden, classes)
    fr.forward_reference(ops, fr.forward_pre(ops) > 0, 2)               # (the guard of z bounds every mask by this one; scale 2)


@pytest.mark.parametrize('cus', [256, 64])
def test_every_gpu_forward_shape_is_exact(cus):
    for feats, hidden in fr.RESIDENT_SHAPES:
        assert fr.first_layer_resident(feats, hidden)
        for classes in fr.CLASSES:
            for n in fr.RESIDENT_ROWS:
                guard_forward(n, feats, hidden, classes)
    for n in (fr.resident_rows_pair_then_single(cus), fr.resident_rows_prefetch(cus)):
        assert n <= fr.ROW_LIMIT
        guard_forward(n, 16, 128, 7)
    for k, (hidden, feats, chunks) in enumerate(fr.WIDE_SHAPES):
        assert not fr.first_layer_resident(feats, hidden) and fr.wide_chunks(feats, hidden) == chunks
        for n in fr.WIDE_ROWS:
            guard_forward(n, feats, hidden, fr.CLASSES[k % 3])
    feats, hidden = fr.WIDE_WALK
    guard_forward(fr.wide_walk_rows(cus), feats, hidden, 7)


@pytest.mark.parametrize('cus', [256, 64])
def test_every_gpu_backward_shape_is_exact(cus):
    for feats in fr.BWD_SMALL_FEATS:
        for hidden in (64, 128):
            for classes in fr.CLASSES:
                for residue in fr.BWD_RESIDUES:
                    fr.backward_reference(fr.backward_case_operands(64 + residue, feats, hidden, classes), 2)
    for hidden, classes, s, residue, n in fr.bwd_deep_cases(cus):
        assert n <= fr.ROW_LIMIT
        fr.backward_reference(fr.backward_case_operands(n, fr.BWD_DEEP_FEATS, hidden, classes), 2)
    for feats, hidden, classes, s, residue in fr.BWD_PIPELINE_EXTRA:
        n = fr.bwd_rows_for(s, residue, feats, cus)
        assert n <= fr.ROW_LIMIT
        fr.backward_reference(fr.backward_case_operands(n, feats, hidden, classes), 2)


# ---- the plans -----------------------------------------------------------------------------------------------------------------
def test_cited_source_lines_say_what_the_restatements_say():
    lines = open(os.path.join(PKG, 'csrc', 'dcr_gcn_first.hip')).read().split('\n')
    for number, text in fr.CITED.items():
        assert text in lines[number - 1], (number, lines[number - 1])
    assert '#define DCR_FIRST_NR 2' in lines[30] and '#define DCR_FIRST_WAVES 8' in lines[33]
    assert '#define DCR_BWD_WAVES 8' in lines[651] and '#define DCR_BWD_UR 2' in lines[654]


def test_plans_at_256_cus():
    cus = 256
    # resident: hidden 128 up to 256 columns, hidden 64 up to 576; no width that is not a multiple of 16
    assert [f for f in range(16, 700, 16) if fr.first_layer_resident(f, 128)] == list(range(16, 257, 16))
    assert [f for f in range(16, 700, 16) if fr.first_layer_resident(f, 64)] == list(range(16, 577, 16))
    assert not fr.first_layer_resident(23, 128) and not fr.first_layer_resident(8, 64)
    # a wave's range: at most 2 units while the grid still grows, 3 = a pair and a single one just past 256 CUs x 16 units
    for n_units in range(1, 16 * cus + 1):
        assert max(fr.resident_wave_units(16 * n_units, cus)) <= 2
    n = fr.resident_rows_pair_then_single(cus)
    assert n == 65537 and sorted(set(fr.resident_wave_units(n, cus))) == [2, 3] and max(fr.resident_wave_units(n - 1, cus)) == 2
    n = fr.resident_rows_prefetch(cus)
    assert n == 98305 and sorted(set(fr.resident_wave_units(n, cus))) == [1, 4] and max(fr.resident_wave_units(n - 1, cus)) == 3
    # K chunks, chunks in flight in the closing loop, row groups
    assert fr.wide_in_flight(128) == 4 and fr.wide_in_flight(64) == 8
    assert [fr.wide_chunks(f, h) for h, f, _ in fr.WIDE_SHAPES] == [1, 3, 4, 5, 9, 3, 7, 8, 9, 17]
    assert [fr.wide_groups(n) for n in (1, 63, 64, 65)] == [1, 1, 1, 2]
    assert fr.wide_ws_floats(65, 272, 128) == 3 * 80 * 128 + 2
    assert fr.wide_walk_rows(cus) == 31 * 64 + 1 and fr.wide_gx(31 * 64 + 1, 4112, 64, cus) == 31 and fr.wide_groups(31 * 64 + 1) == 32
    assert fr.wide_gx(65, 4112, 64, cus) == 2 and fr.wide_gx(65, 23, 128, cus) == 2
    # backward: 18 workgroups along the rows at 15 column blocks; stages per workgroup 1 … 4 within 2,300 rows
    assert fr.bwd_blocks(5003, 300, cus) == 128 and fr.bwd_stages_per_wg(5003, 300, cus) == 2
    assert fr.bwd_blocks(5003, 23, cus) == 157 and fr.bwd_stages_per_wg(5003, 23, cus) == 1
    deep = fr.bwd_deep_cases(cus)
    assert len(deep) == 24 and max(c[4] for c in deep) == 32 * 70 + 32
    for s in fr.BWD_STAGES_PER_WG:
        mine = [c for c in deep if c[2] == s]
        assert sorted(c[3] for c in mine) == sorted(fr.BWD_RESIDUES)                  # every residue at every depth
        for hidden, classes, _, residue, n in mine:
            assert fr.bwd_blocks(n, 3703, cus) == 18 and fr.bwd_stages(n) == (18 if s == 1 else 18 * s - 1)
            assert (n - 1) % 32 + 1 == residue
            assert fr.bwd_ws_floats(n, 3703, hidden, cus) == 18 * (hidden * 3712 + 17 * hidden)
