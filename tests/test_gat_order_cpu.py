"""The conditions on the host replica of the attention kernels' order (tests/gat_order_ref.py) and on the fixtures that
tests/test_gat_limits_gpu.py runs: the replica's fmaf is exact where the twice-rounded one is not, the replica is a valid fp32
evaluation (within the derived bounds of the fp64 restatement), every other order of a row would give other bits on these
operands, the ladder holds the lengths it claims, and the shapes reach the instantiations they are named for.  No GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import gat_order_ref as R
import gat_ref
from conftest import PKG

F32 = np.float32


def _source(name):
    return open(os.path.join(PKG, 'csrc', name)).read()


def test_constants_are_the_kernels():
    gat, pieces = _source('dcr_gat.hip'), _source('dcr_spmm_pieces.h')
    assert int(re.search(r'constexpr\s+int\s+GAT_LONG\s*=\s*(\d+)\s*;', gat).group(1)) == R.GAT_LONG
    assert int(re.search(r'constexpr\s+int\s+DST_LPR\s*=\s*(\d+)\s*;', gat).group(1)) == R.DST_LPR
    assert 'static constexpr int G = 256 / LPR;' in pieces and 'static constexpr int U = LPR <= 8 ? 8 : 4;' in pieces
    assert [R.groups(l) * R.in_flight(l) for l in gat_ref.LPHS] == [512, 256, 64, 32, 16]
    assert '-ffp-contract=off' in _source('build.sh')


# ---- the exact fmaf ----------------------------------------------------------------------------------------------------------
# a·b is a midpoint of the fp32 grid (1.5 + an odd multiple of 2^-24) and c pushes it off by far less than fp64 resolves: the
# fp64 sum lands ON the midpoint and its second rounding goes to the even neighbour, the exact result is the odd one.
E23 = 2.0 ** -23
TRIPLES = [
    (1 + E23, 1.5, -2.0 ** -60, 1.5 + E23),             # 1.5 + 3·2^-24 − tiny: below the midpoint, the odd neighbour
    (1 + 3 * E23, 1.5, 2.0 ** -60, 1.5 + 5 * E23),      # 1.5 + 9·2^-24 + tiny: above the midpoint
    (-(1 + E23), 1.5, 2.0 ** -60, -(1.5 + E23)),        # the mirrored case
    (1 + 5 * E23, 1.5, -2.0 ** -100, 1.5 + 7 * E23),    # 1.5 + 15·2^-24 − tiny
]


def _nearest_f32(x):
    """The fp32 nearest to the Fraction x by search over the neighbours of float(x) (no tie occurs where this is used)."""
    near = F32(float(x))
    cands = [near, np.nextafter(near, F32(np.inf)), np.nextafter(near, F32(-np.inf))]
    return float(min(cands, key=lambda v: abs(Fraction(float(v)) - x)))


@pytest.mark.parametrize('a,b,c,want', TRIPLES)
def test_fmaf_is_exact_where_two_roundings_are_not(a, b, c, want):
    assert all(float(F32(v)) == v for v in (a, b, c, want))                                  # fp32 operands
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    assert _nearest_f32(exact) == want
    assert R.fmaf(a, b, c) == want
    assert float(R.fmaf_v(a, b, c)) == want
    naive = R.fmaf_twice_rounded(a, b, c)
    assert naive != want and abs(naive - want) == E23                                        # the other neighbour


def test_rounding_ties_subnormals_and_the_array_form():
    assert R.round_to_f32(3, -24 - 1) == 3 * 2.0 ** -25                                      # exact
    assert R.round_to_f32((1 << 24) + 1, 0) == float(1 << 24)                                # tie to even, down
    assert R.round_to_f32((1 << 24) + 3, 0) == float((1 << 24) + 4)                          # tie to even, up
    assert R.round_to_f32(3, -151) == 2.0 ** -149 and R.round_to_f32(1, -150) == 0.0         # subnormal quantum, ties to even
    assert R.round_to_f32(-5, -151) == -2.0 ** -149
    assert R.fmaf(2.0 ** -80, 2.0 ** -80, 0.0) == 0.0 and R.fmaf(3.0, 5.0, -15.0) == 0.0
    rng = np.random.default_rng(1)
    k = 4000
    a = (rng.random(3 * k) * 4 - 2).astype(F32)
    b = (rng.random(3 * k) * 4 - 2).astype(F32)
    c = np.concatenate([(rng.random(k) * 4 - 2).astype(F32),                                  # the same magnitude
                        ((rng.random(k) * 2 - 1) * 2.0 ** rng.integers(-70, -20, k)).astype(F32),  # far below the product
                        np.zeros(k, dtype=F32)])
    # products ON a midpoint, pushed off it either way: where the second rounding matters
    a = np.concatenate([a, F32(1) + (rng.integers(0, 1 << 20, k) * 2 + 1).astype(F32) * F32(E23)])
    b = np.concatenate([b, np.full(k, 1.5, dtype=F32)])
    c = np.concatenate([c, (rng.choice([-1.0, 1.0], k) * 2.0 ** rng.integers(-120, -55, k)).astype(F32)])
    got = R.fmaf_v(a, b, c)
    want = np.array([R.fmaf(x, y, w) for x, y, w in zip(a, b, c)], dtype=F32)
    assert np.array_equal(got, want)
    naive = np.array([R.fmaf_twice_rounded(x, y, w) for x, y, w in zip(a[-k:], b[-k:], c[-k:])], dtype=F32)
    assert (naive != want[-k:]).sum() > k // 4                                               # the family is a hard one
    for x, y, w, v in list(zip(a, b, c, want))[::97]:
        assert _nearest_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(w))) == float(v)


# ---- the ladder --------------------------------------------------------------------------------------------------------------
_LADDER = {}


def _ladder():
    """The full ladder, its slot arrays, operands at (H, C) = (3, 4) and the replica's forward and slot terms, computed once."""
    if not _LADDER:
        ei, n, targets, sources = R.ladder()
        heads, c = 3, 4
        vec, lph = R.instantiation(heads, c)
        z, a, b, d_out = R.operands(n, heads, c, seed=1)
        arrays = R.csr_arrays(ei, n)
        out, rec = R.forward(arrays[0], arrays[1], z, a, b, 0.2, lph)
        terms = R.slot_terms(arrays, z, a, b, out, rec, d_out, 0.2, vec, lph)
        _LADDER.update(ei=ei, n=n, targets=targets, sources=sources, heads=heads, c=c, vec=vec, lph=lph, z=z, a=a, b=b, d_out=d_out,
                       arrays=arrays, out=out, rec=rec, terms=terms)
    return _LADDER


def test_the_ladder_reaches_what_it_claims():
    L = _ladder()
    ei, n, arrays = L['ei'], L['n'], L['arrays']
    assert n <= 1500
    deg_in, deg_out = np.bincount(ei[1], minlength=n), np.bincount(ei[0], minlength=n)
    assert (np.diff(arrays[0]) == deg_in).all() and (np.diff(arrays[2]) == deg_out).all()    # add_self_loops=False: as written
    assert deg_in[L['targets']].tolist() == R.IN_LENGTHS and deg_out[L['sources']].tolist() == R.OUT_LENGTHS
    assert not set(L['targets']) & set(L['sources'])
    assert deg_out[L['targets']].max() == 0 and deg_in[L['sources']].max() == 0              # the ladder nodes hold nothing else
    have_in, have_out = set(R.IN_LENGTHS), set(R.OUT_LENGTHS)
    assert set(range(R.GAT_LONG + 2)) <= have_in and set(range(R.GAT_LONG + 2)) <= have_out
    assert {255, 256, 257, 511, 512, 513} <= have_in and {255, 256, 257, 511, 512, 513} <= have_out
    assert {127, 128, 129} <= have_in and R.IN_LENGTHS.count(2 * 512 + 1) == 1
    for lph in gat_ref.LPHS:
        gu = R.groups(lph) * R.in_flight(lph)
        if gu > R.GAT_LONG:
            assert {gu - 1, gu, gu + 1} <= have_in
        assert {0, 1, 2, 7, 8, 9, 95, 96, 97, gu - 1, gu, gu + 1} == set(R.reduced_lengths(lph))
        e2, n2, t2, s2 = R.reduced_ladder(lph)
        assert np.bincount(e2[1], minlength=n2)[t2].tolist() == R.reduced_lengths(lph)
        assert np.bincount(e2[0], minlength=n2)[s2].tolist() == R.reduced_lengths(lph)
    rowptr, col = arrays[0], arrays[1]
    dup = [i for i in L['targets'] if deg_in[i] > R.GAT_LONG and len(set(col[rowptr[i]:rowptr[i + 1]])) < deg_in[i]]
    assert dup                                                                               # a duplicated column in a long row
    # the slot arrays are the documented rule, and the model's own
    from models.gat import gat_csr
    csr = gat_csr(torch.from_numpy(ei), n, add_self_loops=False)
    for mine, theirs in zip(arrays, (csr.rowptr, csr.col, csr.rowptr_t, csr.col_t, csr.slot_t)):
        assert np.array_equal(mine, theirs.numpy().astype(np.int64))
    with_loops = R.csr_arrays(ei, n, True)
    csr = gat_csr(torch.from_numpy(ei), n, add_self_loops=True)
    for mine, theirs in zip(with_loops, (csr.rowptr, csr.col, csr.rowptr_t, csr.col_t, csr.slot_t)):
        assert np.array_equal(mine, theirs.numpy().astype(np.int64))
    # the small graph of the H = 64 shapes
    e3, n3, t3, s3 = R.small_graph()
    d_in, d_out = np.bincount(e3[1], minlength=n3), np.bincount(e3[0], minlength=n3)
    assert n3 <= 250 and {96, 97} <= set(d_in[t3]) and 97 in set(d_out[s3]) and d_in[-1] == 100 and d_out[-1] == 100
    assert n3 % 4 and (n3 * 3) % 64                                                           # idle groups next to the long last row


def test_the_replica_is_a_valid_fp32_evaluation():
    """Within the derived bounds of the fp64 restatement on the ladder: O and the three gradients."""
    L = _ladder()
    z, d_out = torch.from_numpy(L['z']), torch.from_numpy(L['d_out'])
    s_src = torch.from_numpy(np.tile(L['a'], (L['n'], 1)))
    s_dst = torch.from_numpy(np.tile(L['b'], (L['n'], 1)))
    cnt = gat_ref.count_matrix(L['ei'], L['n'], False)
    want = gat_ref.aggregate_reference(z, s_src, s_dst, cnt, d_out)
    bound = gat_ref.bounds(z, s_src, s_dst, cnt, d_out)
    grads = R.backward(L['arrays'], L['z'], L['a'], L['b'], L['out'], L['rec'], L['d_out'], 0.2, L['vec'], L['lph'], terms=L['terms'])
    ratios = {}
    for key, got, w in zip(('O', 'dZ', 'dS_src', 'dS_dst'), (L['out'],) + grads, want):
        ratios[key] = gat_ref.worst_ratio(torch.from_numpy(got), w, bound[key])
    print('order replica against the fp64 restatement, largest error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    assert all(0 < v <= 1.0 for v in ratios.values()), ratios
    counts = np.diff(L['arrays'][0])
    rec = L['rec'].reshape(L['n'], L['heads'], 2)
    assert np.array_equal(rec[:, 0, 1], np.maximum(counts, 1).astype(F32))
    _, e = R.head_scores(L['a'], L['b'], 0.2)
    assert e[0] > 0 > e[1] and e[2] == 0 and np.array_equal(rec[counts > 0, :, 0], np.tile(e, (int((counts > 0).sum()), 1)))


def test_another_order_would_show():
    """A condition on the operands: every long row of either CSR gives other bits as a plain chain, with the G of another LPH and
    with its groups added in reverse; a short row with its slots in reverse."""
    L = _ladder()
    arrays, z, a, b, d_out = L['arrays'], L['z'], L['a'], L['b'], L['d_out']
    long_in = [i for i in range(L['n']) if arrays[0][i + 1] - arrays[0][i] > R.GAT_LONG]
    long_out = [j for j in range(L['n']) if arrays[2][j + 1] - arrays[2][j] > R.GAT_LONG]
    assert len(long_in) == len([k for k in R.IN_LENGTHS if k > R.GAT_LONG]) and len(long_out) == len([k for k in R.OUT_LENGTHS if k > R.GAT_LONG])
    for lph in gat_ref.LPHS:
        others = [R.plan_chain, R.plan_groups_reversed] + [R.plan_other_groups(R.groups(o)) for o in gat_ref.LPHS if o != lph]
        base_o, _ = R.forward(arrays[0], arrays[1], z, a, b, 0.2, lph, rows=long_in)
        base_dz, base_src, _ = R.backward(arrays, z, a, b, L['out'], L['rec'], d_out, 0.2, L['vec'], lph, rows_t=long_out, terms=L['terms'])
        for plan in others:
            o, _ = R.forward(arrays[0], arrays[1], z, a, b, 0.2, lph, plan=plan, rows=long_in)
            dz, _, _ = R.backward(arrays, z, a, b, L['out'], L['rec'], d_out, 0.2, L['vec'], lph, plan=plan, rows_t=long_out, terms=L['terms'])
            assert all((o[i] != base_o[i]).any() for i in long_in), lph
            assert all((dz[j] != base_dz[j]).any() for j in long_out), lph
    short_in = [int(L['targets'][k]) for k in (8, 31, R.GAT_LONG)]
    short_out = [int(L['sources'][k]) for k in (8, 31, R.GAT_LONG)]
    base_o, _ = R.forward(arrays[0], arrays[1], z, a, b, 0.2, 4, rows=short_in)
    o, _ = R.forward(arrays[0], arrays[1], z, a, b, 0.2, 4, plan=R.plan_slots_reversed, rows=short_in)
    base_dz, _, _ = R.backward(arrays, z, a, b, L['out'], L['rec'], d_out, 0.2, L['vec'], 4, rows_t=short_out, terms=L['terms'])
    dz, _, _ = R.backward(arrays, z, a, b, L['out'], L['rec'], d_out, 0.2, L['vec'], 4, plan=R.plan_slots_reversed, rows_t=short_out, terms=L['terms'])
    assert all((o[i] != base_o[i]).any() for i in short_in) and all((dz[j] != base_dz[j]).any() for j in short_out)


def test_the_shapes_reach_the_instantiations_they_are_named_for():
    assert [R.instantiation(*s) for s in R.ORDER_SHAPES] == R.ORDER_INSTANTIATIONS
    assert {l for _, l in R.ORDER_INSTANTIATIONS} == set(gat_ref.LPHS)
    assert [R.instantiation(*s) for s in R.BACKWARD_SHAPES] == R.BACKWARD_INSTANTIATIONS
    assert [l for _, l in R.BACKWARD_INSTANTIATIONS] == list(gat_ref.LPHS)
    assert [R.instantiation(*s) for s in R.CAP_SHAPES] == R.CAP_INSTANTIATIONS
    assert R.instantiation(64, 4) == (4, 4) and R.instantiation(64, 8) == (4, 4) and R.instantiation(5, 6) == (2, 4)
    # the width ladder of the forward's independence check, and what has to be refused
    assert [gat_ref.vec_lph(c, (c,), (0,)) for c in (4, 16, 64, 132, 256)] == [(4, 4), (4, 4), (4, 16), (4, 64), (4, 64)]
    assert gat_ref.vec_lph(4, (4,), (4,)) == (1, 4) and gat_ref.vec_lph(16, (16,), (4,)) == (1, 16)
    assert gat_ref.vec_lph(256, (258,), (0,)) is None and gat_ref.vec_lph(128, (129,), (0,)) is None and gat_ref.vec_lph(128, (128,), (4,)) is None
    reach = {gat_ref.vec_lph(c, (h * c,)) for h, c in gat_ref.EXACT_SHAPES}
    assert reach == {(v, l) for v in (1, 2, 4) for l in gat_ref.LPHS}                         # all fifteen, still
