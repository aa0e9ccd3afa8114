"""The attention kernels (csrc/dcr_gat.hip) at their limits, through the raw ABI: the order of every sum bit for bit against the
host replica of tests/gat_order_ref.py (unit weights), the kernel against its own other routes bit for bit at random weights
(one head alone, permuted heads, a head's first channels alone, a padded graph), the caps of H and C, the slope's edge values,
the backward through underflowed weights and the wrapper's unpacked branch.  Every check is bit equality, the derived bounds of
tests/gat_ref.py (error / bound <= 1) or EINVAL; no tolerance of its own.  ASSUMED, as in gat_ref and gat_order_ref: expf(0) is
exactly 1 and expf is within 2 ulp.  Every raw call writes into NaN-filled buffers and no NaN may be left."""
import numpy as np
import pytest
import torch

import gat_order_ref as R
import gat_ref
from test_gat_gpu import EINVAL, GAT_LONG, NAN, _stream, _view, both, expand, gather, lib  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

KEYS = ('O', 'dZ', 'dS_src', 'dS_dst')
_CACHE = {}


def _graph(name):
    """(edge_index tensor, n, AttnCSR on the GPU, count matrix, targets, sources) of a fixture of gat_order_ref, built once."""
    if name not in _CACHE:
        from models.gat import gat_csr
        make = {'ladder': R.ladder, 'small': R.small_graph}.get(name) or (lambda: R.reduced_ladder(name))
        ei, n, targets, sources = make()
        ei = torch.from_numpy(ei)
        _CACHE[name] = (ei, n, gat_csr(ei.cuda(), n, add_self_loops=False), gat_ref.count_matrix(ei, n, False), targets, sources)
    return _CACHE[name]


def _random(n, heads, c, seed, scale=2.0):
    """(z, s_src, s_dst, d_out) fp32 on the CPU: Z and dO in ±1, scores in ±scale."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g) * 2 - 1
    return u(n, heads * c), u(n, heads) * scale, u(n, heads) * scale, u(n, heads * c)


def _run(lib, csr, z, s_src, s_dst, d_out, slope=0.2, off=0, ld_pad=0):
    """(O, rec, dZ, dS_src, dS_dst) and the device operands (Z, s_src, s_dst); Z and O ``off`` floats past a 16-byte boundary."""
    w = z.shape[1]
    zc, sc, dc = _view(z, w + ld_pad, off), _view(s_src), _view(s_dst)
    out, rec = gather(lib, csr, zc, sc, dc, slope, ldo=w + ld_pad, off_o=off)
    return (out, rec) + expand(lib, csr, zc, sc, dc, out, rec, d_out, slope), (zc, sc, dc)


def _within_bounds(what, got, z, s_src, s_dst, cnt, d_out, slope=0.2):
    want = gat_ref.aggregate_reference(z, s_src, s_dst, cnt, d_out, slope)
    bound = gat_ref.bounds(z, s_src, s_dst, cnt, d_out, slope)
    ratios = {key: gat_ref.worst_ratio(g.cpu(), w, bound[key]) for key, g, w in zip(KEYS, got, want)}
    print(f'GAT limits, {what}: largest error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    for key, ratio in ratios.items():
        assert ratio <= 1.0, (what, key, ratio)


def _unit(n, a, b):
    return torch.from_numpy(np.tile(a, (n, 1))), torch.from_numpy(np.tile(b, (n, 1)))


# ---- a. the order, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('heads,c,off', R.ORDER_SHAPES)
def test_forward_order_on_the_ladder(lib, heads, c, off):
    """Unit weights (constant scores: a head each of pre > 0, < 0, = 0), random float Z: O is the replica's bits on every row of
    the ladder (every length 0 .. 97, G·U ± 1, 1025), and rec = (e, count)."""
    ei, n, csr, _, _, _ = _graph('ladder')
    vec, lph = R.instantiation(heads, c, off)
    z, a, b, _ = R.operands(n, heads, c, seed=100 + c)
    s_src, s_dst = _unit(n, a, b)
    arrays = R.csr_arrays(ei.numpy(), n)
    want, want_rec = R.forward(arrays[0], arrays[1], z, a, b, 0.2, lph)
    out, rec = gather(lib, csr, _view(torch.from_numpy(z), None, off), _view(s_src), _view(s_dst), ldo=None, off_o=off)
    assert torch.equal(rec.cpu()[:n * heads], torch.from_numpy(want_rec))
    assert torch.equal(out.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize('heads,c', R.BACKWARD_SHAPES)
def test_backward_order_on_the_reduced_ladder(lib, heads, c):
    """The same inputs through rowdot, expand and the closing sum: dZ, dS_src and dS_dst are the replica's bits (fmaf chains and
    butterflies of the dots, the strided order of long rows of the transposed pattern, G = 64 in the closing sum)."""
    vec, lph = R.instantiation(heads, c)
    ei, n, csr, _, _, _ = _graph(lph)
    z, a, b, d_out = R.operands(n, heads, c, seed=200 + c)
    s_src, s_dst = _unit(n, a, b)
    arrays = R.csr_arrays(ei.numpy(), n)
    want, want_rec = R.forward(arrays[0], arrays[1], z, a, b, 0.2, lph)
    (out, rec, dz, ds_src, ds_dst), _ = _run(lib, csr, torch.from_numpy(z), s_src, s_dst, torch.from_numpy(d_out))
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and torch.equal(rec.cpu()[:n * heads], torch.from_numpy(want_rec))
    w_dz, w_src, w_dst = R.backward(arrays, z, a, b, want, want_rec, d_out, 0.2, vec, lph)
    assert torch.equal(dz.cpu(), torch.from_numpy(w_dz))
    assert torch.equal(ds_src.cpu(), torch.from_numpy(w_src))
    assert torch.equal(ds_dst.cpu(), torch.from_numpy(w_dst))


# ---- b. non-unit weights: the kernel against its own other routes ------------------------------------------------------------
@pytest.mark.parametrize('c,picked', [(4, (0, 1, 31, 63)), (8, (0, 63))])
def test_a_head_of_64_alone_gives_the_same_bits(lib, c, picked):
    """H = 64 on the ladder against H = 1 calls on strided views of the same buffers (ldz = ldo = 64·C, lds = 64, the pointers
    h·C and h floats in): O, rec and the three gradients of that head.  The H = 64 shape within bounds on the small graph."""
    heads = 64
    ei, n, csr, _, _, _ = _graph('ladder')
    z, s_src, s_dst, d_out = _random(n, heads, c, seed=300 + c)
    (out, rec, dz, ds_src, ds_dst), (zc, sc, dc) = _run(lib, csr, z, s_src, s_dst, d_out)
    for h in picked:
        cols = slice(h * c, (h + 1) * c)
        z1, s1, d1 = zc[:, cols], sc[:, h:h + 1], dc[:, h:h + 1]
        assert z1.stride(0) == heads * c and s1.stride(0) == heads and z1.data_ptr() == zc.data_ptr() + 4 * h * c
        o1, r1 = gather(lib, csr, z1, s1, d1, ldo=heads * c, off_o=h * c)
        g1 = expand(lib, csr, z1, s1, d1, o1, r1, d_out[:, cols])
        assert torch.equal(o1, out[:, cols]) and torch.equal(r1[:n], rec[:n * heads].view(n, heads, 2)[:, h])
        assert torch.equal(g1[0], dz[:, cols]) and torch.equal(g1[1], ds_src[:, h:h + 1]) and torch.equal(g1[2], ds_dst[:, h:h + 1])
    ei, n, csr, cnt, _, _ = _graph('small')
    z, s_src, s_dst, d_out = _random(n, heads, c, seed=310 + c)
    (out, _, dz, ds_src, ds_dst), _ = _run(lib, csr, z, s_src, s_dst, d_out)
    _within_bounds(f'H x C = 64 x {c}, small graph', (out, dz, ds_src, ds_dst), z, s_src, s_dst, cnt, d_out)


def test_permuted_heads_give_permuted_bits(lib):
    heads, c = 5, 6
    ei, n, csr, cnt, _, _ = _graph('ladder')
    z, s_src, s_dst, d_out = _random(n, heads, c, seed=320)
    (out, rec, dz, ds_src, ds_dst), _ = _run(lib, csr, z, s_src, s_dst, d_out)
    _within_bounds('H x C = 5 x 6, ladder', (out, dz, ds_src, ds_dst), z, s_src, s_dst, cnt, d_out)
    perm = torch.tensor([3, 0, 4, 1, 2])
    blocks = lambda t: t.reshape(n, heads, -1)[:, perm.to(t.device)].reshape(n, -1)
    (p_out, p_rec, p_dz, p_src, p_dst), _ = _run(lib, csr, blocks(z), blocks(s_src), blocks(s_dst), blocks(d_out))
    assert torch.equal(p_out, blocks(out)) and torch.equal(p_dz, blocks(dz))
    assert torch.equal(p_src, blocks(ds_src)) and torch.equal(p_dst, blocks(ds_dst))
    assert torch.equal(p_rec[:n * heads], rec[:n * heads].view(n, heads, 2)[:, perm.cuda()].reshape(n * heads, 2))


@pytest.mark.parametrize('c,off', [(4, 1), (16, 0), (64, 0), (132, 0), (256, 0)])
def test_the_first_channels_of_a_head_alone(lib, c, off):
    """Two heads' first 4 channels alone (C = 4, VEC 4, LPH 4) against the same heads at width C (or at C = 4 on operands 4 bytes
    off a 16-byte boundary: VEC 1): short rows of O and their records are the same bits in every instantiation; where LPH is the
    same, long rows too, and dZ."""
    heads, narrow = 2, 4
    ei, n, csr, cnt, _, _ = _graph('ladder')
    z, s_src, s_dst, d_out = _random(n, heads, c, seed=330 + c)
    first = lambda t: t.reshape(n, heads, c)[:, :, :narrow].reshape(n, heads * narrow)
    (w_out, w_rec, w_dz, w_src, w_dst), _ = _run(lib, csr, z, s_src, s_dst, d_out, off=off)
    _within_bounds(f'H x C = 2 x {c}, offset {4 * off} bytes, ladder', (w_out, w_dz, w_src, w_dst), z, s_src, s_dst, cnt, d_out)
    (n_out, n_rec, n_dz, _, _), _ = _run(lib, csr, first(z).contiguous(), s_src, s_dst, first(d_out).contiguous())
    lph = R.instantiation(heads, c, off)[1]
    rows = torch.ones(n, dtype=torch.bool) if lph == 4 else (csr.rowptr[1:] - csr.rowptr[:-1] <= GAT_LONG).cpu()
    assert int((~rows).sum()) == (0 if lph == 4 else len([k for k in R.IN_LENGTHS if k > GAT_LONG]))
    assert torch.equal(first(w_out).cpu()[rows], n_out.cpu()[rows])
    assert torch.equal(w_rec[:n * heads].view(n, heads, 2).cpu()[rows], n_rec[:n * heads].view(n, heads, 2).cpu()[rows])
    if lph == 4:
        assert torch.equal(first(w_dz), n_dz)


@pytest.mark.parametrize('heads,c', [(3, 8), (2, 33)])
def test_isolated_nodes_appended_change_no_bit(lib, heads, c):
    """700 more nodes without a slot: another gridDim and another deal of units to workgroups.  The rows that were there keep
    their bits in all four outputs; the new ones give exact zeros and rec = (0, 1)."""
    from models.gat import gat_csr
    ei, n, csr, cnt, _, _ = _graph('ladder')
    z, s_src, s_dst, d_out = _random(n, heads, c, seed=340 + c)
    (out, rec, dz, ds_src, ds_dst), _ = _run(lib, csr, z, s_src, s_dst, d_out)
    _within_bounds(f'H x C = {heads} x {c}, ladder', (out, dz, ds_src, ds_dst), z, s_src, s_dst, cnt, d_out)
    more = 700
    extra = _random(more, heads, c, seed=350)
    wide = [torch.cat([t, x]) for t, x in zip((z, s_src, s_dst, d_out), extra)]
    (p_out, p_rec, p_dz, p_src, p_dst), _ = _run(lib, gat_csr(ei.cuda(), n + more, add_self_loops=False), *wide)
    for got, want in ((p_out, out), (p_dz, dz), (p_src, ds_src), (p_dst, ds_dst)):
        assert torch.equal(got[:n], want) and float(got[n:].abs().max()) == 0.0
    assert torch.equal(p_rec[:n * heads], rec[:n * heads])
    assert torch.equal(p_rec[n * heads:(n + more) * heads].cpu(), torch.tensor([0.0, 1.0]).repeat(more * heads, 1))


# ---- c. the caps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('heads,c,off', R.CAP_SHAPES + [(3, 4, 0)])
def test_heads_and_widths_at_their_caps(lib, heads, c, off):
    """H = 64 and C = 256, C = 128 at VEC 2 and C = 64 at VEC 1 (LPH 64) on the small graph: the exact quotients at unit weights
    and integer operands, random floats within the bounds.  The graph's LAST row is long and n·H is no multiple of G at LPH 64
    (1 and 2 heads of 256) and at LPH 4 (3 heads of 4): the idle groups of the last workgroup park with it and leave."""
    ei, n, csr, cnt, _, _ = _graph('small')
    lph = R.instantiation(heads, c, off)[1]
    if (heads, c) in ((1, 256), (2, 256), (3, 4)):
        assert (n * heads) % R.groups(lph) and cnt.sum(1)[-1] > GAT_LONG and cnt.sum(0)[-1] > GAT_LONG
    g = torch.Generator().manual_seed(400 + heads * c)
    z = torch.randint(-8, 9, (n, heads * c), generator=g).float()
    d_out = torch.randint(-4, 5, (n, heads * c), generator=g).float()
    zero = torch.zeros(n, heads)
    (out, rec, dz, ds_src, ds_dst), _ = _run(lib, csr, z, zero, zero, d_out, off=off)
    d = cnt.sum(1)
    want = (cnt @ z.double()).float() / d.clamp(min=1).float()[:, None]                 # exact integers, one fp32 division
    assert torch.equal(out.cpu(), want)
    assert torch.equal(rec[:n * heads].view(n, heads, 2).cpu()[:, :, 1], d.clamp(min=1).float()[:, None].expand(n, heads))
    _within_bounds(f'H x C = {heads} x {c}, unit weights', (out, dz, ds_src, ds_dst), z, zero, zero, cnt, d_out)
    z, s_src, s_dst, d_out = _random(n, heads, c, seed=410 + heads * c)
    (out, _, dz, ds_src, ds_dst), _ = _run(lib, csr, z, s_src, s_dst, d_out, off=off)
    _within_bounds(f'H x C = {heads} x {c}, offset {4 * off} bytes, small graph', (out, dz, ds_src, ds_dst), z, s_src, s_dst, cnt, d_out)


def test_128_pieces_are_refused_before_any_launch(lib):
    """C = 256 at VEC 2 and C = 128 at VEC 1 would need 128 lanes a head: EINVAL from both entry points, nothing written."""
    from models.gat import gat_csr
    n = 6
    ring = torch.arange(n)
    csr = gat_csr(torch.stack([ring, (ring + 1) % n]).cuda(), n)
    nan = lambda count: torch.full((count,), NAN, device='cuda')
    z, out, d_out, dz = (nan(n * 260 + 64) for _ in range(4))
    s, rec, ds, w4, wg = nan(n), nan(2 * n), nan(n), nan(4 * n), nan(2 * n)
    for c, ld, off in ((256, 258, 0), (128, 129, 0), (128, 128, 4)):
        assert gat_ref.vec_lph(c, (ld,), (off,)) is None
        rc = lib.dcr_gat_gather_f32_dev(csr.rowptr.data_ptr(), csr.col.data_ptr(), z.data_ptr() + off, s.data_ptr(), s.data_ptr(),
                                        out.data_ptr(), rec.data_ptr(), n, 1, c, ld, 1, ld, 0.2, _stream())
        assert rc == EINVAL, (c, ld, off)
        rc = lib.dcr_gat_expand_f32_dev(csr.rowptr.data_ptr(), csr.rowptr_t.data_ptr(), csr.col_t.data_ptr(), csr.slot_t.data_ptr(),
                                        z.data_ptr() + off, s.data_ptr(), s.data_ptr(), out.data_ptr(), d_out.data_ptr(), rec.data_ptr(),
                                        dz.data_ptr(), ds.data_ptr(), ds.data_ptr(), w4.data_ptr(), wg.data_ptr(), n, 1, c, ld, 1, ld,
                                        0.2, _stream())
        assert rc == EINVAL, (c, ld, off)
        assert b'GAT' in lib.dcr_last_error()
    torch.cuda.synchronize()
    for t in (out, rec, dz, ds, w4, wg):
        assert bool(torch.isnan(t).all())


# ---- d. the slope ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['powerlaw', 'hub'])
@pytest.mark.parametrize('slope', [0.0, 1.0, 0.01, 0.5])
def test_slopes_within_the_bounds(lib, slope, name):
    ei, n, heads, c, loops, z, s_src, s_dst, d_out = gat_ref.fixture(name)
    cnt = gat_ref.count_matrix(ei, n, loops)
    got = both(lib, ei, n, loops, z, s_src, s_dst, d_out, slope)
    _within_bounds(f'slope {slope}, fixture {name!r}', got, z, s_src, s_dst, cnt, d_out, slope)


def _dyadic_scores(n, heads, seed):
    """Scores on the grid 2^-10 in ±2: every pre, and every pre + 8, is exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(-2048, 2049, (n, heads), generator=g).float() / 1024 for _ in range(2))


@pytest.mark.parametrize('slope', [0.0, 1.0, 0.5])
def test_zero_and_negative_zero_take_the_slope_arm(lib, slope):
    """Some pre are exactly 0.0 (x + (−x)) and some exactly −0.0 ((−0.0) + (−0.0)): the kernels' ``pre > 0`` sends both to the
    slope arm, as the restatement's does; a gradient through the other arm would be off by (1 − slope)·g."""
    ei, n, csr, cnt, _, _ = _graph('small')
    heads, c = 2, 8
    z, _, _, d_out = _random(n, heads, c, seed=500)
    g = torch.Generator().manual_seed(501)
    levels = torch.tensor([-0.0, 0.5, -0.5, 1.0])
    s_src = levels[torch.randint(0, 4, (n, heads), generator=g)]
    s_dst = -levels[torch.randint(0, 4, (n, heads), generator=g)]
    s_dst = torch.where(s_dst == 0, torch.tensor(-0.0), s_dst)                             # (−(−0.0) = +0.0: put the sign back)
    src, tgt = ei[0], ei[1]
    pre = s_src[src] + s_dst[tgt]
    assert int(((pre == 0) & ~torch.signbit(pre)).sum()) > 20 and int(((pre == 0) & torch.signbit(pre)).sum()) > 20
    assert int((pre > 0).sum()) > 100 and int((pre < 0).sum()) > 100
    (out, _, dz, ds_src, ds_dst), _ = _run(lib, csr, z, s_src, s_dst, d_out, slope)
    _within_bounds(f'slope {slope}, pre = +0.0 and -0.0', (out, dz, ds_src, ds_dst), z, s_src, s_dst, cnt, d_out, slope)


def test_slope_one_is_the_identity_on_both_arms(lib):
    """At slope 1 the slope arm is 1·pre = pre.  With scores on a dyadic grid, s_dst + 8 moves every pre above 0 (the other arm)
    and every e − m stays the same number: O, den and all three gradients are the same bits, m is 8 larger.  (The issue's
    negated variant changes the weights; the shift alone is what can be built exactly.)"""
    ei, n, csr, cnt, _, _ = _graph('small')
    heads, c = 3, 6
    z, _, _, d_out = _random(n, heads, c, seed=510)
    s_src, s_dst = _dyadic_scores(n, heads, seed=511)
    pre = s_src[ei[0]] + s_dst[ei[1]]
    assert int((pre < 0).sum()) > 100 and float((pre + 8).min()) > 0
    (out, rec, dz, ds_src, ds_dst), _ = _run(lib, csr, z, s_src, s_dst, d_out, 1.0)
    _within_bounds('slope 1.0, dyadic scores', (out, dz, ds_src, ds_dst), z, s_src, s_dst, cnt, d_out, 1.0)
    (p_out, p_rec, p_dz, p_src, p_dst), _ = _run(lib, csr, z, s_src, s_dst + 8, d_out, 1.0)
    for got, want in ((p_out, out), (p_dz, dz), (p_src, ds_src), (p_dst, ds_dst)):
        assert torch.equal(got, want)
    rec, p_rec = rec[:n * heads].cpu(), p_rec[:n * heads].cpu()
    some = (cnt.sum(1) > 0).repeat_interleave(heads)
    assert torch.equal(p_rec[:, 1], rec[:, 1]) and torch.equal(p_rec[some, 0], rec[some, 0] + 8)


# ---- e. the backward through underflowed weights -----------------------------------------------------------------------------
@pytest.mark.parametrize('heads,c', [(1, 4), (3, 6), (8, 8), (2, 64)])
def test_backward_through_underflowed_weights(lib, heads, c):
    """The graph of test_one_dominant_slot_and_the_subtracted_maximum (150 targets, one of 130 slots; one source of every row
    leads by 120): the others' weights are exactly 0 in fp32, the leader's α exactly 1.  So dZ and dS_src of every source that
    leads nowhere are exactly 0.0, and dZ of a leader is the dO row of its target, bit for bit.

    The bounds: gat_ref's are RELATIVE to α and do not hold an underflow term, so where the restatement's α is about e^-120 they
    are about 1e-56 and cannot admit the exact 0.0 asserted above.  On those elements the check is that the restatement's value
    is below fp32's smallest subnormal (0.0 is then its correctly rounded fp32 value); everywhere else, error / bound <= 1."""
    from models.gat import gat_csr
    n_t, per = 150, 7
    lead = torch.arange(n_t) + n_t
    rows, srcs = [], []
    for i in range(n_t):
        k = 129 if i == 7 else per
        others = 300 + (i + torch.arange(k)) % 150
        at = i % (k + 1)
        srcs.append(torch.cat([others[:at], lead[i:i + 1], others[at:]]))
        rows.append(torch.full((k + 1,), i))
    ei = torch.stack([torch.cat(srcs), torch.cat(rows)])
    n = 450
    g = torch.Generator().manual_seed(600 + c)
    z = torch.randn(n, heads * c, generator=g)
    d_out = torch.rand(n, heads * c, generator=g) * 2 - 1
    s_src = torch.zeros(n, heads)
    s_src[n_t:2 * n_t] = 120.0
    s_dst = torch.zeros(n, heads)
    cnt = gat_ref.count_matrix(ei, n, False)
    assert float(cnt.sum(1).max()) == 130 and float(cnt.sum(0)[300:].min()) >= 1
    (out, rec, dz, ds_src, ds_dst), _ = _run(lib, gat_csr(ei.cuda(), n, add_self_loops=False), z, s_src, s_dst, d_out)
    assert torch.equal(out.cpu()[:n_t], z[lead])
    assert torch.equal(rec[:n_t * heads].cpu(), torch.tensor([120.0, 1.0]).repeat(n_t * heads, 1))      # α of a leader: 1 / 1
    dz, ds_src, ds_dst = dz.cpu(), ds_src.cpu(), ds_dst.cpu()
    nowhere = torch.ones(n, dtype=torch.bool)
    nowhere[lead] = False
    assert float(dz[nowhere].abs().max()) == 0.0 and float(ds_src[nowhere].abs().max()) == 0.0
    assert torch.equal(dz[lead], d_out[:n_t])
    want = gat_ref.aggregate_reference(z, s_src, s_dst, cnt, d_out)
    bound = gat_ref.bounds(z, s_src, s_dst, cnt, d_out)
    tiny = 2.0 ** -149
    assert float(want[1][nowhere].abs().max()) < tiny and float(want[2][nowhere].abs().max()) < tiny
    keep = ~nowhere
    ratios = {'O': gat_ref.worst_ratio(out.cpu(), want[0], bound['O']),
              'dZ': gat_ref.worst_ratio(dz[keep], want[1][keep], bound['dZ'][keep]),
              'dS_src': gat_ref.worst_ratio(ds_src[keep], want[2][keep], bound['dS_src'][keep]),
              'dS_dst': gat_ref.worst_ratio(ds_dst, want[3], bound['dS_dst'])}
    print(f'GAT limits, dominant slot H x C = {heads} x {c}: largest error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    for key, ratio in ratios.items():
        assert ratio <= 1.0, (key, ratio)


# ---- f. the wrapper's unpacked branch ----------------------------------------------------------------------------------------
def _through_wrapper(csr, z, s_src, s_dst, leaves, d_out):
    from models.gat import gat_aggregate
    out = gat_aggregate(z, s_src, s_dst, csr)
    out.backward(d_out.cuda())
    torch.cuda.synchronize()
    return out.detach(), [t.grad for t in leaves]


def test_the_unpacked_branch_of_the_wrapper(lib):
    """gat_aggregate on the HIP backend with three separate tensors, with scores of different row strides and with a column-major
    Z: the bits of the raw call on contiguous copies, forward and backward.  The packed layout of GATConv (one buffer of
    ld = H·C + 2·H + pad) gives the same O and dZ bits and its dS_* within the bounds."""
    from models import gcn
    assert gcn._AGG_BACKEND == 'hip'
    ei, n, csr, cnt, _, _ = _graph('small')
    heads, c = 3, 5
    z, s_src, s_dst, d_out = _random(n, heads, c, seed=700)
    (out, _, dz, ds_src, ds_dst), _ = _run(lib, csr, z, s_src, s_dst, d_out)
    _within_bounds('H x C = 3 x 5, small graph', (out, dz, ds_src, ds_dst), z, s_src, s_dst, cnt, d_out)
    raw = (out, dz, ds_src, ds_dst)

    def same(o, grads):
        for got, want in zip([o] + grads, raw):
            assert got.shape == want.shape and torch.equal(got, want)

    leaves = [t.clone().cuda().requires_grad_(True) for t in (z, s_src, s_dst)]              # three allocations
    same(*_through_wrapper(csr, *leaves, leaves, d_out))
    wide = torch.full((n, heads + 3), NAN, device='cuda')                                    # s_src strided, s_dst not
    wide[:, :heads] = s_src.cuda()
    wide.requires_grad_(True)
    leaves = [z.clone().cuda().requires_grad_(True), wide, s_dst.clone().cuda().requires_grad_(True)]
    o, grads = _through_wrapper(csr, leaves[0], wide[:, :heads], leaves[2], leaves, d_out)
    assert float(grads[1][:, heads:].abs().max()) == 0.0
    same(o, [grads[0], grads[1][:, :heads], grads[2]])
    z_t = z.t().contiguous().cuda().requires_grad_(True)                                     # column-major Z
    leaves = [z_t, s_src.clone().cuda().requires_grad_(True), s_dst.clone().cuda().requires_grad_(True)]
    assert z_t.t().stride() == (1, n)
    o, grads = _through_wrapper(csr, z_t.t(), leaves[1], leaves[2], leaves, d_out)
    same(o, [grads[0].t(), grads[1], grads[2]])
    # the packed layout
    from models.gat import _packed
    w = heads * c
    ld = w + 2 * heads + (-(w + 2 * heads) % 4)
    buf = torch.zeros(n, ld)
    buf[:, :w], buf[:, w:w + heads], buf[:, w + heads:w + 2 * heads] = z, s_src, s_dst
    buf = buf.cuda().requires_grad_(True)
    parts = (buf[:, :w], buf[:, w:w + heads], buf[:, w + heads:w + 2 * heads])
    assert ld == 24 and _packed(*parts) is not None and _packed(*[t.clone().cuda() for t in (z, s_src, s_dst)]) is None
    o, grads = _through_wrapper(csr, *parts, [buf], d_out)
    grad = grads[0]
    assert torch.equal(o, out) and torch.equal(grad[:, :w], dz) and float(grad[:, w + 2 * heads:].abs().max()) == 0.0
    _within_bounds('H x C = 3 x 5, packed layout', (o, grad[:, :w], grad[:, w:w + heads], grad[:, w + heads:w + 2 * heads]),
                   z, s_src, s_dst, cnt, d_out)
