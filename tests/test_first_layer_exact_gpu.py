"""csrc/dcr_gcn_first.hip through the raw C ABI (``dcr_first_layer_fwd_ws_f32_dev``, ``dcr_first_layer_bwd_f32_dev`` and their
workspace calls, include/dcr.h) with a tolerance of ZERO: the persistent MFMA forward with W1 in LDS, the K-chunked forward whose
last workgroup adds the chunks' tiles, and the backward that double-buffers its operands through LDS.

The operands are small integers (tests/first_layer_ref.py), so every fp32 partial sum is exact and pre, z_train, z_eval, db1, dW2
and dW1 must EQUAL the int64 results in any order of summation.  tests/test_first_layer_ref_cpu.py shows that a dropped 16-row
unit, a K chunk added twice or skipped, a stage multiplying the previous stage's rows, a keep bit one column on, a pad column in
dW1 or b1 added per chunk would each break that equality, and runs the exactness guard for every shape used here.

Protocol of every case: Â·X is [n + 16, F16 + 8] with the columns feats … F16 zero and NaN in the columns beyond and in the 16 rows
past n; dz and pre carry 16 NaN rows past n; every output and workspace starts filled with one NaN bit pattern (the K-chunked
kernel's tickets zero, as its contract asks), z is [n, 2·classes + 6], the workspaces and the backward's packed outputs carry 64
guard floats.  After the call every live entry equals the integer reference, every padding column, row past n and guard float
still holds the pattern, and a second call into the dirty workspace gives the same bits (the tickets zero again).  The forward's
mask is the ``bits`` the kernel wrote, which must be the host Philox decisions AND (pre > 0) on the integer pre; the backward's is
made on the host, independent of the sign of pre.

The plan a case is meant to reach — K chunks, row groups per workgroup, units per wave, stages per workgroup — is read from the
device (CU count) and the ABI (workspace sizes), asserted, and named in the case's id or label."""
import ctypes

import numpy as np
import pytest
import torch

import dropout_ref
import first_layer_ref as fr

pytestmark = pytest.mark.gpu

SEED, OFFSET = 0x123456789ABCDEF0, 7


def L():
    from dcr import _lib
    return _lib.lib()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_equal(got, want_int, label, name):
    """``got`` (fp32, device) equals the int64 reference entry by entry; the first difference goes into the message."""
    want = torch.from_numpy(np.ascontiguousarray(want_int)).to(torch.float32).cuda().reshape(got.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        at = tuple(bad[0].tolist())
        raise AssertionError((label, name, 'entries that differ', len(bad), 'of', got.numel(), 'first', at, 'got', got[at].item(),
                              'want', want[at].item()))


def untouched(t, label, name):
    assert fr.same_bits(t, fr.SENTINEL), (label, name, 'was written')


# ---- forward -------------------------------------------------------------------------------------------------------------------
def fwd_workspace(n, feats, hidden):
    need = ctypes.c_int64(-1)
    assert L().dcr_first_layer_fwd_workspace(n, feats, hidden, ctypes.byref(need)) == 0
    return need.value


def fwd_call(ax, ldx, w1, b1, w2, pre, z, classes, ldz, bits, n, feats, hidden, p, ws, ws_floats):
    return L().dcr_first_layer_fwd_ws_f32_dev(ax.data_ptr(), ldx, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), pre.data_ptr(), z.data_ptr(),
                                              z.data_ptr() + 4 * classes, ldz, bits.data_ptr(), None, n, feats, hidden, classes, p, SEED,
                                              OFFSET, None, ws.data_ptr(), ws_floats, st())


class Forward:
    """The device buffers of one forward case."""

    def __init__(self, n, feats, hidden, classes):
        self.n, self.feats, self.hidden, self.classes = n, feats, hidden, classes
        self.ops = fr.forward_case_operands(n, feats, hidden, classes)
        self.F16, self.ldx, self.ldz = fr.f16_of(feats), fr.f16_of(feats) + fr.LDX_PAD, 2 * classes + fr.LDZ_PAD
        self.ax = fr.ax_buffer(self.ops['ax']).cuda()
        self.w1, self.b1, self.w2 = (fr.f32(self.ops[k]).cuda() for k in ('w1', 'b1', 'w2'))
        self.need = fwd_workspace(n, feats, hidden)
        self.resident = self.need == 0
        self.tickets = 0 if self.resident else fr.wide_groups(n)
        self.words = dropout_ref.bits_words(n * hidden)
        self.ws = self.fresh_ws()

    def fresh_ws(self):
        ws = fr.sentinel_filled(self.need + fr.WS_GUARD, 'cuda')
        if self.tickets:
            ws[self.need - self.tickets:self.need] = 0.0            # the tickets: zero before the first use
        return ws

    def outputs(self):
        return (fr.sentinel_filled((self.n + fr.EXTRA_ROWS, self.hidden), 'cuda'), fr.sentinel_filled((self.n, self.ldz), 'cuda'),
                torch.full((self.words + 8,), -1, dtype=torch.int64, device='cuda'))

    def call(self, pre, z, bits, p, **change):
        a = dict(ldx=self.ldx, ldz=self.ldz, ws_floats=self.need)
        a.update(change)
        rc = fwd_call(self.ax, a['ldx'], self.w1, self.b1, self.w2, pre, z, self.classes, a['ldz'], bits, self.n, self.feats, self.hidden, p,
                      self.ws, a['ws_floats'])
        torch.cuda.synchronize()
        return rc


def run_forward(n, feats, hidden, classes, p, label, decided=None):
    label = (label, dict(n=n, feats=feats, hidden=hidden, classes=classes, p=p))
    c = Forward(n, feats, hidden, classes)
    assert c.resident == fr.first_layer_resident(feats, hidden), label
    assert c.need == (0 if c.resident else fr.wide_ws_floats(n, feats, hidden)), label
    pre, z, bits = c.outputs()
    assert c.call(pre, z, bits, p) == 0, label
    want_pre = fr.forward_pre(c.ops)
    dev_equal(pre[:n], want_pre, label, 'pre')
    untouched(pre[n:], label, 'pre past its last row')
    # the mask: the host's decisions AND pre > 0, nothing past the words of the rows
    if decided is None:
        decided = dropout_ref.decisions(n * hidden, p, SEED, OFFSET) if p > 0.0 else np.ones(n * hidden, dtype=np.bool_)
    words = bits.cpu().numpy().view(np.uint64)
    assert np.array_equal(words[:c.words], dropout_ref.pack_bits(decided & (want_pre.reshape(-1) > 0), n * hidden)), (label, 'bits')
    assert (words[c.words:] == np.uint64(2 ** 64 - 1)).all(), (label, 'bits past the rows were written')
    keep = dropout_ref.unpack_bits(words, n * hidden).reshape(n, hidden)
    _, z_train, z_eval = fr.forward_reference(c.ops, keep, fr.scale_of(p))
    dev_equal(z[:, :classes], z_train, label, 'z_train')
    dev_equal(z[:, classes:2 * classes], z_eval, label, 'z_eval')
    untouched(z[:, 2 * classes:], label, 'padding columns of z')
    untouched(c.ws[c.need:], label, 'the workspace past its stated size')
    if c.tickets:
        assert not c.ws[c.need - c.tickets:c.need].view(torch.int32).any(), (label, 'tickets not zero after the call')
        assert not torch.isnan(c.ws[:c.need - c.tickets]).any(), (label, 'a partial tile was left unwritten')
    else:
        untouched(c.ws, label, 'the workspace of a shape that needs none')
    # a second call into the dirty workspace: the same bits everywhere
    pre2, z2, bits2 = c.outputs()
    assert c.call(pre2, z2, bits2, p) == 0, label
    assert fr.same_bits(pre2, pre) and fr.same_bits(z2, z) and torch.equal(bits2, bits), (label, 'a dirty workspace changed the result')
    untouched(c.ws[c.need:], label, 'the workspace past its stated size (second call)')
    if c.tickets:
        assert not c.ws[c.need - c.tickets:c.need].view(torch.int32).any(), (label, 'tickets not zero after the second call')
    return c


@pytest.mark.parametrize('classes', fr.CLASSES)
@pytest.mark.parametrize('feats,hidden', fr.RESIDENT_SHAPES, ids=[f'F{f}-H{h}-resident' for f, h in fr.RESIDENT_SHAPES])
def test_resident_forward_exact(feats, hidden, classes):
    """k_first_layer_fwd: one to four MFMA steps of 16 columns and the widest W1 either hidden size keeps in LDS (the two-step loop's
    odd tail at 16, 80 and 576 columns); one unit with 1, 15 and 16 live rows, a second unit with 1 and 15, a third with one.  Up to
    33 rows every wave has one unit: the single-unit tail of the walk."""
    for k, n in enumerate(fr.RESIDENT_ROWS):
        units = fr.resident_wave_units(n, cus())
        assert max(units) == 1 and len(units) == fr.cdiv(n, 16)
        c = run_forward(n, feats, hidden, classes, (0.5, 0.0)[k % 2], 'resident, one unit per wave')
        assert c.resident


@pytest.mark.parametrize('walk', ['pair-then-single', 'two-pairs-prefetch'])
def test_resident_forward_walks_pairs_of_units(walk):
    """Rows derived from the CU count: 256·CUs + 1 is the smallest n at which a wave takes NR = 2 units together and ends on a single
    one (units per wave 3; below it the grid still grows and no wave has more than 2), 384·CUs + 1 the smallest with two pairs in
    a wave, the second one's first piece of Â·X loaded under the first one's epilogue.  (p = 0: every decision is keep.)"""
    n = fr.resident_rows_pair_then_single(cus()) if walk == 'pair-then-single' else fr.resident_rows_prefetch(cus())
    if n > fr.ROW_LIMIT:
        pytest.skip(f'{n} rows on {cus()} CUs: above the {fr.ROW_LIMIT}-row limit of a case')
    units = fr.resident_wave_units(n, cus())
    assert max(fr.resident_wave_units(n - 1, cus())) == max(units) - 1
    assert sorted(set(units)) == ([2, 3] if walk == 'pair-then-single' else [1, 4]), (n, sorted(set(units)))
    run_forward(n, 16, 128, 7, 0.0, f'resident, units per wave {sorted(set(units))}')


@pytest.mark.parametrize('hidden,feats,chunks', fr.WIDE_SHAPES, ids=[f'H{h}-F{f}-chunks{c}' for h, f, c in fr.WIDE_SHAPES])
def test_k_chunked_forward_exact(hidden, feats, chunks):
    """k_first_layer_wide at one chunk (a width that is no multiple of 16: W1 staged by scalar loads), a last chunk 16 columns wide,
    and chunk counts below, at, just above and at twice-plus-one the chunks the closing loop keeps in flight (32 / HM: 4 at hidden
    128, 8 at 64).  n = 1, 63, 64, 65: one row group, its last unit ragged, full, and a second group of one row."""
    k = [s[1] for s in fr.WIDE_SHAPES].index(feats)
    classes = fr.CLASSES[k % 3]
    for j, n in enumerate(fr.WIDE_ROWS):
        need = fwd_workspace(n, feats, hidden)
        groups = fr.wide_groups(n)
        assert groups == (2 if n > 64 else 1)
        assert (need - groups) % (fr.cdiv(n, 16) * 16 * hidden) == 0 and (need - groups) // (fr.cdiv(n, 16) * 16 * hidden) == chunks, (need, chunks)
        assert fr.wide_gx(n, feats, hidden, cus()) == groups                  # every workgroup has one row group
        c = run_forward(n, feats, hidden, classes, (0.5, 0.0)[(j + k) % 2], f'K-chunked, {chunks} chunks, {fr.wide_in_flight(hidden)} in flight')
        assert not c.resident


def test_k_chunked_forward_walks_row_groups():
    """n_groups > gx: a workgroup keeps its chunk of W1, walks two row groups and loads the second one's rows under the first one's
    closing sum.  gx = ceil(2·CUs / 17 chunks) at 4112 columns and hidden 64 (31 on 256 CUs); n = 64·gx + 1."""
    feats, hidden = fr.WIDE_WALK
    n = fr.wide_walk_rows(cus())
    if n > fr.ROW_LIMIT:
        pytest.skip(f'{n} rows on {cus()} CUs: above the {fr.ROW_LIMIT}-row limit of a case')
    gx, groups = fr.wide_gx(n, feats, hidden, cus()), fr.wide_groups(n)
    need = fwd_workspace(n, feats, hidden)
    assert (need - groups) // (fr.cdiv(n, 16) * 16 * hidden) == 17 and groups == gx + 1 and fr.cdiv(groups, gx) == 2, (n, gx, groups)
    run_forward(n, feats, hidden, 7, 0.5, f'K-chunked, 17 chunks, gx {gx}, {groups} row groups: workgroup 0 walks 2')


# ---- backward ------------------------------------------------------------------------------------------------------------------
def bwd_workspace(n, feats, hidden):
    need = ctypes.c_int64(-1)
    assert L().dcr_first_layer_bwd_workspace(n, feats, hidden, ctypes.byref(need)) == 0
    return need.value


class Backward:
    def __init__(self, n, feats, hidden, classes):
        self.n, self.feats, self.hidden, self.classes = n, feats, hidden, classes
        self.ops = fr.backward_case_operands(n, feats, hidden, classes)
        self.F16, self.ldx = fr.f16_of(feats), fr.f16_of(feats) + fr.LDX_PAD
        self.ax = fr.ax_buffer(self.ops['ax']).cuda()
        self.dz, self.pre = fr.rows_buffer(self.ops['dz']).cuda(), fr.rows_buffer(self.ops['pre']).cuda()
        self.w2 = fr.f32(self.ops['w2']).cuda()
        self.bits = fr.pack_keep(self.ops['keep']).cuda()
        self.need = bwd_workspace(n, feats, hidden)
        per = hidden * self.F16 + 17 * hidden
        assert self.need > 0 and self.need % per == 0
        self.blocks = self.need // per
        self.ws = fr.sentinel_filled(self.need + fr.WS_GUARD, 'cuda')
        self.sizes = (hidden * feats, hidden, classes * hidden)

    def outputs(self):
        return tuple(fr.sentinel_filled(s + fr.WS_GUARD, 'cuda') for s in self.sizes)

    def call(self, dw1, db1, dw2, p, **change):
        a = dict(ldx=self.ldx, ws_floats=self.need)
        a.update(change)
        rc = L().dcr_first_layer_bwd_f32_dev(self.dz.data_ptr(), self.w2.data_ptr(), self.bits.data_ptr(), self.pre.data_ptr(), self.ax.data_ptr(),
                                             a['ldx'], dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), self.ws.data_ptr(), a['ws_floats'], self.n,
                                             self.feats, self.hidden, self.classes, p, st())
        torch.cuda.synchronize()
        return rc


def run_backward(n, feats, hidden, classes, p, stages_per_wg, label):
    c = Backward(n, feats, hidden, classes)
    reached = fr.cdiv(fr.bwd_stages(n), c.blocks)
    label = (label, dict(n=n, feats=feats, hidden=hidden, classes=classes, p=p, workgroups=c.blocks, stages=fr.bwd_stages(n),
                         stages_per_workgroup=reached, column_blocks=fr.cdiv(c.F16, 256)))
    assert c.blocks == fr.bwd_blocks(n, feats, cus()), label
    assert reached == stages_per_wg, label
    _, want_db1, want_dw2, want_dw1 = fr.backward_reference(c.ops, fr.scale_of(p))
    outs = c.outputs()
    assert c.call(*outs, p) == 0, label
    for out, size, want, name in zip(outs, c.sizes, (want_dw1, want_db1, want_dw2), ('dW1', 'db1', 'dW2')):
        dev_equal(out[:size], want.reshape(-1), label, name)
        untouched(out[size:], label, f'the floats past {name}')
    untouched(c.ws[c.need:], label, 'the workspace past its stated size')
    assert not torch.isnan(c.ws[:c.need]).any(), (label, 'a part of the workspace was left unwritten')
    again = c.outputs()
    assert c.call(*again, p) == 0, label
    assert all(fr.same_bits(a, b) for a, b in zip(again, outs)), (label, 'a dirty workspace changed the result')
    untouched(c.ws[c.need:], label, 'the workspace past its stated size (second call)')
    return c


@pytest.mark.parametrize('classes', fr.CLASSES)
@pytest.mark.parametrize('hidden', [64, 128])
@pytest.mark.parametrize('feats', fr.BWD_SMALL_FEATS)
def test_backward_column_blocks_and_ragged_rows_exact(feats, hidden, classes):
    """k_first_layer_bwd with one stage per workgroup: a 256-column block 16, 240 and 256 columns wide, and a second block 16 wide
    (272); n = 64 + r, r = 1, 15, 16, 17, 31, 32: two whole stages and a last one with one row, a ragged first unit, a full first
    unit, one and fifteen rows in the second unit, and none missing."""
    for k, residue in enumerate(fr.BWD_RESIDUES):
        n = 64 + residue
        assert fr.bwd_stages(n) == 3
        run_backward(n, feats, hidden, classes, (0.5, 0.0)[k % 2], 1, 'backward, 1 stage per workgroup')


def deep_cases():
    return [pytest.param(h, c, s, r, id=f'H{h}-C{c}-stages_per_wg{s}-last_stage_rows{r}') for h, c, s, r, _ in fr.bwd_deep_cases(256)]


@pytest.mark.parametrize('hidden,classes,stages_per_wg,residue', deep_cases())
def test_backward_stage_pipeline_exact(hidden, classes, stages_per_wg, residue):
    """3703 columns (15 column blocks, the last 128 wide with 7 pad columns): few workgroups along the rows (18 on 256 CUs), so a
    workgroup walks 1, 2, 3 or 4 stages — both staging buffers, both parities of the stage loop unrolled by two, the copies of the
    next stage issued between this stage's MFMAs — and the last workgroup one stage fewer, ending on the ragged stage that is
    filled by plain loads.  n is derived from the CU count (about 600 … 2,300 rows on 256 CUs)."""
    n = fr.bwd_rows_for(stages_per_wg, residue, fr.BWD_DEEP_FEATS, cus())
    if n > fr.ROW_LIMIT:
        pytest.skip(f'{n} rows on {cus()} CUs: above the {fr.ROW_LIMIT}-row limit of a case')
    run_backward(n, fr.BWD_DEEP_FEATS, hidden, classes, (0.5, 0.0)[(stages_per_wg + classes) % 2], stages_per_wg,
                 f'backward, {stages_per_wg} stages per workgroup')


@pytest.mark.parametrize('feats,hidden,classes,stages_per_wg,residue', fr.BWD_PIPELINE_EXTRA,
                         ids=[f'F{f}-H{h}-C{c}-stages_per_wg{s}-last_stage_rows{r}' for f, h, c, s, r in fr.BWD_PIPELINE_EXTRA])
def test_backward_stage_pipeline_narrow_blocks_exact(feats, hidden, classes, stages_per_wg, residue):
    """The pipeline where a stage's copy of Â·X is two wave-instructions (a 16-column block: only two of the eight waves copy): the
    second column block of 272 columns, and 16 columns."""
    n = fr.bwd_rows_for(stages_per_wg, residue, feats, cus())
    if n > fr.ROW_LIMIT:
        pytest.skip(f'{n} rows on {cus()} CUs: above the {fr.ROW_LIMIT}-row limit of a case')
    run_backward(n, feats, hidden, classes, 0.5, stages_per_wg, f'backward, {stages_per_wg} stages per workgroup')


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refused_forward_calls_write_nothing():
    """ldx below F16, ldx no multiple of 4, ldz below the classes, a workspace one float short: an error code and a message, and
    pre, z, bits and the workspace as they were; the next valid call is exact."""
    n, feats, hidden, classes = 65, 272, 128, 7
    c = Forward(n, feats, hidden, classes)
    pre, z, bits = c.outputs()
    before = c.ws.clone()
    for label, change in (('ldx < F16', dict(ldx=c.F16 - 4)), ('ldx % 4', dict(ldx=c.F16 + 2)), ('ldz < classes', dict(ldz=classes - 1)),
                          ('workspace one float short', dict(ws_floats=c.need - 1))):
        assert c.call(pre, z, bits, 0.5, **change) != 0, label
        assert len(L().dcr_last_error()) > 0, label
        untouched(pre, label, 'pre')
        untouched(z, label, 'z')
        assert bool((bits == -1).all()), (label, 'bits were written')
        assert fr.same_bits(c.ws, before), (label, 'the workspace was written')
    run_forward(n, feats, hidden, classes, 0.5, 'valid call after the refusals')
    r = Forward(33, 64, 128, 7)                                                   # the resident kernel takes no workspace: strides only
    pre, z, bits = r.outputs()
    for label, change in (('ldx < F16', dict(ldx=60)), ('ldx % 4', dict(ldx=66)), ('ldz < classes', dict(ldz=6))):
        assert r.call(pre, z, bits, 0.5, **change) != 0, label
        untouched(pre, label, 'pre')
        untouched(z, label, 'z')
        assert bool((bits == -1).all()), (label, 'bits were written')


def test_refused_backward_calls_write_nothing():
    n, feats, hidden, classes = 81, 272, 64, 7
    c = Backward(n, feats, hidden, classes)
    outs = c.outputs()
    for label, change in (('ldx < F16', dict(ldx=c.F16 - 4)), ('ldx % 4', dict(ldx=c.F16 + 2)), ('workspace one float short', dict(ws_floats=c.need - 1))):
        assert c.call(*outs, 0.5, **change) != 0, label
        assert len(L().dcr_last_error()) > 0, label
        for out, name in zip(outs, ('dW1', 'db1', 'dW2')):
            untouched(out, label, name)
        untouched(c.ws, label, 'the workspace')
    run_backward(n, feats, hidden, classes, 0.5, 1, 'valid call after the refusals')
