"""Every dropout keep bit of the GCN kernels against a host Philox (tests/dropout_ref.py, pinned on the CPU by
tests/test_dropout_stream_cpu.py): the rule include/dcr.h states in its dropout section, compared bit for bit — no tolerance
on any bit, on any kept value or on any masked gradient entry.  Contractions are bounded a priori against float64:
    forward   |z - h·Wᵀ|        <= (H + 2) 2^-24 (|h|·|W|ᵀ)            any summation order, fused multiply-adds or not
    backward  |dx - m (dz·W) s|  <= (C + 2) 2^-24 s (|dz|·|W|)          s = 1 / (1 - p): C products, the scale and its rounding
    sums over n rows (column sums, dW, dW1, db1): max(1e-5, 4 · 2^-23 · sqrt(n)) of the largest reference entry (tests/test_gcn.py).
The backward kernels get masks from numpy's generator — not from Philox, not tied to the sign of x — packed by dropout_ref: they
must read the layout include/dcr.h documents, not merely the one a forward kernel of the same build writes.

dcr_act_linear_bwd_f32_dev's grid cap (4.2 M rows) stays out: a case above it would move gigabytes for one grid-stride step."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dropout_ref
from conftest import PKG

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEEDS = (5, 0x123456789ABCDEF0, 2 ** 64 - 1)                  # small, a non-zero high word, every bit set
PS = (0.0, 0.5, 0.3, 2.0 ** -16, 1.0 - 2.0 ** -20)
TAILS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 3001 * 129)


def _lib():
    from dcr import _lib as loader
    return loader


def _dev():
    return torch.device('cuda', 0)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _ok(rc):
    _lib().check(rc)


def _up(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(_dev())


def _words(t):
    return t.cpu().numpy().view(np.uint64)


def _bits32(t):
    """The float32 tensor's bit patterns (so that -0.0 and +0.0 differ and NaN equals itself)."""
    return t.detach().cpu().numpy().view(np.uint32)


def _same_f32(got_t, want_np):
    return np.array_equal(_bits32(got_t).reshape(-1), np.ascontiguousarray(want_np, dtype=np.float32).view(np.uint32).reshape(-1))


def _counter_cell(value):
    return _up(np.array([value], dtype=np.uint64))


def _special_values(shape, rng):
    """float32 normals with exact +0.0, -0.0, denormals of both signs and tiny / huge magnitudes sprinkled in."""
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    specials = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1e-39, -1.1e-39, 1.17549435e-38, -1.17549435e-38, 3.0e4, -3.0e4],
                        dtype=np.float32)
    if flat.size <= 8:
        idx = np.arange(flat.size)
        flat[idx[::2]] = specials[rng.integers(0, specials.size, idx[::2].size)]
    else:
        idx = rng.choice(flat.size, size=max(4, flat.size // 8), replace=False)
        flat[idx] = specials[rng.integers(0, specials.size, idx.size)]
    return x


def _mask(shape, rng):
    return rng.random(shape) < 0.6


def _sum_rel(n):
    return max(1e-5, 4.0 * 2.0 ** -23 * float(n) ** 0.5)


def _close_sum(got_t, want, n):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got_t.detach().cpu().numpy().astype(np.float64).reshape(want.shape) - want).max()
    return err <= _sum_rel(n) * max(np.abs(want).max(), 1e-30)


def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


# ---- the stand-alone kernel ----------------------------------------------------------------------------------------------

def _standalone(x_np, x_t, p, seed, offset, cell_value, words):
    """One call of the stand-alone kernel (the counter entry point when cell_value is not None) -> (y, bits) tensors; y has
    eight guard elements and bits starts poisoned, so a stray or a missing store shows."""
    L, n = _lib().lib(), x_np.size
    y = torch.full((n + 8,), float('nan'), device=_dev())
    bits = torch.full((words,), -1, dtype=torch.int64, device=_dev())
    if cell_value is None:
        _ok(L.dcr_relu_dropout_fwd_f32_dev(x_t.data_ptr(), y.data_ptr(), bits.data_ptr(), n, p, seed, offset, _st()))
    else:
        cell = _counter_cell(cell_value)
        _ok(L.dcr_relu_dropout_fwd_f32_ctr_dev(x_t.data_ptr(), y.data_ptr(), bits.data_ptr(), n, p, seed, offset, cell.data_ptr(), _st()))
        torch.cuda.synchronize()
        assert int(_words(cell)[0]) == cell_value              # the kernel reads the counter; the caller moves it
    torch.cuda.synchronize()
    assert torch.isnan(y[n:]).all()
    return y[:n], bits


def _check_standalone(x_np, x_t, p, seed, offset, cell_value, words):
    o = dropout_ref.stream_offset(offset, cell_value or 0)
    want_y, keep = dropout_ref.relu_dropout(x_np, p, seed, o)
    y, bits = _standalone(x_np, x_t, p, seed, offset, cell_value, words)
    what = (x_np.size, p, hex(seed), hex(offset), cell_value)
    got = _words(bits)
    assert np.array_equal(got, dropout_ref.pack_bits(keep, x_np.size, words=words)), what    # pad bits and pad words zero
    assert _same_f32(y, want_y), what
    assert int(np.unpackbits(got.view(np.uint8)).sum()) == int(keep.sum()), what
    return _bits32(y).copy(), got.copy()


OFFSET_CASES = ((0, None), (2 ** 32 - 1, 3), (2 ** 40 + 7, None), (2 ** 40, 7), (5, 2 ** 40 + 2))


@pytest.mark.parametrize('n', TAILS)
def test_standalone_kernel_every_bit(n):
    """dcr_relu_dropout_fwd_f32_dev and _ctr_dev: bits, pad bits, y and the kept count against the host stream, for every p,
    seed and offset case; 2^32 - 1 with *offset_dev = 3 carries into the counter's high word; 2^40 + 7 given whole and split
    two ways between offset and *offset_dev gives the same call."""
    L = _lib().lib()
    rng = np.random.default_rng(1000 + n)
    x_np = _special_values(n, rng)
    x_t = _up(x_np)
    words = ctypes.c_int64()
    _ok(L.dcr_relu_dropout_bits_words(n, ctypes.byref(words)))
    assert words.value >= dropout_ref.bits_words(n)
    for p in PS:
        for seed in SEEDS:
            seen = {}
            for offset, cell in OFFSET_CASES:
                res = _check_standalone(x_np, x_t, p, seed, offset, cell, words.value)
                o = dropout_ref.stream_offset(offset, cell or 0)
                if o in seen:
                    assert np.array_equal(seen[o][0], res[0]) and np.array_equal(seen[o][1], res[1])
                seen[o] = res
            assert len(seen) == 3


def test_standalone_kernel_beyond_2_to_24_elements():
    """n = 2^24 + 5: quad indices past 2^22, a tail of one element in the last quad.  (One n this large; p at both ends of
    the threshold's range and in the middle, the seed with every bit set, the carrying offset.)"""
    L = _lib().lib()
    n = 2 ** 24 + 5
    rng = np.random.default_rng(7)
    x_np = _special_values(n, rng)
    x_t = _up(x_np)
    words = ctypes.c_int64()
    _ok(L.dcr_relu_dropout_bits_words(n, ctypes.byref(words)))
    for p, seed, offset, cell in ((0.5, 2 ** 64 - 1, 2 ** 32 - 1, 3), (1.0 - 2.0 ** -20, SEEDS[1], 2 ** 40 + 7, None),
                                  (2.0 ** -16, 5, 2 ** 40, 7)):
        _check_standalone(x_np, x_t, p, seed, offset, cell, words.value)


def test_counter_wraps_as_a_64_bit_sum():
    n = 1025
    x_np = _special_values(n, np.random.default_rng(3))
    words = ctypes.c_int64()
    _ok(_lib().lib().dcr_relu_dropout_bits_words(n, ctypes.byref(words)))
    _check_standalone(x_np, _up(x_np), 0.3, SEEDS[1], 2 ** 64 - 1, 2, words.value)     # o = 1


# ---- activation fused into the next contraction ------------------------------------------------------------------------------

def _act_linear_row_cap():
    """Rows one launch of dcr_act_linear_fwd_f32_dev covers without its grid stride, read from the launcher: the cap on the
    workgroups times 4 waves times 16 rows."""
    src = open(os.path.join(PKG, 'csrc', 'dcr_gcn.hip')).read()
    body = src[src.index('static void launch_act_linear_fwd('):]
    m = re.search(r'if \(blocks > ([0-9][0-9 *]*)\) blocks = ([0-9][0-9 *]*);', body)
    assert m and m.group(1).strip() == m.group(2).strip(), 'launch_act_linear_fwd: grid cap not found'
    assert 'int64_t blocks = (n_waves + 3) / 4;' in body and 'n_waves = (n_rows + 15) / 16;' in body
    cap = 1
    for f in m.group(1).split('*'):
        cap *= int(f)
    return cap * 4 * 16


ACT_ROWS = (1, 3, 15, 16, 17, 65, 5003)
ACT_P = {1: 0.5, 3: 2.0 ** -16, 15: 0.3, 16: 1.0 - 2.0 ** -20, 17: 0.0, 65: 0.3, 5003: 0.4}


def _act_linear_case(hidden, classes, n, p, seed, offset, cell_value, rng_seed):
    L = _lib().lib()
    rng = np.random.default_rng(rng_seed)
    x_np = _special_values((n, hidden), rng)
    w_np = (rng.standard_normal((classes, hidden)) * 0.1).astype(np.float32)
    x_t, w_t = _up(x_np), _up(w_np)
    o = dropout_ref.stream_offset(offset, cell_value)
    want_h, keep = dropout_ref.relu_dropout(x_np, p, seed, o)
    need = dropout_ref.bits_words(n * hidden)
    want_bits = dropout_ref.pack_bits(keep, n * hidden)
    absw = np.abs(w_np.astype(np.float64)).T
    want_tr = want_h.astype(np.float64) @ w_np.astype(np.float64).T
    bound_tr = (hidden + 2) * U * (np.abs(want_h.astype(np.float64)) @ absw)
    relu = np.where(x_np > 0, x_np, np.float32(0.0)).astype(np.float64)
    want_ev = relu @ w_np.astype(np.float64).T
    bound_ev = (hidden + 2) * U * (relu @ absw)
    cell = _counter_cell(cell_value)

    def call(train, evaluate, store_h):
        both = train and evaluate
        ldz = 2 * classes if both else classes
        z = torch.full((n, ldz), float('nan'), device=_dev())
        z_tr = z[:, :classes] if train else None
        z_ev = (z[:, classes:] if both else z) if evaluate else None
        h = torch.full((n, hidden), float('nan'), device=_dev()) if store_h else None
        bits = torch.full((need + 8,), -1, dtype=torch.int64, device=_dev())
        _ok(L.dcr_act_linear_fwd_f32_dev(x_t.data_ptr(), w_t.data_ptr(), None if h is None else h.data_ptr(),
                                         None if z_tr is None else z_tr.data_ptr(), None if z_ev is None else z_ev.data_ptr(), ldz,
                                         bits.data_ptr(), n, hidden, classes, p, seed, offset, cell.data_ptr(), _st()))
        torch.cuda.synchronize()
        what = (hidden, classes, n, p, train, evaluate)
        got = _words(bits)
        assert (got[need:] == np.uint64(2 ** 64 - 1)).all(), what                 # nothing past the words the rows reach
        if train:
            assert np.array_equal(got[:need], want_bits), what
            err = np.abs(z_tr.cpu().numpy().astype(np.float64) - want_tr)
            assert (err <= bound_tr).all(), (what, float((err - bound_tr).max()))
            if store_h:
                assert _same_f32(h, want_h), what
        else:
            assert (got[:need] == np.uint64(2 ** 64 - 1)).all(), what             # an evaluation call draws nothing
        if evaluate:
            err = np.abs(z_ev.cpu().numpy().astype(np.float64) - want_ev)
            assert (err <= bound_ev).all(), (what, float((err - bound_ev).max()))
        return z.cpu().numpy().view(np.uint32)

    pair = call(True, True, True)
    only_tr = call(True, False, False)
    only_ev = call(False, True, False)
    assert np.array_equal(pair[:, :classes], only_tr) and np.array_equal(pair[:, classes:], only_ev)
    assert int(_words(cell)[0]) == cell_value


@pytest.mark.parametrize('classes', [1, 6, 7, 16])
@pytest.mark.parametrize('hidden', [64, 128])
def test_act_linear_forward_every_bit(hidden, classes):
    """dcr_act_linear_fwd_f32_dev, pair / train-only / eval-only: the bits are the host stream's on x, h_train the exact product,
    both z within the a-priori bound of a float64 contraction."""
    for k, n in enumerate(ACT_ROWS):
        _act_linear_case(hidden, classes, n, ACT_P[n], SEEDS[k % 3], 2 ** 32 - 1, 3, 100 * hidden + 10 * classes + k)


@pytest.mark.parametrize('hidden,classes', [(128, 16), (64, 7)])
def test_act_linear_forward_above_the_grid_cap(hidden, classes):
    cap = _act_linear_row_cap()
    n = 131072 + 17
    assert n > cap, f'the grid cap moved to {cap} rows: choose a larger n for this test'
    _act_linear_case(hidden, classes, n, 0.3, SEEDS[1], 2 ** 40, 7, 17)


# ---- the one-kernel first layer and the decisions drawn ahead of it ----------------------------------------------------------

FIRST_SHAPES = ((256, 128), (16, 128), (32, 64), (1433, 128), (3703, 64), (23, 64))


def _first_layer_rows(feats, hidden):
    """The edge sizes, and one above the rows a single pass of the grid covers (the launchers of csrc/dcr_gcn_first.hip: the
    resident kernel runs at most one workgroup of 8 waves x 2 units x 16 rows per CU; the K-chunked one ceil(2 CUs / chunks)
    workgroups of 64 rows per chunk), checked against the library's own statement of which kernel takes the shape."""
    L = _lib().lib()
    ws = ctypes.c_int64()
    _ok(L.dcr_first_layer_fwd_workspace(1000, feats, hidden, ctypes.byref(ws)))
    resident = ws.value == 0
    assert resident == (feats % 16 == 0 and 4 * (hidden * ((feats + 63) // 64 * 64) + 17 * hidden) <= 160 * 1024)
    if resident:
        cap = _cus() * 8 * 2 * 16
    else:
        f16 = (feats + 15) // 16 * 16
        kch = 16384 // hidden
        chunks = (f16 + kch - 1) // kch
        cap = (2 * _cus() + chunks - 1) // chunks * 64
    big = cap + 65
    assert big > cap
    return (1, 63, 64, 65, 2485, big), resident


@pytest.mark.parametrize('feats,hidden', FIRST_SHAPES)
def test_first_layer_forward_every_bit(feats, hidden):
    """dcr_first_layer_fwd_ws_f32_dev, both kernels: the bits are the host stream's applied to the pre-activation the kernel
    wrote; dcr_dropout_words_dev's words are the packed decisions and its stamp {o, seed, threshold, n_rows}; a call given
    those words gives the same bits, and a call given words stamped for another offset ignores them.  Every buffer starts
    poisoned: the words' fields of a row group's rows past n_rows must come out zero too (they once were left unwritten)."""
    L = _lib().lib()
    classes, p, seed, offset, cell_value = 7, 0.3, SEEDS[1], 2 ** 32 - 1, 3
    o = dropout_ref.stream_offset(offset, cell_value)
    rows, resident = _first_layer_rows(feats, hidden)
    f16 = (feats + 15) // 16 * 16
    g = torch.Generator(device=_dev()).manual_seed(feats * 1000 + hidden)
    w1 = torch.randn(hidden, feats, device=_dev(), generator=g) * (feats ** -0.5)
    b1 = torch.randn(hidden, device=_dev(), generator=g) * 0.1
    w2 = torch.randn(classes, hidden, device=_dev(), generator=g) * 0.1
    cell = _counter_cell(cell_value)
    for n in rows:
        what = (feats, hidden, n)
        axp = torch.zeros(n, f16, device=_dev())
        axp[:, :feats] = torch.randn(n, feats, device=_dev(), generator=g)
        wsf = ctypes.c_int64()
        _ok(L.dcr_first_layer_fwd_workspace(n, feats, hidden, ctypes.byref(wsf)))
        assert (wsf.value == 0) == resident
        ws = torch.zeros(max(wsf.value, 4), device=_dev())
        need = dropout_ref.bits_words(n * hidden)
        assert need == dropout_ref.stamp_index(n, hidden)
        count = ctypes.c_int64()
        _ok(L.dcr_dropout_words_count(n, hidden, ctypes.byref(count)))
        assert count.value == need + 8

        def forward(dwords):
            pre = torch.full((n, hidden), float('nan'), device=_dev())
            both = torch.full((n, 2 * classes), float('nan'), device=_dev())
            bits = torch.full((need + 8,), -1, dtype=torch.int64, device=_dev())
            _ok(L.dcr_first_layer_fwd_ws_f32_dev(axp.data_ptr(), f16, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), pre.data_ptr(),
                                                 both.data_ptr(), both.data_ptr() + 4 * classes, 2 * classes, bits.data_ptr(),
                                                 None if dwords is None else dwords.data_ptr(), n, feats, hidden, classes, p, seed,
                                                 offset, cell.data_ptr(), ws.data_ptr(), wsf.value, _st()))
            torch.cuda.synchronize()
            assert not torch.isnan(pre).any() and not torch.isnan(both).any(), what
            return pre, both, _words(bits)

        def draw(off, cell_t):
            dwords = torch.full((count.value,), -1, dtype=torch.int64, device=_dev())
            _ok(L.dcr_dropout_words_dev(dwords.data_ptr(), n, hidden, p, seed, off, None if cell_t is None else cell_t.data_ptr(), _st()))
            torch.cuda.synchronize()
            return dwords

        pre, both, bits = forward(None)
        pre_np = pre.cpu().numpy()
        decided = dropout_ref.decisions(n * hidden, p, seed, o)
        want_bits = dropout_ref.pack_bits(decided & (pre_np.reshape(-1) > 0), n * hidden)
        assert np.array_equal(bits[:need], want_bits), what
        assert (bits[need:] == np.uint64(2 ** 64 - 1)).all(), what
        # drawn ahead: the decisions, the stamp, and the same call through them
        dwords = draw(offset, cell)
        got = _words(dwords)
        assert np.array_equal(got[:need], dropout_ref.pack_bits(decided, n * hidden)), what
        assert np.array_equal(got[need:need + 4], dropout_ref.words_stamp(p, seed, o, n)), what
        assert (got[need + 4:] == np.uint64(2 ** 64 - 1)).all(), what
        pre_d, both_d, bits_d = forward(dwords)
        assert torch.equal(pre_d, pre) and torch.equal(both_d, both), what
        assert np.array_equal(bits_d[:need], want_bits) and (bits_d[need:] == np.uint64(2 ** 64 - 1)).all(), what
        assert int(_words(dwords)[need + 4]) == dropout_ref.stream_offset(o, 1), what     # the offset of the call expected next
        # words of another call (offset o + 5, given whole): ignored
        other = draw(dropout_ref.stream_offset(o, 5), None)
        got = _words(other)
        other_decided = dropout_ref.decisions(n * hidden, p, seed, dropout_ref.stream_offset(o, 5))
        assert np.array_equal(got[:need], dropout_ref.pack_bits(other_decided, n * hidden)), what
        assert np.array_equal(got[need:need + 4], dropout_ref.words_stamp(p, seed, dropout_ref.stream_offset(o, 5), n)), what
        if n * hidden >= 64:
            assert not np.array_equal(other_decided, decided)
        pre_o, both_o, bits_o = forward(other)
        assert torch.equal(pre_o, pre) and torch.equal(both_o, both), what
        assert np.array_equal(bits_o[:need], want_bits), what
        if not resident:
            n_groups = ((n + 15) // 16 + 3) // 4
            assert int(ws[wsf.value - n_groups:].view(torch.int32).abs().sum().item()) == 0     # the tickets are zero again
    assert int(_words(cell)[0]) == cell_value


# ---- backward kernels on masks made on the host ------------------------------------------------------------------------------

@pytest.mark.parametrize('n', TAILS)
def test_relu_dropout_backward_applies_a_host_mask(n):
    L = _lib().lib()
    rng = np.random.default_rng(2000 + n)
    words = ctypes.c_int64()
    _ok(L.dcr_relu_dropout_bits_words(n, ctypes.byref(words)))
    g_np = _special_values(n, rng)
    g_t = _up(g_np)
    for p in (0.3, 0.5, 1.0 - 2.0 ** -20, 0.0):
        mask = _mask(n, rng)
        bits = _up(dropout_ref.pack_bits(mask, n, words=words.value))
        gin = torch.full((n + 8,), float('nan'), device=_dev())
        _ok(L.dcr_relu_dropout_bwd_f32_dev(g_t.data_ptr(), gin.data_ptr(), bits.data_ptr(), n, p, _st()))
        torch.cuda.synchronize()
        want = np.where(mask, g_np * dropout_ref.scale32(p), np.float32(0.0)).astype(np.float32)
        assert _same_f32(gin[:n], want), (n, p)
        assert torch.isnan(gin[n:]).all()


BWD_ROWS = (1, 255, 256, 257, 5003)


def _backward_case(hidden, classes, n, p, rng_seed):
    """All four backward kernels on one host-made mask."""
    L = _lib().lib()
    rng = np.random.default_rng(rng_seed)
    feats = 300 if n == 5003 else 23                        # 300: two 256-column tiles of the input width in the one-kernel backward
    f16 = (feats + 15) // 16 * 16
    scale = 1.0 / (1.0 - p)
    mask = _mask((n, hidden), rng)
    dz = rng.standard_normal((n, classes)).astype(np.float32)
    w = (rng.standard_normal((classes, hidden)) * 0.1).astype(np.float32)
    x = rng.standard_normal((n, hidden)).astype(np.float32)             # the pre-activation: its sign is NOT the mask's
    ax = np.zeros((n, f16), dtype=np.float32)
    ax[:, :feats] = rng.standard_normal((n, feats)).astype(np.float32)
    dz64, w64, x64 = dz.astype(np.float64), w.astype(np.float64), x.astype(np.float64)
    want_dx = np.where(mask, (dz64 @ w64) * scale, 0.0)
    bound_dx = (classes + 2) * U * scale * (np.abs(dz64) @ np.abs(w64))
    want_cs = want_dx.sum(0)
    h64 = np.where(mask, x64 * scale, 0.0)
    want_dw = dz64.T @ h64
    want_dw1 = want_dx.T @ ax[:, :feats].astype(np.float64)
    need = dropout_ref.bits_words(n * hidden)
    bits = _up(dropout_ref.pack_bits(mask, n * hidden, words=need + 4))
    dz_t, w_t, x_t, ax_t = _up(dz), _up(w), _up(x), _up(ax)
    what = (hidden, classes, n, p)

    def check_dx(dx, name):
        got = dx.cpu().numpy()
        assert not got[~mask].any(), (name, what)                            # a masked entry is exactly zero
        err = np.abs(got.astype(np.float64) - want_dx)
        assert (err <= bound_dx).all(), (name, what, float((err - bound_dx).max()))

    def fresh(*shape):
        return torch.full(shape, float('nan'), device=_dev())

    dx = fresh(n, hidden)
    _ok(L.dcr_act_linear_bwd_f32_dev(dz_t.data_ptr(), w_t.data_ptr(), bits.data_ptr(), dx.data_ptr(), n, hidden, classes, p, _st()))
    torch.cuda.synchronize()
    check_dx(dx, 'act_linear_bwd')

    wsf = ctypes.c_int64()
    _ok(L.dcr_act_linear_bwd_workspace(n, hidden, ctypes.byref(wsf)))
    ws, dx, cs = fresh(max(wsf.value, 1)), fresh(n, hidden), fresh(hidden)
    _ok(L.dcr_act_linear_bwd_colsum_f32_dev(dz_t.data_ptr(), w_t.data_ptr(), bits.data_ptr(), dx.data_ptr(), cs.data_ptr(), ws.data_ptr(),
                                            wsf.value, n, hidden, classes, p, _st()))
    torch.cuda.synchronize()
    check_dx(dx, 'act_linear_bwd_colsum')
    assert _close_sum(cs, want_cs, n), ('act_linear_bwd_colsum column sums', what)

    _ok(L.dcr_act_linear_bwd_fused_workspace(n, hidden, ctypes.byref(wsf)))
    ws, dx, cs, dw = fresh(max(wsf.value, 1)), fresh(n, hidden), fresh(hidden), fresh(classes, hidden)
    _ok(L.dcr_act_linear_bwd_fused_f32_dev(dz_t.data_ptr(), w_t.data_ptr(), bits.data_ptr(), x_t.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                           cs.data_ptr(), ws.data_ptr(), wsf.value, n, hidden, classes, p, _st()))
    torch.cuda.synchronize()
    check_dx(dx, 'act_linear_bwd_fused')
    assert _close_sum(cs, want_cs, n), ('act_linear_bwd_fused column sums', what)
    assert _close_sum(dw, want_dw, n), ('act_linear_bwd_fused dW', what)
    fused_blocks = wsf.value // (17 * hidden)

    _ok(L.dcr_first_layer_bwd_workspace(n, feats, hidden, ctypes.byref(wsf)))
    ws, dw1, db1, dw2 = fresh(max(wsf.value, 4)), fresh(hidden, feats), fresh(hidden), fresh(classes, hidden)
    _ok(L.dcr_first_layer_bwd_f32_dev(dz_t.data_ptr(), w_t.data_ptr(), bits.data_ptr(), x_t.data_ptr(), ax_t.data_ptr(), f16, dw1.data_ptr(),
                                      db1.data_ptr(), dw2.data_ptr(), ws.data_ptr(), wsf.value, n, feats, hidden, classes, p, _st()))
    torch.cuda.synchronize()
    assert _close_sum(db1, want_cs, n), ('first_layer_bwd db1', what)
    assert _close_sum(dw2, want_dw, n), ('first_layer_bwd dW2', what)
    assert _close_sum(dw1, want_dw1, n), ('first_layer_bwd dW1', what)
    return fused_blocks


@pytest.mark.parametrize('classes', [1, 7, 16])
@pytest.mark.parametrize('hidden', [64, 128])
def test_backward_kernels_apply_a_host_mask(hidden, classes):
    """dcr_act_linear_bwd_f32_dev, _colsum_, dcr_act_linear_bwd_fused_f32_dev and dcr_first_layer_bwd_f32_dev on a mask that no
    forward kernel wrote: dx within the a-priori bound of float64 mask (dz·W) / (1 - p) and exactly zero where masked; the sums
    over rows within the project's bound for float32 sums of n terms."""
    for k, n in enumerate(BWD_ROWS):
        _backward_case(hidden, classes, n, (0.3, 0.5)[k % 2], 10000 * hidden + 100 * classes + k)


def test_backward_kernels_above_the_fused_grid_cap():
    n = 262144 + 257
    blocks = _backward_case(64, 7, n, 0.3, 99)
    assert blocks < (n + 255) // 256, f'{blocks} workgroups cover {n} rows without a grid stride: choose a larger n for this test'


# ---- the Python wiring: which seed, which offset, and who moves the counter --------------------------------------------------

@pytest.fixture
def stream_state():
    """A seed with its top bit set and a counter about to carry into its high word; both put back afterwards."""
    from models import gcn
    gcn.set_aggregate_backend('hip')
    ctr = gcn._dropout_counter(_dev())
    saved_ctr, saved_seed = ctr.clone(), torch.initial_seed()
    seed = 2 ** 63 + 12345
    torch.manual_seed(seed)
    ctr.fill_(2 ** 32 - 2)
    yield gcn, ctr, seed
    ctr.copy_(saved_ctr)
    torch.manual_seed(saved_seed)


def test_python_calls_use_the_torch_seed_and_the_device_counter(stream_state):
    gcn, ctr, seed = stream_state
    from models.gcn import _ActLinearFn, _FirstLayerFn, _ReluDropoutFn
    assert torch.initial_seed() == seed
    rng = np.random.default_rng(12)
    n, hidden, classes, feats, p = 333, 64, 7, 48, 0.3
    x_np = _special_values((n, hidden), rng)
    x = _up(x_np)
    w = _up((rng.standard_normal((classes, hidden)) * 0.1).astype(np.float32))
    c = int(ctr.item())
    assert c == 2 ** 32 - 2

    y = _ReluDropoutFn.apply(x, p)
    want_y, keep = dropout_ref.relu_dropout(x_np, p, seed, c)
    assert _same_f32(y, want_y) and int(ctr.item()) == c + 1
    need = dropout_ref.bits_words(n * hidden)

    z_tr, z_ev = _ActLinearFn.apply(x.clone().requires_grad_(True), w, p, True, True)
    _, keep = dropout_ref.relu_dropout(x_np, p, seed, c + 1)
    assert np.array_equal(_words(z_tr.grad_fn.bits)[:need], dropout_ref.pack_bits(keep, n * hidden))
    assert int(ctr.item()) == c + 2
    _ActLinearFn.apply(x, w, 0.0, False, True)                               # evaluation only: draws nothing, advances nothing
    assert int(ctr.item()) == c + 2
    drop = torch.nn.Dropout(p).eval()
    assert torch.equal(gcn.relu_dropout(x, torch.nn.ReLU(), drop), torch.relu(x)) and int(ctr.item()) == c + 2

    ax = _up(rng.standard_normal((n, feats)).astype(np.float32))
    w1 = _up((rng.standard_normal((hidden, feats)) * feats ** -0.5).astype(np.float32)).requires_grad_(True)
    b1 = _up((rng.standard_normal(hidden) * 0.1).astype(np.float32))
    f_tr, f_ev = _FirstLayerFn.apply(ax, w1, b1, w, p, True, True)           # offset c + 2 = 2^32: the carry
    assert c + 2 == 2 ** 32
    pre = f_tr.grad_fn.pre.cpu().numpy()
    keep = dropout_ref.decisions(n * hidden, p, seed, c + 2) & (pre.reshape(-1) > 0)
    assert np.array_equal(_words(f_tr.grad_fn.bits)[:need], dropout_ref.pack_bits(keep, n * hidden))
    assert int(ctr.item()) == c + 3
    _FirstLayerFn.apply(ax, w1.detach(), b1, w, 0.0, False, True)
    assert int(ctr.item()) == c + 3


def test_captured_call_draws_the_next_offset_at_every_replay(stream_state):
    """One relu_dropout call captured on a single stream (no side streams): the launch parameters are constants, the counter
    in device memory moves — replays give the masks of offsets c0, c0 + 1, c0 + 2."""
    gcn, ctr, seed = stream_state
    rng = np.random.default_rng(13)
    p = 0.5
    x_np = _special_values((257, 129), rng)
    x = _up(x_np)
    act, drop = torch.nn.ReLU(), torch.nn.Dropout(p).train()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gcn.relu_dropout(x, act, drop)                                        # (eager first: nothing is created inside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    c0 = int(ctr.item())
    assert c0 == 2 ** 32 - 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        y = gcn.relu_dropout(x, act, drop)
    torch.cuda.synchronize()
    assert int(ctr.item()) == c0                                              # a capture runs nothing
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        want_y, _ = dropout_ref.relu_dropout(x_np, p, seed, c0 + k)
        assert _same_f32(y, want_y), k
        assert int(ctr.item()) == c0 + k + 1
