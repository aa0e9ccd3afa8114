"""Plain restatement of the GCN dropout stream, for the tests to check the kernels against.

Written from the rule include/dcr.h states in its dropout section (numpy only; the Philox rounds are cheeger_ref's, which
tests/test_cheeger_cpu.py and tests/test_dropout_stream_cpu.py pin to the Random123 known answer).  Nothing here imports the
package under test or holds device code: the checker does not live in what it checks.

For a tensor of n elements in row-major order, element e = 4t + j (quad t, j in 0..3), o = offset + *offset_dev (64-bit sum):
    r        = Philox-4x32-10(counter {lo32(t >> 1), hi32(t >> 1), lo32(o), hi32(o)}, key {lo32(seed), hi32(seed)})
    draw     = (r[j] >> 16 (t & 1)) & 0xFFFF
    decision = draw >= min(floor(p 65536), 65535)
    keep     = decision and x[e] > 0
    y[e]     = keep ? x[e] * float32(1 / (1 - p)) : 0
    bit t & 63 of word 4 (t >> 6) + j of `bits` is keep; bits of no element are 0.
A row-structured [n_rows x H] activation is the same with t = row H/4 + col/4, j = col % 4 (its row-major flattening).
"""
import numpy as np

import cheeger_ref

_M64 = 0xFFFFFFFFFFFFFFFF
_M32 = 0xFFFFFFFF


def threshold(p):
    """min(floor(p 65536), 65535): an element is kept when its 16-bit draw is >= this, so P(keep) = 1 - threshold / 65536."""
    th = int(np.floor(np.float64(p) * np.float64(65536.0)))
    return min(th, 65535)


def scale32(p):
    """float32(1 / (1 - p)), the quotient formed in float64."""
    return np.float32(np.float64(1.0) / (np.float64(1.0) - np.float64(p)))


def stream_offset(offset, offset_dev=0):
    """o = offset + *offset_dev as the 64-bit sum (wraps at 2^64)."""
    return (int(offset) + int(offset_dev)) & _M64


def draws(n, seed, offset):
    """uint16 [n]: the 16-bit draw of every element of an n-element tensor under (seed, o = offset)."""
    n, seed, offset = int(n), int(seed) & _M64, int(offset) & _M64
    quads = (n + 3) // 4
    calls = (quads + 1) // 2
    c = np.arange(calls, dtype=np.uint64)
    r = cheeger_ref.philox4x32_10(c & np.uint64(_M32), c >> np.uint64(32), np.full(calls, offset & _M32, dtype=np.uint64),
                                  np.full(calls, offset >> 32, dtype=np.uint64), seed & _M32, seed >> 32)
    out = np.empty((calls, 2, 4), dtype=np.uint16)     # [call t >> 1][half t & 1][j]
    for j in range(4):
        out[:, 0, j] = r[j] & np.uint64(0xFFFF)
        out[:, 1, j] = (r[j] >> np.uint64(16)) & np.uint64(0xFFFF)
    return out.reshape(-1)[:n]


def decisions(n, p, seed, offset):
    """bool [n]: draw >= threshold(p) — the dropout decision of every element, before the activation's sign is known."""
    return draws(n, seed, offset) >= np.uint16(threshold(p))


def relu_dropout(x, p, seed, offset):
    """(y float32, keep bool) of dropout_p(relu(x)) for a float32 array x, flattened in row-major order."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    flat = x.reshape(-1)
    keep = decisions(flat.size, p, seed, offset) & (flat > np.float32(0.0))
    y = np.where(keep, flat * scale32(p), np.float32(0.0)).astype(np.float32)
    return y.reshape(x.shape), keep.reshape(x.shape)


def bits_words(n):
    """The fewest 64-bit words that hold one bit per element of n: four per 64 quads begun."""
    return ((int(n) + 3) // 4 + 63) // 64 * 4


def pack_bits(keep_bool, n, words=None):
    """uint64 [words]: bit t & 63 of word 4 (t >> 6) + j is keep_bool[4t + j]; every other bit 0.  ``words`` defaults to
    bits_words(n); a larger count (a kernel's own buffer size) pads with zero words."""
    n = int(n)
    k = np.asarray(keep_bool, dtype=np.bool_).reshape(-1)
    assert k.size == n
    need = bits_words(n)
    words = need if words is None else int(words)
    assert words >= need
    full = np.zeros(need // 4 * 64 * 4, dtype=np.uint8)
    full[:n] = k
    by_word = full.reshape(need // 4, 64, 4).transpose(0, 2, 1)            # [t >> 6][j][t & 63]
    packed = np.packbits(np.ascontiguousarray(by_word), axis=2, bitorder='little')   # [.., .., 8] bytes, little-endian
    out = np.zeros(words, dtype='<u8')
    out[:need] = packed.reshape(-1).view('<u8')
    return out.astype(np.uint64)


def unpack_bits(words, n):
    """bool [n] from the packed words (the inverse of pack_bits on the bits that belong to an element)."""
    n = int(n)
    need = bits_words(n)
    w = np.ascontiguousarray(np.asarray(words).reshape(-1)[:need]).astype('<u8')
    assert w.size == need
    bits = np.unpackbits(w.view(np.uint8).reshape(need // 4, 4, 8), axis=2, bitorder='little')   # [t >> 6][j][t & 63]
    return bits.transpose(0, 2, 1).reshape(-1)[:n].astype(np.bool_)


def words_stamp(p, seed, offset, n_rows):
    """uint64 [4] = {o, seed, threshold, n_rows}: what dcr_dropout_words_dev leaves behind the decisions it drew."""
    return np.array([int(offset) & _M64, int(seed) & _M64, threshold(p), int(n_rows)], dtype=np.uint64)


def stamp_index(n_rows, hidden):
    """Index of the stamp's first word: ceil(n_rows / RPW) 4, RPW = 64 / (hidden / 4) rows sharing four words."""
    rpw = 64 // (int(hidden) // 4)
    return (int(n_rows) + rpw - 1) // rpw * 4
