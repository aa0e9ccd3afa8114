"""The GCN dropout stream's restatement (tests/dropout_ref.py), the parts that need no GPU: the Philox rounds against the
Random123 known answer, the threshold and its clamp, the bit layout's round trip, and the statistics of the stream — derived
bounds at fixed seeds, so that the bit-for-bit comparison on the GPU (tests/test_dropout_stream_gpu.py) is a comparison with
something that is itself pinned."""
import numpy as np
import pytest

import cheeger_ref
import dropout_ref

SEED, OFFSET = 0x123456789ABCDEF0, 2 ** 40 + 7


def test_philox_known_answers():
    # Random123 kat_vectors, philox4x32 10 rounds: zero counter and key (what tests/test_cheeger_cpu.py pins) ...
    out = cheeger_ref.philox4x32_10(np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(1), 0, 0)
    assert [int(w[0]) for w in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # ... all ones, and the digits of pi: every counter word, both key words and their carries take part
    f = np.full(1, 0xFFFFFFFF, dtype=np.uint64)
    out = cheeger_ref.philox4x32_10(f, f, f, f, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(w[0]) for w in out] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    c = [np.full(1, v, dtype=np.uint64) for v in (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344)]
    out = cheeger_ref.philox4x32_10(*c, 0xA4093822, 0x299F31D0)
    assert [int(w[0]) for w in out] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_draws_are_the_rule_spelled_out_element_by_element():
    """draws() vectorises the rule; here it is one element at a time, with the counter, the half and the word written out."""
    n = 37
    got = dropout_ref.draws(n, SEED, OFFSET)
    assert got.dtype == np.uint16 and got.shape == (n,)
    for e in range(n):
        t, j = divmod(e, 4)
        call = t >> 1
        r = cheeger_ref.philox4x32_10(np.array([call & 0xFFFFFFFF]), np.array([call >> 32]), np.array([OFFSET & 0xFFFFFFFF]),
                                      np.array([OFFSET >> 32]), SEED & 0xFFFFFFFF, SEED >> 32)
        assert int(got[e]) == (int(r[j][0]) >> (16 * (t & 1))) & 0xFFFF, e
    # a prefix of a longer tensor is the same stream; the seed's and the offset's high words both matter
    assert np.array_equal(dropout_ref.draws(1000, SEED, OFFSET)[:n], got)
    assert not np.array_equal(dropout_ref.draws(n, SEED & 0xFFFFFFFF, OFFSET), got)
    assert not np.array_equal(dropout_ref.draws(n, SEED, OFFSET & 0xFFFFFFFF), got)
    assert dropout_ref.stream_offset(2 ** 32 - 1, 3) == 2 ** 32 + 2
    assert dropout_ref.stream_offset(2 ** 64 - 1, 2) == 1
    assert np.array_equal(dropout_ref.decisions(n, 0.3, SEED, OFFSET), got >= 19660)


def test_threshold_and_its_clamp():
    assert dropout_ref.threshold(0.0) == 0
    assert dropout_ref.threshold(0.5) == 32768
    assert dropout_ref.threshold(0.3) == 19660                 # floor(19660.8)
    assert dropout_ref.threshold(2.0 ** -16) == 1
    assert dropout_ref.threshold(1.0 - 2.0 ** -20) == 65535    # floor gives 65535 here; the clamp is not yet at work
    assert dropout_ref.threshold(65535.0 / 65536.0) == 65535
    assert dropout_ref.threshold(np.nextafter(1.0, 0.0)) == 65535
    assert dropout_ref.threshold(1.0) == 65535                 # the clamp: floor gives 65536, which no 16-bit draw reaches
    assert dropout_ref.threshold(np.nextafter(2.0 ** -16, 0.0)) == 0
    # p = 0 keeps every element, whatever it draws; the clamp still keeps a draw of 65535
    assert dropout_ref.decisions(4099, 0.0, SEED, OFFSET).all()
    d = dropout_ref.draws(1 << 20, SEED, OFFSET)
    assert (d == 65535).any()
    assert np.array_equal(dropout_ref.decisions(1 << 20, 1.0 - 2.0 ** -20, SEED, OFFSET), d == 65535)
    assert dropout_ref.scale32(0.5) == np.float32(2.0) and dropout_ref.scale32(1.0 - 2.0 ** -20) == np.float32(2.0 ** 20)
    assert dropout_ref.scale32(0.3) == np.float32(1.0 / 0.7)


@pytest.mark.parametrize('n', [1, 3, 4, 255, 256, 257, 1023, 1025])
def test_pack_unpack_round_trip(n):
    rng = np.random.default_rng(n)
    keep = rng.random(n) < 0.5
    words = dropout_ref.pack_bits(keep, n)
    assert words.dtype == np.uint64 and words.size == dropout_ref.bits_words(n) == ((n + 3) // 4 + 63) // 64 * 4
    assert np.array_equal(dropout_ref.unpack_bits(words, n), keep)
    # the layout, bit by bit: element 4t + j is bit t & 63 of word 4 (t >> 6) + j, and no other bit is set
    want = [0] * words.size
    for e in np.flatnonzero(keep).tolist():
        t, j = divmod(e, 4)
        want[4 * (t >> 6) + j] |= 1 << (t & 63)
    assert [int(w) for w in words] == want
    padded = dropout_ref.pack_bits(keep, n, words=words.size + 12)
    assert np.array_equal(padded[:words.size], words) and not padded[words.size:].any()
    assert np.array_equal(dropout_ref.unpack_bits(padded, n), keep)
    ones = dropout_ref.pack_bits(np.ones(n, dtype=bool), n)
    assert sum(bin(int(w)).count('1') for w in ones) == n


def test_words_stamp():
    s = dropout_ref.words_stamp(0.3, 2 ** 64 - 1, 2 ** 40 + 7, 5003)
    assert s.dtype == np.uint64 and [int(v) for v in s] == [2 ** 40 + 7, 2 ** 64 - 1, 19660, 5003]
    assert dropout_ref.stamp_index(5003, 128) == (5003 + 1) // 2 * 4 and dropout_ref.stamp_index(5003, 64) == (5003 + 3) // 4 * 4
    assert dropout_ref.stamp_index(5003, 128) == dropout_ref.bits_words(5003 * 128)
    assert dropout_ref.stamp_index(5003, 64) == dropout_ref.bits_words(5003 * 64)


def _corr(a, b):
    a = a.astype(np.float64) - a.mean(dtype=np.float64)
    b = b.astype(np.float64) - b.mean(dtype=np.float64)
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize('n,p', [(387129, 0.3), (1 << 24, 0.5), (1000003, 0.999999)])
def test_statistics_of_the_stream(n, p):
    """Derived, not measured: the kept share of n independent decisions of probability q = 1 - threshold / 65536 has standard
    deviation sqrt(q (1 - q) / n); the sample correlation of n independent pairs has standard deviation 1 / sqrt(n).  Five of
    either.  Fixed seeds: the outcome is deterministic, and a case outside 5 sigma is a finding about the design."""
    q = 1.0 - dropout_ref.threshold(p) / 65536.0
    d = dropout_ref.draws(n, SEED, OFFSET)
    keep = dropout_ref.decisions(n, p, SEED, OFFSET)
    assert np.array_equal(keep, d >= dropout_ref.threshold(p))
    sigma = np.sqrt(q * (1.0 - q) / n)
    share = keep.mean(dtype=np.float64)
    print(f'n={n} p={p}: kept share {share:.9f}, q {q:.9f}, {abs(share - q) / sigma:.2f} sigma')
    assert abs(share - q) <= 5.0 * sigma
    # the draws as [call][half][word]: whole calls only
    calls = n // 8
    by_call = d[:calls * 8].reshape(calls, 2, 4)
    pairs = [('low and high half of one word', by_call[:, 0, :].reshape(-1), by_call[:, 1, :].reshape(-1)),
             ('neighbouring words of one call', by_call[:, :, :3].reshape(-1), by_call[:, :, 1:].reshape(-1)),
             ('neighbouring elements', d[:-1], d[1:]),
             ('offsets o and o + 1', d, dropout_ref.draws(n, SEED, OFFSET + 1))]
    for name, a, b in pairs:
        r = _corr(a, b)
        print(f'  {name}: correlation {r:+.3e}, {abs(r) * np.sqrt(a.size):.2f} sigma over {a.size} pairs')
        assert abs(r) <= 5.0 / np.sqrt(a.size), name
