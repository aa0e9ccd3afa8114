"""Plain restatement of the Monte-Carlo Cheeger estimate, for the tests to check the product against.

Written from the definitions only (numpy, networkx and Python's ``random``); nothing here imports
``experiment.compute_cheeger`` or the library (the checker does not live in what it checks).  tests/test_cheeger_cpu.py pins
this file to the recorded outputs of the reference itself (tests/golden/cheeger_reference.json) before anything on the GPU is
judged by it.

For the graph ``to_networkx(data, to_undirected=True)`` builds, ``G.edges`` yields every undirected edge once as (a, b) with
a < b.  For a subset S:  in = #{a in S, b in S}, lo = #{a in S, b not in S}, hi = #{a not in S, b in S}, out = the rest.
  'reference'    lo / min(2 in, 2 out)                      (one-sided boundary over induced volumes)
  'conductance'  (lo + hi) / min(2 in + lo + hi, 2 out + lo + hi)
inf when the smaller volume is zero; the quotient is Python's int / int.
"""
import random

import networkx as nx
import numpy as np


def undirected_edges(edge_index):
    """(a, b) int64 arrays with a < b, each undirected edge once (self-loops dropped: the device graph has none)."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    a, b = np.minimum(ei[0], ei[1]), np.maximum(ei[0], ei[1])
    pairs = np.unique(np.stack([a, b], 1)[a != b], axis=0)
    return pairs[:, 0], pairs[:, 1]


def to_graph(edge_index, num_nodes):
    G = nx.Graph()
    G.add_nodes_from(range(num_nodes))
    G.add_edges_from(zip(*(x.tolist() for x in undirected_edges(edge_index))))
    return G


def counts(edge_index, members):
    """int64 [B, 4] = (in, lo, hi, out) for bool members [B, n]."""
    a, b = undirected_edges(edge_index)
    m = np.asarray(members, dtype=np.bool_)
    out = np.empty((m.shape[0], 4), dtype=np.int64)
    for j in range(m.shape[0]):
        ma, mb = m[j, a], m[j, b]
        out[j] = ((ma & mb).sum(), (ma & ~mb).sum(), (~ma & mb).sum(), (~ma & ~mb).sum())
    return out


def value(c_in, c_lo, c_hi, c_out, definition='reference'):
    c_in, c_lo, c_hi, c_out = int(c_in), int(c_lo), int(c_hi), int(c_out)
    if definition == 'reference':
        cut, m = c_lo, min(2 * c_in, 2 * c_out)
    elif definition == 'conductance':
        cut = c_lo + c_hi
        m = min(2 * c_in + cut, 2 * c_out + cut)
    else:
        raise ValueError(definition)
    return float('inf') if m == 0 else cut / m


def values(cnt, definition='reference'):
    return [value(*row, definition=definition) for row in np.asarray(cnt).tolist()]


def randint_members(count, num_nodes):
    """The subsets of ``count`` draws, nodes visited in ascending order: member iff ``random.randint(0, 1) == 0``."""
    m = np.empty((count, num_nodes), dtype=np.bool_)
    for j in range(count):
        for v in range(num_nodes):
            m[j, v] = random.randint(0, 1) == 0
    return m


def estimate(edge_index, num_nodes, iterations, definition='reference'):
    """(result, all_results) of the estimator from the current state of Python's global stream."""
    vals = values(counts(edge_index, randint_members(iterations, num_nodes)), definition)
    return min(vals, default=float('inf')), vals


def unpack(words, count):
    """bool [count, n] from uint64 words [n, W]."""
    w = np.ascontiguousarray(np.asarray(words, dtype='<u8'))
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder='little')
    return bits[:, :count].T.astype(np.bool_)


# ---- the Philox family as include/dcr.h states it ------------------------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 (Salmon et al., Random123) on uint64 arrays holding 32-bit values; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LOW for c in (c0, c1, c2, c3))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_members(seed, first, count, num_nodes):
    """bool [count, n]: node v is in subset j iff bit (j & 31) of word (j >> 5) & 3 of Philox-4x32-10 with counter
    {v low, v high, (j >> 7) low, (j >> 7) high} and key {seed low, seed high} is set; j = first .. first + count - 1."""
    v = np.arange(num_nodes, dtype=np.uint64)
    m = np.empty((count, num_nodes), dtype=np.bool_)
    cache = {}
    for i in range(count):
        j = first + i
        blk = j >> 7
        if blk not in cache:
            cache = {blk: philox4x32_10(v & _LOW, v >> _S32, np.uint64(blk & 0xFFFFFFFF), np.uint64(blk >> 32),
                                        seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)}
        m[i] = (cache[blk][(j >> 5) & 3] >> np.uint64(j & 31)) & np.uint64(1)
    return m
