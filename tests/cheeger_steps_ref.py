"""Host restatement of the Cheeger count kernels' steps (csrc/dcr_cheeger.hip), numpy only, for the tests of their limits.

Four pieces, each written from the source it restates and pinned by tests/test_cheeger_steps_cpu.py before anything on the
GPU is judged by it:
  * the constants, read from the source text (a silent change there fails an assertion instead of moving a test off its limit);
  * ``geometry``: the integer arithmetic of ``launch_sliced`` and of the lane launch in ``cheeger_run``;
  * ``slot_layout``: the adjacency slots of a freshly created graph (``dcr_graph_create`` in csrc/dcr_graph.hip);
  * ``sliced_replica``: ``k_cheeger_sliced`` lane by lane in uint64, with keyword arguments that plant faults in it;
and one independent reference that does not walk the graph at all:
  * ``palette_counts``: when every node's membership row is one of K rows, the counts of a subset are a K x K table of edge
    counts weighted by the subset's bits of the K rows.  K * K * B operations whatever the graph's size.
"""
import os
import re
from collections import namedtuple

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'discrete-curvature-rewiring_amd', 'csrc')


def _source(name='dcr_cheeger.hip'):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _need(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f'{what} not found in the source'
    return m


def _constants():
    src = _source()
    m = _need(r'constexpr\s+int\s+CH_LOW\s*=\s*(\d+)\s*,\s*CH_HIGH\s*=\s*(\d+)\s*,\s*CH_RUN\s*=\s*(\d+)\s*;', src, 'CH_LOW / CH_HIGH / CH_RUN')
    low, high, run = (int(x) for x in m.groups())
    _need(r'constexpr\s+int\s+CH_MAX_ROUNDS\s*=\s*\(\(1\s*<<\s*CH_HIGH\)\s*-\s*1\)\s*/\s*CH_RUN\s*;', src, 'CH_MAX_ROUNDS = ((1 << CH_HIGH) - 1) / CH_RUN')
    max_words = int(_need(r'constexpr\s+int64_t\s+CHEEGER_MAX_WORDS\s*=\s*(\d+)\s*;', src, 'CHEEGER_MAX_WORDS').group(1))
    # launch_sliced: rounds = cap_total * groups / (per_round * PER_CU * (num_cu or CU_DEFAULT)) + 1, at least MIN_ROUNDS
    m = _need(r'int64_t rounds = \(g->cap_total \* groups\) / \(per_round \* (\d+) \* \(g->num_cu > 0 \? g->num_cu : (\d+)\)\) \+ 1;\s*'
              r'if \(rounds < (\d+)\) rounds = (\d+);\s*if \(rounds > CH_MAX_ROUNDS\) rounds = CH_MAX_ROUNDS;', src, 'the rounds rule of launch_sliced')
    per_cu, cu_default, min_a, min_b = (int(x) for x in m.groups())
    assert min_a == min_b
    _need(r'const int64_t per_round = \(int64_t\)\(256 / WL\) \* CH_RUN;\s*const int groups = \(W \+ WL - 1\) / WL;', src, 'per_round / groups')
    _need(r'const int64_t chunk = per_round \* rounds;\s*const unsigned gx = \(unsigned\)\(\(g->cap_total \+ chunk - 1\) / chunk\);', src, 'chunk / gx')
    # cheeger_run: the ladder of WL, first condition that holds
    body = src[src.index('static int cheeger_run('):]
    body = body[:body.index('\nstatic int cheeger_draw(')]
    ladder = [(op, int(k), int(wl)) for op, k, wl in re.findall(r'else if \(W (>=|>|==) (\d+)\) \{\s*launch_sliced<(\d+)>\(g, W\);', body)]
    last = _need(r'\} else \{\s*launch_sliced<(\d+)>\(g, W\);\s*\}', body, 'the last rung of the WL ladder')
    ladder.append((None, 0, int(last.group(1))))
    assert len(re.findall(r'launch_sliced<\d+>', body)) == len(ladder), 'a rung of the WL ladder was not understood'
    # the lane launch: per = cap_total * W / (DIV * (num_cu or CU_DEFAULT)) + 1, rounded up to ROUND, at least MIN
    m = _need(r'int64_t per = g->cap_total \* W / \((\d+) \* \(g->num_cu > 0 \? g->num_cu : (\d+)\)\) \+ 1;\s*'
              r'per = \(per \+ (\d+)\) / (\d+) \* (\d+);\s*if \(per < (\d+)\) per = (\d+);\s*'
              r'const unsigned gx = \(unsigned\)\(\(g->cap_total \+ per - 1\) / per\);', body, 'the per rule of the lane launch')
    div, cu_lane, r1, r2, r3, pmin_a, pmin_b = (int(x) for x in m.groups())
    assert r1 + 1 == r2 == r3 and pmin_a == pmin_b and cu_lane == cu_default
    return dict(CH_LOW=low, CH_HIGH=high, CH_RUN=run, CH_MAX_ROUNDS=((1 << high) - 1) // run, CHEEGER_MAX_WORDS=max_words,
                WG_PER_CU=per_cu, CU_DEFAULT=cu_default, MIN_ROUNDS=min_a, WL_LADDER=tuple(ladder),
                LANE_DIV=div, LANE_ROUND=r2, LANE_MIN=pmin_a)


CONSTANTS = _constants()
CH_LOW, CH_HIGH, CH_RUN = CONSTANTS['CH_LOW'], CONSTANTS['CH_HIGH'], CONSTANTS['CH_RUN']
CH_MAX_ROUNDS, CHEEGER_MAX_WORDS = CONSTANTS['CH_MAX_ROUNDS'], CONSTANTS['CHEEGER_MAX_WORDS']
WL_LADDER = CONSTANTS['WL_LADDER']


def slack_for(deg):
    """``slack_for`` of csrc/dcr_graph.hip, read from its text: max(8, deg / 4)."""
    m = _need(r'static inline int32_t slack_for\(int32_t deg\) \{\s*int32_t s = deg / (\d+);\s*return s < (\d+) \? (\d+) : s;', _source('dcr_graph.hip'),
              'slack_for')
    q, a, b = (int(x) for x in m.groups())
    assert a == b
    return np.maximum(np.asarray(deg) // q, a)


def word_lanes(W):
    """WL of ``cheeger_run`` for W words."""
    for op, k, wl in WL_LADDER:
        if op is None or (op == '>=' and W >= k) or (op == '>' and W > k) or (op == '==' and W == k):
            return wl
    raise AssertionError('unreachable')


Geometry = namedtuple('Geometry', ['sliced', 'lane'])   # sliced = (WL, groups, rounds, chunk, grid_x), lane = (per, grid_x)


def geometry(cap_total, W, num_cu, max_rounds=None):
    """The launch geometry of both shapes for ``cap_total`` slots and W words; ``num_cu`` <= 0 is a handle that has not asked
    the device yet.  ``max_rounds`` replaces the clamp (a planted fault)."""
    cap_total, W = int(cap_total), int(W)
    cus = int(num_cu) if num_cu > 0 else CONSTANTS['CU_DEFAULT']
    WL = word_lanes(W)
    per_round = (256 // WL) * CH_RUN
    groups = (W + WL - 1) // WL
    rounds = (cap_total * groups) // (per_round * CONSTANTS['WG_PER_CU'] * cus) + 1
    rounds = max(rounds, CONSTANTS['MIN_ROUNDS'])
    rounds = min(rounds, CH_MAX_ROUNDS if max_rounds is None else max_rounds)
    chunk = per_round * rounds
    per = cap_total * W // (CONSTANTS['LANE_DIV'] * cus) + 1
    per = (per + CONSTANTS['LANE_ROUND'] - 1) // CONSTANTS['LANE_ROUND'] * CONSTANTS['LANE_ROUND']
    per = max(per, CONSTANTS['LANE_MIN'])
    return Geometry((WL, groups, rounds, chunk, (cap_total + chunk - 1) // chunk), (per, (cap_total + per - 1) // per))


Layout = namedtuple('Layout', ['rowinfo', 'col', 'slot_row', 'cap_total'])   # rowinfo int32 [n, 2] = (start, degree)


def slot_layout(edge_index, n):
    """The adjacency slots ``dcr_graph_create`` uploads: the pairs (src, dst) with dst < src are kept in order (the first of
    each undirected pair when the input is not strictly sorted), each appends dst to src's row and src to dst's row, a row
    of ``deg`` neighbours has ``deg + max(8, deg / 4)`` slots, the rows follow each other in node order, free slots hold -1."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    src, dst = ei[0], ei[1]
    assert ((src >= 0) & (dst >= 0) & (src < n) & (dst < n) & (src != dst)).all()
    keep = np.flatnonzero(dst < src)
    key = src * np.int64(n) + dst
    if not (np.diff(key) > 0).all():                       # not strictly sorted: duplicates may occur, the first one counts
        _, first = np.unique(key[keep], return_index=True)
        keep = keep[np.sort(first)]
    u, v = src[keep], dst[keep]
    deg = np.bincount(np.concatenate([u, v]), minlength=n).astype(np.int64)
    cap = deg + slack_for(deg)
    start = np.concatenate([[0], np.cumsum(cap)[:-1]]) if n else np.zeros(0, dtype=np.int64)
    cap_total = int(cap.sum())
    assert cap_total <= 2 ** 31 - 1
    rows = np.stack([u, v], 1).ravel()                     # the order of the appends: edge by edge, src's row then dst's
    vals = np.stack([v, u], 1).ravel()
    order = np.argsort(rows, kind='stable')
    rows, vals = rows[order], vals[order]
    within = np.arange(rows.shape[0]) - np.repeat(np.concatenate([[0], np.cumsum(deg)[:-1]]) if n else [], deg)
    col = np.full(cap_total, -1, dtype=np.int32)
    col[start[rows] + within] = vals
    slot_row = np.repeat(np.arange(n, dtype=np.int32), cap)
    return Layout(np.stack([start, deg], 1).astype(np.int32), col, slot_row, cap_total)


_ONE = np.uint64(1)


def _planes_add1(L, x):
    """``planes_add1``: L += x, x one bit per counter (L is [CH_LOW, lanes]; written for CH_LOW planes as the kernel's is for 3)."""
    for p in range(CH_LOW - 1):
        t = L[p] & x
        L[p] ^= x
        x = t
    L[CH_LOW - 1] ^= x


def _planes_fold(H, L, drop_carry):
    """``planes_fold``: H += L, L = 0; a carry out of the top plane of H is lost, as in the kernel."""
    carry = np.zeros_like(L[0])
    for p in range(CH_LOW):
        a, b = H[p].copy(), L[p].copy()
        s = a ^ b
        H[p] = s ^ carry
        carry = (a & b) | (s & carry)
        L[p] = 0
    if drop_carry:
        carry = np.zeros_like(carry)
    for p in range(CH_LOW, H.shape[0]):
        t = H[p] & carry
        H[p] ^= carry
        carry = t


def sliced_replica(layout, words, W, geom, *, planes_high=CH_HIGH, max_rounds=None, drop_carry=False, planes_read=CH_HIGH,
                   workgroups=None, num_cu=0):
    """int64 [64 W, 3] = (in, lo, hi): what the workgroups ``workgroups`` (pairs (blockIdx.x, blockIdx.y); None = all) of
    ``k_cheeger_sliced<WL>`` add to the totals, replayed with one numpy element per thread of the workgroup.

    ``geom`` is ``geometry(...)`` or its ``sliced`` tuple.  The faults: ``planes_high`` planes in the high counter instead of
    CH_HIGH; ``max_rounds`` a different clamp in the launcher (the geometry is taken again with it, for ``num_cu``);
    ``drop_carry`` loses the carry out of plane CH_LOW - 1 in ``planes_fold``; ``planes_read`` planes are turned into integers."""
    if max_rounds is not None:
        geom = geometry(layout.cap_total, W, num_cu, max_rounds=max_rounds)
    WL, groups, rounds, chunk, grid_x = geom.sliced if isinstance(geom, Geometry) else geom
    words = np.asarray(words, dtype=np.uint64)
    assert words.ndim == 2 and words.shape[1] == W
    NS = 256 // WL
    assert chunk == NS * CH_RUN * rounds
    rowinfo, col, slot_row, cap_total = layout
    t = np.arange(256)
    wsub, stream = t & (WL - 1), t // WL
    counts = np.zeros((3, 64 * W), dtype=np.int64)
    if workgroups is None:
        workgroups = [(bx, by) for by in range(groups) for bx in range(grid_x)]
    for bx, by in workgroups:
        assert 0 <= bx < grid_x and 0 <= by < groups
        w = by * WL + wsub
        active = w < W
        wc = np.where(active, w, 0)
        s_begin = bx * NS * CH_RUN * rounds
        L = np.zeros((3, CH_LOW, 256), dtype=np.uint64)
        H = np.zeros((3, planes_high, 256), dtype=np.uint64)
        for r in range(rounds):
            s_run = s_begin + r * CH_RUN * NS + stream
            if s_begin + r * CH_RUN * NS >= cap_total:
                break
            for i in range(CH_RUN):
                s = s_run + i * NS
                ok = active & (s < cap_total)
                sc = np.where(ok, s, 0)
                u = np.where(ok, slot_row[sc], 0)
                v = np.where(ok, col[sc], -1)
                ok = ok & ((s - rowinfo[u, 0]) < rowinfo[u, 1]) & (v > u)
                mu = np.where(ok, words[u, wc], np.uint64(0))
                mv = np.where(ok, words[np.where(ok, v, 0), wc], np.uint64(0))
                _planes_add1(L[0], mu & mv)
                _planes_add1(L[1], mu & ~mv)
                _planes_add1(L[2], ~mu & mv)
            for c in range(3):
                _planes_fold(H[c], L[c], drop_carry)
        # planes -> integers: the counter of (thread, bit) is the sum over the planes read of its bit << p; the counters of the
        # NS streams of a word are added (uint32, as cnt[] in the kernel) and go to the totals of that word
        for c in range(3):
            cnt = np.zeros((256, 64), dtype=np.uint32)
            for p in range(min(planes_read, planes_high)):
                bits = np.unpackbits(H[c, p].astype('<u8').view(np.uint8).reshape(256, 8), axis=1, bitorder='little')
                cnt += bits.astype(np.uint32) << np.uint32(p)
            per_word = cnt.reshape(NS, WL, 64).sum(axis=0, dtype=np.uint32)
            for ow in range(WL):
                wo = by * WL + ow
                if wo < W:
                    counts[c, 64 * wo:64 * wo + 64] += per_word[ow]
    return np.ascontiguousarray(counts.T)


def palette_members(node_palette, palette_words):
    """uint64 [n, W]: node v's row is row ``node_palette[v]`` of ``palette_words`` [K, W]."""
    return np.ascontiguousarray(np.asarray(palette_words, dtype=np.uint64)[np.asarray(node_palette)])


def palette_counts(edge_index, n, node_palette, palette_words, block_words=2048):
    """int64 [64 W, 4] = (in, lo, hi, out) of the subsets ``palette_members`` packs.

    c[p][q] = number of undirected edges a < b with a in class p and b in class q, from the edge list once.  With
    x_p = bit j of palette row p:  in[j] = sum c[p][q] x_p x_q,  lo[j] = sum c[p][q] x_p (1 - x_q),
    hi[j] = sum c[p][q] (1 - x_p) x_q,  out = E - in - lo - hi: all int64, the inner sums over q (over p for hi) as matrix
    products of c with the bit rows."""
    pal = np.asarray(node_palette, dtype=np.int64)
    pw = np.asarray(palette_words, dtype=np.uint64)
    K, W = pw.shape
    assert pal.shape == (n,) and K <= 8 and pal.min(initial=0) >= 0 and pal.max(initial=0) < K
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    lo_end, hi_end = np.minimum(ei[0], ei[1]), np.maximum(ei[0], ei[1])
    key = np.unique((lo_end * np.int64(n) + hi_end)[lo_end != hi_end])   # every undirected edge once, self-loops dropped
    a, b = key // n, key % n
    c = np.bincount(pal[a] * K + pal[b], minlength=K * K).reshape(K, K).astype(np.int64)
    out = np.empty((64 * W, 4), dtype=np.int64)
    for w0 in range(0, W, block_words):
        blk = np.ascontiguousarray(pw[:, w0:w0 + block_words]).astype('<u8')
        x = np.unpackbits(blk.view(np.uint8).reshape(K, -1), axis=1, bitorder='little').astype(np.int64)   # [K, bits]
        cx, ctx = c @ x, c.T @ x                     # cx[p] = sum_q c[p][q] x_q;  ctx[q] = sum_p c[p][q] x_p
        n_in = (x * cx).sum(axis=0)
        sl = slice(64 * w0, 64 * w0 + x.shape[1])
        out[sl, 0] = n_in
        out[sl, 1] = (x * c.sum(axis=1)[:, None]).sum(axis=0) - n_in
        out[sl, 2] = (x * c.sum(axis=0)[:, None]).sum(axis=0) - (x * ctx).sum(axis=0)
    out[:, 3] = a.shape[0] - out[:, :3].sum(axis=1)
    return out


# ---- the clamp graph ------------------------------------------------------------------------------------------------------
CLAMP_HUBS, CLAMP_LEAVES, CLAMP_W = 32, 16640, 200
CLAMP_N = CLAMP_HUBS + CLAMP_LEAVES


def clamp_graph():
    """(edge_index, n): complete bipartite, hubs 0..31 first, leaves 32..16671; 532,480 edges.  A hub's row is its 16,640
    leaves in ascending order (every one a slot with col > row) and 4,160 free slots; a leaf's row is the 32 hubs and 8 free
    slots: 32 * 20,800 + 16,640 * 40 = 1,331,200 slots, which at W = 200 asks for 151 runs per lane: the clamp holds it at 146."""
    hubs = np.repeat(np.arange(CLAMP_HUBS, dtype=np.int64), CLAMP_LEAVES)
    leaves = np.tile(np.arange(CLAMP_HUBS, CLAMP_N, dtype=np.int64), CLAMP_HUBS)
    key = np.sort(np.concatenate([hubs * CLAMP_N + leaves, leaves * CLAMP_N + hubs]))
    return np.stack([key // CLAMP_N, key % CLAMP_N]), CLAMP_N


def clamp_palette(W, seed=2024):
    """(node_palette int64 [n], palette_words uint64 [8, W]).  Rows: all ones, all zeros, 0xAAAA..., 0x5555..., four random.
    Hub 0 has row 2 (inside the odd subsets of every word, outside the even ones).  The k-th leaf sits in slot k of every
    hub's row; the sliced kernel's workgroup 0 at WL = 16 gives slot k to stream k % 16.  Stream 0's leaves have row 0 (all
    inside: ``in`` saturates in the odd subsets, ``hi`` in the even ones), stream 1's row 1 (all outside: ``lo`` saturates in
    the odd subsets), stream 2's and 3's rows 3 and 2, and the leaves of the other streams and the other hubs any of the eight."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pw = np.empty((8, W), dtype=np.uint64)
    pw[0], pw[1] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)
    pw[2], pw[3] = np.uint64(0xAAAAAAAAAAAAAAAA), np.uint64(0x5555555555555555)
    pw[4:] = rng.integers(0, 2 ** 64, size=(4, W), dtype=np.uint64)
    pal = np.empty(CLAMP_N, dtype=np.int64)
    pal[:CLAMP_HUBS] = rng.integers(0, 8, size=CLAMP_HUBS)
    pal[0] = 2
    k = np.arange(CLAMP_LEAVES)
    leaf = rng.integers(0, 8, size=CLAMP_LEAVES)
    for stream, row in ((0, 0), (1, 1), (2, 3), (3, 2)):
        leaf[k % 16 == stream] = row
    pal[CLAMP_HUBS:] = leaf
    return pal, pw
