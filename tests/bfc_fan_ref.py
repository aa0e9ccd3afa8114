"""Graphs whose Balanced Forman ingredients are known in closed form, for the edge-by-edge pass (csrc/dcr_bfc_nc.hip:
k_nc_fine_edges / nc_edge_wg) and the kernels that share its batches, piece list and queue.  Plain numpy.

A *fan* is one edge {u, v} and three disjoint node sets: C (common neighbours), X (neighbours of u only), Y (neighbours of v
only), a 0/1 matrix M (|Y| x |X|) of y-x edges and, optionally, pads: degree-1 nodes hung on a y, which lengthen its row
without touching X or C.  Then, for the edge (u, v),
    T = |C|,  |sq1| = columns of M with a one,  |sq2| = rows of M with a one,  gamma = max(row sums, column sums)
(0 when either |sq| is 0, as oracle/sdrf_oracle.py: bfc_ingredients gives it), deg u = |X| + |C| + 1, deg v = |Y| + |C| + 1.
Every id is the caller's, so the caller decides the orientation (u < v or u > v), where u sits in the ascending row of v, and
the hash buckets of N(u).

Restated here, each read from or checked against the sources: the closing expression (``bfc_formula``; the CPU test compares
it with the oracle by bits), the bucket of an id in the LDS table (``bucket``), the table the host picks for a degree bound
(``slots_for``), and the layout of the adjacency rows at creation (``layout``), from which ``stream_plan`` derives what the
kernel's second sweep sees of the fan edge: batches of 64 entries of row v, their flat list of aligned 16-byte pieces, the row
of every piece and which streamed ids are looked up.  ``CASES`` is the list the GPU tests run and the CPU test proves."""
import functools
import os
import re

import numpy as np

from conftest import PKG


def _source(name):
    with open(os.path.join(PKG, 'csrc', name)) as f:
        return f.read()


def _int(pattern, text, what):
    m = re.search(pattern, text)
    assert m, what + ' not found'
    return int(m.group(1), 0)


@functools.lru_cache(maxsize=None)
def limits():
    """Constants of the kernels and of the host, as the sources spell them."""
    nc, route, graph = _source('dcr_bfc_nc.hip'), _source('dcr_pass_route.h'), _source('dcr_graph.hip')
    L = {
        'NC_MAXD': _int(r'constexpr\s+int\s+NC_MAXD\s*=\s*(\d+)\s*;', route, 'NC_MAXD'),
        'DIRTY_EDITS': _int(r'constexpr\s+int\s+DIRTY_EDITS\s*=\s*(\d+)\s*;', route, 'DIRTY_EDITS'),
        'NC_Q': _int(r'#define NC_Q (\d+)', nc, 'NC_Q'),
        'NC_QCAP': _int(r'#define NC_QCAP (\d+)', nc, 'NC_QCAP'),
        'NCF_W': _int(r'constexpr int NCF_W = (\d+);', nc, 'NCF_W'),
        'HASH_MUL': _int(r'asm\("v_mul_u32_u24 %0, (0x[0-9a-fA-F]+), %1"', nc, 'hash multiplier'),
    }
    # the bucket rule: BITS = log2(SLOTS / 4), the top BITS bits of the 24-bit product
    assert re.search(r'constexpr int BITS = __builtin_ctz\(SLOTS / 4\);', nc), 'hash_bucket: BITS'
    assert re.search(r'return \(prod >> \(24 - BITS\)\) & \(\(1u << BITS\) - 1\);', nc), 'hash_bucket: shift'
    # the host's table choice, run_nc_fine
    assert re.search(r'const int64_t dmax = g->max_deg_bound < NC_MAXD \? g->max_deg_bound : NC_MAXD;', nc), 'run_nc_fine: dmax'
    m = re.search(r'if \(dmax <= (\d+) / 2 - 2\) DCR_NCF_LAUNCH\((\d+), \d+\);\s*else if \(dmax <= (\d+) / 2 - 2\) DCR_NCF_LAUNCH\((\d+), \d+\);'
                  r'\s*else DCR_NCF_LAUNCH\((\d+), \d+\);', nc)
    assert m and m.group(1) == m.group(2) and m.group(3) == m.group(4), 'run_nc_fine: table choice'
    L['TABLES'] = (int(m.group(1)), int(m.group(3)), int(m.group(5)))
    assert re.search(r'if \(ok && ru\.y > NCF_SLOTS / 2 - 2\)', nc), 'k_nc_fine_edges: half-load rule'
    # rows at creation: capacity = degree + slack_for(degree), laid out in node order
    m = re.search(r'slack_for\(int32_t deg\) \{\s*int32_t s = deg / (\d+);\s*return s < (\d+) \? (\d+) : s;', graph)
    assert m and m.group(2) == m.group(3), 'slack_for'
    L['SLACK_DIV'], L['SLACK_MIN'] = int(m.group(1)), int(m.group(2))
    assert re.search(r'cap\[\(size_t\)u\] = deg\[\(size_t\)u\] \+ slack_for\(deg\[\(size_t\)u\]\);', graph), 'dcr_graph_create: capacity'
    return L


def bfc_formula(d1, d2, T, s1, s2, gamma):
    """The closing expression in float64, left to right (oracle/sdrf_oracle.py: bfc_formula, bfc_naive.py:31-40; an edge with an
    endpoint of degree 1 never gets here: it is 0.0 by bfc_naive.py:18-19)."""
    d1, d2, T, s1, s2, gamma = (int(t) for t in (d1, d2, T, s1, s2, gamma))
    dmax, dmin = max(d1, d2), min(d1, d2)
    r = 2 / d1 + 2 / d2 - 2 + 2 * T / dmax + T / dmin
    if s1 == 0 or s2 == 0:
        return r
    return r + 1 / gamma / dmax * (s1 + s2)


def bits(x):
    return int(np.float64(x).view(np.int64))


def bucket(ids, slots):
    """Home bucket of an id in a table of ``slots`` slots (4 per bucket): ((id & 0xFFFFFF) * 0x9E3779 & 0xFFFFFF) >> (24 - BITS)."""
    nb = slots // 4
    b = nb.bit_length() - 1
    assert 1 << b == nb
    ids = np.asarray(ids, dtype=np.uint64)
    return ((((ids & np.uint64(0xFFFFFF)) * np.uint64(limits()['HASH_MUL'])) & np.uint64(0xFFFFFF)) >> np.uint64(24 - b)).astype(np.int64)


def table_fill(keys, slots):
    """Keys per bucket once ``keys`` are in a table of ``slots`` slots, and whether any left its home bucket.  (A key goes to the
    first bucket at or behind its home with a free slot; how many each bucket ends up with does not depend on the order.)"""
    nb = slots // 4
    count = np.zeros(nb, dtype=np.int64)
    spilled = False
    for h in bucket(keys, slots).tolist():
        while count[h] == 4:
            h, spilled = (h + 1) % nb, True
        count[h] += 1
    return count, spilled


def slots_for(bound):
    """The table run_nc_fine picks for the host's bound on the largest degree."""
    L = limits()
    dmax = min(int(bound), L['NC_MAXD'])
    for slots in L['TABLES'][:-1]:
        if dmax <= slots // 2 - 2:
            return slots
    return L['TABLES'][-1]


def coalesce(src, dst, n):
    """Symmetric, without duplicates, sorted by (row, column): the rows of a new graph are ascending by id."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    assert np.all(src != dst)
    key = np.unique(np.concatenate([src, dst]) * np.int64(n) + np.concatenate([dst, src]))
    return np.stack([key // n, key % n]).astype(np.int64)


def fan(u, v, X, C, Y, M, pads=None, n=None):
    """(edge_index, n, u, v, expected6) of the fan.  ``pads``: {index into Y: a count of fresh ids, or the ids}; fresh ids
    start behind the largest id in use.  ``expected6`` = (deg u, deg v, T, |sq1|, |sq2|, gamma) of the edge (u, v)."""
    X, C, Y = [int(t) for t in X], [int(t) for t in C], [int(t) for t in Y]
    M = np.asarray(M).astype(bool).reshape(len(Y), len(X))
    pads = dict(pads or {})
    used = {int(u), int(v)} | set(X) | set(C) | set(Y)
    assert len(used) == 2 + len(X) + len(C) + len(Y), 'u, v, X, C and Y must be disjoint'
    given = [int(t) for p in pads.values() if not isinstance(p, (int, np.integer)) for t in p]
    assert len(set(given)) == len(given) and not set(given) & used, 'pad ids must be fresh'
    fresh = max(used | set(given)) + 1
    src, dst = [u] + [u] * (len(X) + len(C)) + [v] * (len(C) + len(Y)), [v] + X + C + C + Y
    yi, xi = np.nonzero(M)
    src += [Y[i] for i in yi]
    dst += [X[j] for j in xi]
    for i, p in sorted(pads.items()):
        if isinstance(p, (int, np.integer)):
            p = list(range(fresh, fresh + int(p)))
            fresh += len(p)
        src += [Y[i]] * len(p)
        dst += [int(t) for t in p]
    top = max(max(src), max(dst)) + 1
    n = top if n is None else int(n)
    assert n >= top
    col, row = M.sum(0), M.sum(1)
    s1, s2 = int((col > 0).sum()), int((row > 0).sum())
    gamma = int(max(col.max(), row.max())) if s1 and s2 else 0
    expected6 = (len(X) + len(C) + 1, len(Y) + len(C) + 1, len(C), s1, s2, gamma)
    return coalesce(src, dst, n), n, int(u), int(v), expected6


def with_leaf(expected6, leaves=1):
    """expected6 once ``leaves`` fresh degree-1 nodes hang on u: only deg u moves."""
    return (expected6[0] + leaves,) + tuple(expected6[1:])


# ---------------------------------------------------------------------------------------------- what the kernel sees of a fan
def layout(ei, n):
    """(start, degree) of every row as dcr_graph_create lays them out."""
    L = limits()
    deg = np.bincount(ei[0], minlength=n).astype(np.int64)
    cap = deg + np.maximum(L['SLACK_MIN'], deg // L['SLACK_DIV'])
    return np.cumsum(cap) - cap, deg


def _rows(ei, n):
    ptr = np.searchsorted(ei[0], np.arange(n + 1))
    return lambda k: ei[1][ptr[k]:ptr[k + 1]]


def stream_plan(ei, n, u, v):
    """Sweep 2 of nc_edge_wg for the edge (u, v) on the graph as created (an edge added at u later moves nothing here: row v
    and the rows of its members stay where they are, and the new leaf is no neighbour of any of them).  One dict per batch of
    64 entries of row v: ``wave`` (which of the NCF_W waves takes it), ``pos`` of its first entry, ``lane_of`` (the batch lane of
    every piece: the row of the piece), ``hit`` (pieces x 4: entry inside its row, in N(u) and not v: a full look-up) and
    ``starts`` (row starts of the streamed rows)."""
    start, deg = layout(ei, n)
    row = _rows(ei, n)
    nu = set(row(u).tolist())
    rowv = row(v)
    W = limits()['NCF_W']
    out = []
    for base in range(0, len(rowv), 64):
        lane_of, hit, starts = [], [], []
        for lane, k in enumerate(rowv[base:base + 64].tolist()):
            if k == u or k in nu or deg[k] == 0:
                continue
            x, y = int(start[k]), int(deg[k])
            ids = row(k)
            starts.append(x)
            for p in range(((x + y + 3) >> 2) - (x >> 2)):
                a = (x & ~3) + 4 * p
                lane_of.append(lane)
                hit.append([x <= a + t < x + y and int(ids[a + t - x]) in nu and int(ids[a + t - x]) != v for t in range(4)])
        out.append({'wave': (base // 64) % W, 'pos': base, 'lane_of': np.array(lane_of, dtype=np.int64),
                    'hit': np.array(hit, dtype=bool).reshape(len(lane_of), 4), 'starts': starts})
    return out


def reach(ei, n, u, v):
    """Facts about the fan edge's pass that the case list claims (tests/test_bfc_fan_ref_cpu.py asserts them per case)."""
    L = limits()
    plan = stream_plan(ei, n, u, v)
    spans, full_positions = [], 0
    for b in plan:
        P = len(b['lane_of'])
        for j0 in range(0, P, 64):
            jl = min(j0 + 63, P - 1)
            spans.append(int(b['lane_of'][jl] - b['lane_of'][j0]))                 # piece_row: rl - rf
            if jl - j0 == 63:
                full_positions += int(b['hit'][j0:j0 + 64].all(axis=0).sum())      # an entry position that hits in all 64 lanes
    rowv = _rows(ei, n)(v)
    posu = int(np.flatnonzero(rowv == u)[0])
    return {
        'deg_v': len(rowv),
        'posu': posu,
        'posu_wave': (posu // 64) % L['NCF_W'],
        'pieces': max(len(b['lane_of']) for b in plan),                              # of the largest batch
        'spans': spans,
        'lookups': max(int(b['hit'].sum()) for b in plan),                           # of the largest batch: queue items
        'full_positions': full_positions,
        'full_piece': any(bool(b['hit'].all(axis=1).any()) for b in plan),
        'unaligned_start': any(x % 4 for b in plan for x in b['starts']),
        'waves': sorted({b['wave'] for b in plan if len(b['lane_of'])}),
    }


# ---------------------------------------------------------------------------------------------- the cases
class Pool:
    """Fresh ids in ascending order, skipping the reserved ones."""

    def __init__(self, reserved=(), first=0):
        self.reserved, self.next = set(int(t) for t in reserved), first

    def take(self, k):
        out = []
        while len(out) < k:
            if self.next not in self.reserved:
                out.append(self.next)
            self.next += 1
        return out


def _sparse(ny, nx):
    """Every y has an x or two, no x more than a few y: hits in every batch, nothing dense."""
    M = np.zeros((ny, nx), dtype=bool)
    i = np.arange(ny)
    M[i, (7 * i) % nx] = True
    M[i[::3], (3 * i[::3] + 1) % nx] = True
    return M


def _plain(du, dv, nc=3, M=None, pads=None):
    """u = 0 < v = 1, then C, Y, X in ascending blocks of ids; deg u = du, deg v = dv."""
    P = Pool(first=2)
    C, Y, X = P.take(nc), P.take(dv - 1 - nc), P.take(du - 1 - nc)
    return fan(0, 1, X, C, Y, _sparse(len(Y), len(X)) if M is None else M(len(Y), len(X)), pads)


def _placed(dv, where, u_above_v, extra=4):
    """deg v = dv with u at position ``where`` of the ascending row of v (0, dv - 1 or 256); deg u = dv + extra."""
    nc = 3
    pos = {'first': 0, 'last': dv - 1, 'at256': 256}[where]
    assert 0 <= pos < dv
    P = Pool(first=1 if u_above_v else 0)
    low = P.take(pos)
    u = P.take(1)[0]
    others = low + P.take(dv - 1 - pos)
    v = 0 if u_above_v else P.take(1)[0]
    C = others[::max(1, len(others) // nc)][:nc]                                    # spread over the batches of row v
    Y = [k for k in others if k not in C]
    X = P.take(dv + extra - 1 - nc)
    return fan(u, v, X, C, Y, _sparse(len(Y), len(X)))


def _pieces_many():
    """160 rows of Y of 16-20 entries: a batch of 64 of them has more than 64 * NC_Q pieces."""
    def M(ny, nx):
        out = np.zeros((ny, nx), dtype=bool)
        for i in range(ny):
            out[i, [(5 * i + 11 * t) % nx for t in range(3)]] = True
        return out
    return _plain(200, 164, M=M, pads={i: 12 + i % 5 for i in range(160)})          # row = v + 3 x + 12..16 pads


def _pieces_short():
    """160 rows of Y of one or two entries: dozens of row starts inside one step of 64 pieces."""
    def M(ny, nx):
        out = np.zeros((ny, nx), dtype=bool)
        out[np.arange(0, ny, 2), np.arange(0, ny, 2) % nx] = True
        return out
    return _plain(200, 164, M=M)


def _pieces_long():
    """Three rows of Y of 300 entries and more: a step of 64 pieces crosses at most a few row starts."""
    return _plain(450, 7, M=lambda ny, nx: np.eye(ny, nx, dtype=bool), pads={0: 300, 1: 333, 2: 410})


def _queue_dense():
    """160 rows of Y with 8 ones each: 512 look-ups in a batch of 64 rows."""
    def M(ny, nx):
        out = np.zeros((ny, nx), dtype=bool)
        for i in range(ny):
            out[i, [(3 * i + 29 * t) % nx for t in range(8)]] = True
        return out
    return _plain(260, 164, M=M)


def _queue_full_pieces():
    """Two rows of Y made of neighbours of u only (700 and 350 of them): whole steps of 64 pieces with four hits each."""
    def M(ny, nx):
        out = np.zeros((ny, nx), dtype=bool)
        out[0, :700] = True
        out[1, 100:450] = True
        out[2, 7] = True
        return out
    return _plain(760, 7, M=M)


def _gamma_600():
    """|Y| = 600 and one column of M all ones: gamma = 600.  That x shares its home bucket (4,096 slots) with one common
    neighbour and with no other key, so the two sit in one word of the slot state: a counter at 600 next to a flagged half."""
    du, dv, slots = 640, 604, 4096
    assert slots_for(du + 1) == slots
    b = bucket(np.arange(3000), slots)
    count = np.bincount(b, minlength=slots // 4)
    home = next(h for h in range(1, slots // 4) if count[h] >= 2 and count[h - 1] <= 2)
    x0, c0 = (int(t) for t in np.flatnonzero(b == home)[:2])
    others = [int(t) for t in np.flatnonzero(b == home)[2:]] + [int(t) for t in np.flatnonzero(b == home - 1)]
    P = Pool(reserved=[x0, c0] + others, first=0)                                  # nothing else of N(u) in or before that bucket
    u, v = P.take(2)
    C, Y = [c0] + P.take(2), P.take(dv - 4)
    X = [x0] + P.take(du - 5)
    M = _sparse(len(Y), len(X))
    M[:, 0] = True
    return fan(u, v, X, C, Y, M)


def _spill(slots, du, n_ids=65536):
    """Eleven ids of the LAST bucket of the table: six of X, the three smallest and the three largest, and two of C between
    them, so that at least four keys leave the bucket, the chain wraps into bucket 0 (which holds keys of its own) and, whatever
    the order of insertion, two or more of the spilled keys are x with ones in M: hits that only the walk finds.  The other three
    are non-neighbours of u hung on rows of Y: candidates the fast test lets through and nc_find must reject.  Bucket 0 gets
    three x, a common neighbour and two such non-neighbours as well."""
    assert slots_for(du + 1) == slots
    b = bucket(np.arange(n_ids), slots)
    last = [int(t) for t in np.flatnonzero(b == slots // 4 - 1)[:11]]
    zero = [int(t) for t in np.flatnonzero(b == 0)[1:7]]                            # (id 0 itself hashes to bucket 0: left out)
    assert len(last) == 11 and len(zero) == 6
    P = Pool(reserved=last + zero, first=0)
    u, v = P.take(2)
    nc, ny, special = 4, 50, last[0:3] + last[5:8] + zero[:3]
    C = last[3:5] + zero[3:4] + P.take(nc - 3)
    Y = P.take(ny)
    X = special + P.take(du - 1 - nc - len(special))
    M = _sparse(len(Y), len(X))
    for j in range(len(special)):                                                  # the x of the full buckets: 1 + j ones each
        M[:, j] = False
        M[5 * j:5 * j + 1 + j, j] = True
    pads = {0: last[8:10], 1: last[10:11] + zero[4:5], 2: zero[5:6]}
    return fan(u, v, X, C, Y, M, pads)


def _nc_maxd():
    return _plain(limits()['NC_MAXD'] - 1, 70)


# name -> builder.  Every case is checked at deg u + 1 (one leaf added to u): the table cases name that degree.
CASES = {
    'table_510': lambda: _plain(509, 70),
    'table_2046': lambda: _plain(2045, 70),
    'table_nc_maxd': _nc_maxd,
    'pieces_many': _pieces_many,
    'pieces_short': _pieces_short,
    'pieces_long': _pieces_long,
    'queue_dense': _queue_dense,
    'queue_full_pieces': _queue_full_pieces,
    'gamma_600': _gamma_600,
    'spill_1024': lambda: _spill(1024, 300),
    'spill_4096': lambda: _spill(4096, 1200),
    'spill_16384': lambda: _spill(16384, 2100),
}
ROW_DEGREES = (63, 64, 65, 256, 257, 513)
for _dv in ROW_DEGREES:
    for _where in ('first', 'last') + (('at256',) if _dv > 257 else ()):          # (257: position 256 is the last)
        CASES['row_%d_%s_above' % (_dv, _where)] = functools.partial(_placed, _dv, _where, True)
# the other orientation (the slot is in u's own row: posu is found and not used), every position and every degree once
for _dv, _where in ((63, 'last'), (64, 'first'), (65, 'last'), (256, 'first'), (257, 'last'), (513, 'at256')):
    CASES['row_%d_%s_below' % (_dv, _where)] = functools.partial(_placed, _dv, _where, False)


@functools.lru_cache(maxsize=None)
def case(name):
    """The fan of a case, built once; nobody writes to its arrays."""
    return CASES[name]()
