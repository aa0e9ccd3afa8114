"""Graphs whose Balanced Forman ingredients are known in closed form, for the device-memory paths of csrc/dcr_bfc_giant.hip: the
giant path (giant_edge: k_giant_mark / sweep / stream / finish / unmark) and the hub-side sweep (k_find_hubs, k_hub_edges,
process_hub_edges).  Plain numpy, in the style of tests/bfc_fan_ref.py, whose restated closing expression is the one used here.

Every family takes the kernel limits it is about as parameters, so that tests/test_hub_giant_ref_cpu.py can prove its closed
forms against the C oracle with hubs of a few hundred neighbours and tests/test_hub_giant_limits_gpu.py can run it at the
limits the sources spell (``limits``).  Rows of a new graph are ascending by id, so an id decides its position in every row.

    three_hubs    two adjacent hubs a, b with more than ``base`` neighbours each and a third, c, adjacent to both; every common
                  neighbour, every 4-cycle corner and every row with hits sits behind position ``base`` of the rows of a and b
    stream_fan    one edge {a, b} with more than ``grid`` rows in DY = N(b) \\ N(a), long rows, a row without a hit, hits behind
                  a row's position 2 * block, gamma decided by a row or by a corner
    stars         hubs that are not adjacent, leaves with one partner per group of leaves (4-cycles through the hub), leaves
                  joined in pairs (a triangle), plain leaves (degree 1)
    crossing      a hub whose row is full at a given degree, next to nodes of given degrees: for edits across a threshold
"""
import functools
import os
import re

import numpy as np

from bfc_fan_ref import bfc_formula, bits, coalesce   # noqa: F401  (re-exported: the tests take them from here)
from conftest import PKG


def _source(name):
    with open(os.path.join(PKG, 'csrc', name)) as f:
        return f.read()


def _int(pattern, text, what, group=1):
    m = re.search(pattern, text)
    assert m, what + ' not found'
    return int(m.group(group), 0)


@functools.lru_cache(maxsize=None)
def limits():
    """Constants of csrc/dcr_bfc_giant.hip and of the routing rules, as the sources spell them."""
    giant, route, common, bfc = (_source(t) for t in ('dcr_bfc_giant.hip', 'dcr_pass_route.h', 'dcr_bfc_common.h', 'dcr_bfc.hip'))
    L = {
        'NC_MAXD': _int(r'constexpr\s+int\s+NC_MAXD\s*=\s*(\d+)\s*;', route, 'NC_MAXD'),
        'NC_MAXOTHER': _int(r'constexpr int NC_MAXOTHER = (\d+);', common, 'NC_MAXOTHER'),
        'HUB_OTHER_MAX': _int(r'constexpr int HUB_OTHER_MAX = (\d+);', common, 'HUB_OTHER_MAX'),
        'HUB_TOUCH_CAP': _int(r'constexpr int HUB_TOUCH_CAP = (\d+);', giant, 'HUB_TOUCH_CAP'),
        'BLOCK': _int(r'k_giant_stream, dim3\(gs\), dim3\((\d+)\)', giant, 'block of k_giant_stream'),
        # giant_edge: mark / sweep / unmark grids of (d + 255) / 256 workgroups, capped
        'GRID_CAP': _int(r'\(da \+ 255\) / 256 > (\d+) \? (\d+) :', giant, 'grid cap of giant_edge'),
        'STREAM_GRID': _int(r'db > (\d+) \? (\d+) : db < 1', giant, 'grid cap of k_giant_stream'),
        'FIND_GRID': _int(r'\(n \+ 255\) / 256 > (\d+) \? (\d+) :', giant, 'grid cap of k_find_hubs'),
        'HUB_CNT_MB': _int(r'int64_t waves = \(\(int64_t\)(\d+) << 20\) / \(\(int64_t\)dh \* 4\);', giant, 'counter budget'),
        'HUB_WAVES_MAX': _int(r'if \(waves > (\d+)\) waves = (\d+);', giant, 'wave cap'),
        'GIANT_KEYS': 16384,
    }
    assert re.search(r'\(dh \+ 255\) / 256 > %d \? %d :' % (L['GRID_CAP'], L['GRID_CAP']), giant), 'process_hub_edges: grid cap'
    assert re.search(r'if \(waves > dh\) waves = dh;\s*waves = \(waves / 4\) \* 4;\s*if \(waves < 4\) waves = 4;', giant), 'wave rule'
    assert re.search(r'if \(at < HUB_TOUCH_CAP\) touched\[at\] = px - 1;', giant) and re.search(r'if \(ntl <= HUB_TOUCH_CAP\)', giant)
    # the largest table of the edge-centric kernels: NC_MAXD = GIANT_KEYS / 2 - 2, and the giant list exists from 2 * bound + 2 keys
    assert re.search(r'2 \* \(int64_t\)g->max_deg_bound \+ 2 > bin_max_keys\(NBINS - 1\)', bfc), 'giant_possible'
    assert L['NC_MAXD'] == L['GIANT_KEYS'] // 2 - 2 and L['NC_MAXOTHER'] == L['GIANT_KEYS'] - 2
    L['TRIP'] = L['GRID_CAP'] * L['BLOCK']           # entries of a row that the first trip of mark / sweep / unmark covers
    return L


def hub_waves(dh):
    """Waves process_hub_edges launches for a hub of ``dh`` neighbours (one counter array of dh words each)."""
    L = limits()
    w = (L['HUB_CNT_MB'] << 20) // (dh * 4)
    w = min(w, L['HUB_WAVES_MAX'], dh)
    return max(w // 4 * 4, 4)


def slack_full_degree(limit):
    """The degree d0 at creation whose row is full at exactly ``limit`` entries (capacity d0 + max(8, d0 // 4))."""
    d0 = next(d for d in range(limit, 0, -1) if d + max(8, d // 4) <= limit)
    assert d0 + max(8, d0 // 4) == limit, 'no creation degree fills a row at %d' % limit
    return d0


def _six(du, dv, T, rows, ncols):
    """(deg u, deg v, T, |sq u|, |sq v|, gamma) from the rows of DY = N(v) \\ N(u) given as lists of column indices into DX."""
    col = np.zeros(max(ncols, 1), dtype=np.int64)
    for r in rows:
        assert len(set(r)) == len(r)
        col[list(r)] += 1
    su, sv = int((col > 0).sum()), sum(1 for r in rows if len(r))
    gamma = max(int(col.max()), max([len(r) for r in rows] + [0])) if su and sv else 0
    return (int(du), int(dv), int(T), su, sv, gamma)


def flip(e6):
    """The ingredients of (v, u) from those of (u, v)."""
    return (e6[1], e6[0], e6[2], e6[4], e6[3], e6[5])


def tri_values(e6):
    """{'augmented', 'haantjes'} of an edge from its ingredients (classical_curvatures.py:17-27)."""
    return {'augmented': float(4 - e6[0] - e6[1] + 3 * e6[2]), 'haantjes': float(e6[2])}


# ---------------------------------------------------------------------------------------------- giant path: three hubs
def three_hubs(base, dc, nc=5, nx=16, n_oa=9, n_ob=6, n_fbl=8,
               rows_ab=((0, 1, 2, 3, 4), (0, 5), (0,), (6, 7), (0, 9, 15)),
               rows_bc=((0, 1, 2), (2,), (2, 7), ()),
               rows_ac=((3, 4), (4, 10, 11, 12), (4,))):
    """Hubs a = 0, b = 1, c = 2, pairwise adjacent.  Rows (positions):
        a: b, c, FA (``base`` leaves), then C, XL, OA                b: a, c, FB (``base`` leaves), then C, YR, OB, FBL
        c: a, b, OA, OB, FC (leaves; the first of them are the rows ZB and ZA)
    C: common neighbours of a and b.  YR_i - XL_j for j in rows_ab[i]: the 4-cycles of {a, b}.  OA / OB: common neighbours of c
    with a / b only.  ZB_i - FBL_j for j in rows_bc[i]: the 4-cycles of {b, c};  ZA_i - XL_j for j in rows_ac[i]: those of {a, c}.
    Everything behind FA / FB sits at a position above ``base`` + 1 of its hub's row.  deg a > deg b > deg c.
    Returns (edge_index, n, info); info['edges'][(u, v)] = the six ingredients of (u, v)."""
    a, b, c = 0, 1, 2
    nxt = [3]

    def take(k):
        out = list(range(nxt[0], nxt[0] + k))
        nxt[0] += k
        return out

    FA, FB = take(base), take(base)
    C, XL, OA, YR, OB, FBL = take(nc), take(nx), take(n_oa), take(len(rows_ab)), take(n_ob), take(n_fbl)
    n_fc = dc - 2 - n_oa - n_ob
    assert n_fc >= len(rows_bc) + len(rows_ac)
    FC = take(n_fc)
    ZB, ZA = FC[:len(rows_bc)], FC[len(rows_bc):len(rows_bc) + len(rows_ac)]
    src, dst = [a, a, b], [b, c, c]

    def star(h, leaves):
        src.extend([h] * len(leaves))
        dst.extend(leaves)

    for h, parts in ((a, (FA, C, XL, OA)), (b, (FB, C, YR, OB, FBL)), (c, (OA, OB, FC))):
        for p in parts:
            star(h, p)
    for ys, xs, rows in ((YR, XL, rows_ab), (ZB, FBL, rows_bc), (ZA, XL, rows_ac)):
        for y, r in zip(ys, rows):
            star(y, [xs[j] for j in r])
    n = nxt[0]
    da, db = 2 + base + nc + nx + n_oa, 2 + base + nc + len(rows_ab) + n_ob + n_fbl
    assert da > db > dc
    info = {'a': a, 'b': b, 'c': c, 'C': C, 'XL': XL, 'OA': OA, 'YR': YR, 'OB': OB, 'FBL': FBL, 'deg': (da, db, dc),
            'edges': {(a, b): _six(da, db, nc + 1, rows_ab, nx),
                      (b, c): _six(db, dc, n_ob + 1, rows_bc, n_fbl),
                      (a, c): _six(da, dc, n_oa + 1, rows_ac, nx)}}
    return coalesce(src, dst, n), n, info


# ---------------------------------------------------------------------------------------------- giant path: streamed rows
def stream_rows(block, gamma_by):
    """(rows before position ``grid`` of b's row, rows behind it) as (pads, columns): a row longer than ``block``, a long row
    without a hit, a row longer than 2 * block whose hits all sit behind its position 2 * block (pads have smaller ids than any
    x), and gamma decided by a row ('row': block + 44 hits in one row, no column above 2) or by a corner ('corner': x0 in nine
    rows, no row above 3 hits)."""
    if gamma_by == 'row':
        first = [(0, tuple(range(block + 44))), (block + 10, ())]
        second = [(2 * block + 8, tuple(range(5, 12))), (0, (0, 1, 2))]
    else:
        first = [(0, (0, 1)), (block + 10, ()), (block + 44, (0,))]
        second = [(2 * block + 8, (0, 5, 6))] + [(0, (0,))] * 6
    return first, second


def stream_fan(da, grid, block, gamma_by, nc=3):
    """a = 0, b = 1; ids ascending: pads, C, the first rows, ``grid`` leaves of b, the second rows, X (leaves of a).  Row b is
    a, C, first rows, leaves, second rows: the second rows sit at positions >= ``grid``.  Returns (edge_index, n, info)."""
    first, second = stream_rows(block, gamma_by)
    rows = first + second
    a, b = 0, 1
    nxt = [2]

    def take(k):
        out = list(range(nxt[0], nxt[0] + k))
        nxt[0] += k
        return out

    pads = [take(p) for p, _ in rows]
    C, Y1, YF, Y2 = take(nc), take(len(first)), take(grid), take(len(second))
    X = take(da - 1 - nc)
    assert max(max(r[1], default=-1) for r in rows) < len(X)
    src, dst = [a], [b]
    for h, parts in ((a, (C, X)), (b, (C, Y1, YF, Y2))):
        for p in parts:
            src.extend([h] * len(p))
            dst.extend(p)
    for y, pad, (_, cols) in zip(Y1 + Y2, pads, rows):
        for k in pad + [X[j] for j in cols]:
            src.append(y)
            dst.append(k)
    n = nxt[0]
    db = 1 + nc + len(Y1) + grid + len(Y2)
    info = {'a': a, 'b': b, 'Y1': Y1, 'Y2': Y2, 'X': X, 'rows': rows, 'row_len': [1 + p + len(cols) for p, cols in rows],
            'edges': {(a, b): _six(da, db, nc, [cols for _, cols in rows], len(X))}}
    return coalesce(src, dst, n), n, info


# ---------------------------------------------------------------------------------------------- hub-side sweep: stars
class Stars:
    """Hubs 0 .. H-1, not adjacent to each other; then one partner per group; then the leaves, one block of ids per hub, so
    that the leaf at position p of hub k's row is ``base[k] + p``; ``spare`` isolated nodes at the end.  A group is a list of
    positions: its partner is adjacent to exactly those leaves.  A pair (p, q) joins two leaves.  A leaf is in at most one
    group or pair.  With the hub at ``dh`` neighbours (leaves appended later change nothing else):
        leaf of a group of g      (dh, 2, 0, g - 1, 1, g - 1)      N(leaf) \\ N(hub) = {partner}, whose row hits the g - 1 others
        leaf of a pair            (dh, 2, 1, 0, 0, 0)
        plain leaf                degree 1: 0.0 by bfc_naive.py:18-19
    """

    def __init__(self, hubs, spare=0):
        self.H = len(hubs)
        self.deg = [int(h['deg']) for h in hubs]
        groups = [(k, list(g)) for k, h in enumerate(hubs) for g in h.get('groups', ())]
        self.base, nxt = [], self.H + len(groups)
        for d in self.deg:
            self.base.append(nxt)
            nxt += d
        self.spare0, self.n = nxt, nxt + spare
        self.kind = [np.zeros(d, dtype=np.int64) for d in self.deg]        # 0 plain, -1 pair, g >= 2 size of the group
        src, dst = [], []
        for k, d in enumerate(self.deg):
            src.extend([k] * d)
            dst.extend(range(self.base[k], self.base[k] + d))
        self.partner = []
        for gi, (k, g) in enumerate(groups):
            assert len(g) >= 2 and len(set(g)) == len(g) and max(g) < self.deg[k] and not self.kind[k][g].any()
            self.kind[k][g] = len(g)
            self.partner.append(self.H + gi)
            src.extend([self.H + gi] * len(g))
            dst.extend(self.base[k] + p for p in g)
        for k, h in enumerate(hubs):
            for p, q in h.get('pairs', ()):
                assert p != q and self.kind[k][p] == 0 and self.kind[k][q] == 0
                self.kind[k][[p, q]] = -1
                src.append(self.base[k] + p)
                dst.append(self.base[k] + q)
        self.ei = coalesce(src, dst, self.n)

    def six(self, k, p, dh=None):
        dh, g = self.deg[k] if dh is None else dh, int(self.kind[k][p])
        return (dh, 1, 0, 0, 0, 0) if g == 0 else (dh, 2, 1, 0, 0, 0) if g < 0 else (dh, 2, 0, g - 1, 1, g - 1)

    def values(self, k, dh=None):
        """Balanced Forman of every creation-time hub-leaf edge of hub k, by position."""
        out = np.zeros(self.deg[k], dtype=np.float64)
        for g in np.unique(self.kind[k]).tolist():
            at = np.flatnonzero(self.kind[k] == g)
            out[at] = 0.0 if g == 0 else bfc_formula(*self.six(k, int(at[0]), dh))
        return out


def touch_star(dh, K, waves, s):
    """One hub; a partner adjacent to K + 1 leaves: positions s .. s + K - 1 and s + K - 1 + waves, which the wave of position
    s + K - 1 takes one round later.  Each of the K + 1 edges flags its own slot and finds K unflagged slots: ntouch = K + 1."""
    late = s + K - 1 + waves
    assert late < dh
    return Stars([{'deg': dh, 'groups': [list(range(s, s + K)) + [late]]}]), late


def budget_stars(d_small, d_big, d_small2, waves_of=hub_waves):
    """Three hubs; every hub has a group of consecutive leaves, a group whose leaves all belong to ONE wave (positions 7 + r *
    waves: the same wave meets the same slots round after round), and pairs."""
    hubs = []
    for d in (d_small, d_big, d_small2):
        w = waves_of(d)
        rounds = min(31, (d - 8) // w + 1)
        one_wave = [7 + r * w for r in range(rounds)]
        lo = 10
        cons = [p for p in range(lo, lo + 60) if p not in one_wave][:50]
        used = set(one_wave) | set(cons)
        free = [p for p in range(100, min(d, 100 + 1200)) if p not in used]
        pairs = [(free[2 * i], free[2 * i + 1]) for i in range(min(500, len(free) // 2))]
        hubs.append({'deg': d, 'groups': [cons] + ([one_wave] if len(one_wave) >= 2 else []), 'pairs': pairs})
    return Stars(hubs)


# ---------------------------------------------------------------------------------------------- edits across a threshold
def crossing(limit, other_degrees, seed, second_hub=None, n_common=0):
    """Hub 0 with d0 = slack_full_degree(limit) neighbours at creation: nodes 1 .. d0 - len(other_degrees) and one node of each
    degree in ``other_degrees`` (a star of its own fresh leaves).  Nodes up to ``limit`` + 40 carry sparse random edges among
    themselves (every one of them far below any class limit), so that the edges of the hub have triangles and 4-cycles.
    ``second_hub``: the degree of a hub adjacent to hub 0 (in place of ``other_degrees``), with ``n_common`` common leaves.
    Returns (edge_index, n, info): info['grow'] are the nodes to add to hub 0 until it has ``limit`` neighbours, info['fresh']
    nodes that are adjacent to neither hub afterwards."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d0 = slack_full_degree(limit)
    others = [second_hub] if second_hub else list(other_degrees)
    pool = limit + 40
    centres = list(range(pool + 1, pool + 1 + len(others)))
    nxt = centres[-1] + 1 if centres else pool + 1
    src, dst = [], []
    own = list(range(1, d0 - len(others) + 1))
    src += [0] * d0
    dst += own + centres
    for ctr, d in zip(centres, others):
        common = own[:n_common] if second_hub else []
        leaves = list(range(nxt, nxt + d - 1 - len(common)))
        nxt += len(leaves)
        src += [ctr] * (len(leaves) + len(common))
        dst += leaves + common
    bg = rng.integers(1, pool + 1, size=(2, 3 * pool))
    keep = bg[0] != bg[1]
    src += bg[0][keep].tolist()
    dst += bg[1][keep].tolist()
    n = nxt
    info = {'d0': d0, 'centres': centres, 'grow': list(range(own[-1] + 1, own[-1] + 1 + limit - d0)),
            'fresh': list(range(own[-1] + 1 + limit - d0, pool + 1))}
    return coalesce(src, dst, n), n, info
