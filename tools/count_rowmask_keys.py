"""Host count behind the size of class M's row-mask tables (csrc/dcr_bfc_h2.hip, h2_rows_unit).

For every class-M unit of a preferential-attachment graph that the row-mask path takes (at most 128 rows, and the pieces of each
wave's rows within the register-resident batch, by the container's layout of a new graph), replay sweeps A and B on the host with
the kernel's own hashes: which entries find their B2 bit set, how many distinct keys those are (what the exact table has to hold,
the members of N(u) included) and how many of the entries are candidate occurrences (what the candidate list has to hold).  Prints
the distribution over the units and how many units exceed each candidate table size.

    python tools/count_rowmask_keys.py [--nodes 100000] [--m 10]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'discrete-curvature-rewiring_amd'))

L1 = 16                                            # class M: h2_l1(3)
MAXW = (1024, 2048, 4096, 8192)
KEYCAP_M = 2800
WAVES_M, BATCH_PIECES = 4, 64 * 12                 # row i of a unit belongs to wave i % 4; H2_NPB = 12 pieces per lane


def mul24(key, mult):
    return ((key & 0xFFFFFF).astype(np.uint64) * np.uint64(mult)).astype(np.uint64) & np.uint64(0xFFFFFFFF)


def h2_bit(key):
    return ((mul24(key, 0x9e3779) >> np.uint64(24 - L1)) & np.uint64((1 << L1) - 1)).astype(np.int64)


def word_mask(key, b):
    return (np.uint64(1) << (b & 31).astype(np.uint64)) | (np.uint64(1) << ((mul24(key, 0xb55a4f) >> np.uint64(19)) & np.uint64(31)))


def unit(rows, u):
    """(exact-table keys, candidate occurrences) of node u under the kernel's bitmaps.  The order in which the
    kernel's lanes set the bits of B1 decides which occurrence of a key is the one that finds them set, not whether the key's B2
    bit ends up set: any order gives the same B2 but for collisions between singletons, which this replay takes in row order."""
    nb = rows[u]
    keys = np.concatenate([rows[v] for v in nb])
    keys = keys[keys != u].astype(np.int64)
    b = h2_bit(keys)
    m = word_mask(keys, b)
    b1 = {}
    b2 = set()
    for k in nb:                                   # h2_seed
        bb = int(h2_bit(np.array([k]))[0])
        b1[bb >> 5] = b1.get(bb >> 5, 0) | int(word_mask(np.array([k]), np.array([bb]))[0])
        b2.add(bb >> 2)
    for bb, mm in zip(b.tolist(), m.tolist()):     # sweep A
        old = b1.get(bb >> 5, 0)
        if old & mm == mm:
            b2.add(bb >> 2)
        b1[bb >> 5] = old | mm
    flagged = np.fromiter(((bb >> 2) in b2 for bb in b.tolist()), dtype=bool, count=b.size)   # sweep B
    fk = keys[flagged]
    isnb = np.isin(fk, nb)
    table = np.union1d(np.unique(fk), nb).size
    return table, int((~isnb).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=100000)
    ap.add_argument('--m', type=int, default=10)
    args = ap.parse_args()
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(args.nodes, args.m, seed=12345)
    order = np.lexsort((ei[1], ei[0]))
    src, dst = ei[0][order], ei[1][order]
    ptr = np.searchsorted(src, np.arange(n + 1))
    rows = [dst[ptr[i]:ptr[i + 1]] for i in range(n)]
    deg = np.diff(ptr)
    W = np.add.reduceat(deg[dst], ptr[:-1])
    in_m = ~((deg <= 64) & (W <= MAXW[2])) & (W <= MAXW[3]) & (deg + W // 4 <= KEYCAP_M)
    units = np.flatnonzero(in_m)
    small = units[deg[units] <= 128]
    # 16-byte pieces of every row as dcr_graph_create lays a new graph out: rows in node order, max(8, degree / 4) slots of slack each
    start = np.concatenate([[0], np.cumsum(deg + np.maximum(8, deg // 4))[:-1]])
    pieces = np.where(deg > 0, ((start + deg + 3) >> 2) - (start >> 2), 0)
    fit = np.array([u for u in small if max(int(pieces[rows[u][w::WAVES_M]].sum()) for w in range(WAVES_M)) <= BATCH_PIECES], dtype=np.int64)
    print('graph N=%d m=%d: class-M units %d, of at most 128 rows %d, of them within the register batch %d (%.1f %% of class M), of them at most 64 rows %d' %
          (n, args.m, units.size, small.size, fit.size, 100.0 * fit.size / max(units.size, 1), int((deg[fit] <= 64).sum())))
    tab, cand = np.array([unit(rows, int(u)) for u in fit]).T
    for name, a in (('exact-table keys (members of N(u) included)', tab), ('candidate occurrences', cand)):
        print('%s: median %d, 90 %% %d, 99 %% %d, max %d' % (name, np.median(a), np.percentile(a, 90), np.percentile(a, 99), a.max()))
    for slots in (512, 1024, 2048):
        for load in (0.75, 1.0):
            print('  units with more than %.0f %% of %d slots: %d' % (100 * load, slots, int((tab > load * slots).sum())))
    for cap in (1024, 2048, 4096):
        print('  units with more than %d candidate occurrences: %d' % (cap, int((cand > cap).sum())))


if __name__ == '__main__':
    main()
