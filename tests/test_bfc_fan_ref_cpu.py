"""tests/bfc_fan_ref.py against the C oracle, and proof that the case list of tests/test_bfc_fine_gpu.py reaches the limits it
names.  No GPU: a mistake in the builder, in the restated formula or in a case's shape is caught here, not on the device."""
import numpy as np
import pytest

import bfc_fan_ref as F


@pytest.fixture(scope='module')
def oracle():
    from oracle import c_oracle
    return c_oracle


@pytest.fixture(scope='module')
def reached():
    return {name: F.reach(*F.case(name)[:4]) for name in F.CASES}


def _table_keys(name):
    """(N(u) with one leaf added to u, the table's slots) of a case as the GPU tests run it."""
    ei, n, u, v, e6 = F.case(name)
    keys = ei[1][ei[0] == u].tolist() + [n]
    assert len(keys) == e6[0] + 1
    return keys, F.slots_for(e6[0] + 1)


@pytest.mark.parametrize('name', sorted(F.CASES))
def test_fan_matches_the_oracle(oracle, name):
    """The oracle's ingredients of the fan edge are the closed-form ones and its value has the bits of the restated formula,
    before and after the leaf the GPU tests add to u; u owns the edge (deg u >= deg v) and is the largest degree, so the
    host's bound is deg u."""
    ei, n, u, v, e6 = F.case(name)
    C = oracle.CGraph(ei, n + 1)
    assert ei.shape[1] == 2 * C.num_edges()
    deg = np.bincount(ei[0], minlength=n)
    assert e6[0] == deg[u] == deg.max() and e6[1] == deg[v] and e6[0] >= e6[1] and n + 1 < 66000 and C.num_edges() < 45000
    for want in (e6, F.with_leaf(e6)):
        assert tuple(int(t) for t in C.ingredients(u, v)) == want, name
        assert tuple(int(t) for t in C.ingredients(v, u)) == (want[1], want[0], want[2], want[4], want[3], want[5]), name
        assert F.bits(C.curv_edge(u, v)) == F.bits(F.bfc_formula(*want)) == F.bits(oracle.bfc_formula(*want)), name
        C.add_edge(u, n)
    assert e6[3] > 0 and e6[4] > 0 and e6[5] > 0 and e6[2] > 0       # every fan has triangles and 4-cycles


def test_formula_bits_on_a_grid(oracle):
    """The restated closing expression against the oracle's, both branches."""
    for d1, d2, T, s1, s2, g in [(2, 5, 0, 0, 0, 0), (3, 3, 1, 0, 0, 0), (510, 70, 3, 0, 4, 0), (511, 513, 3, 66, 70, 2),
                                 (8190, 70, 3, 66, 66, 2), (641, 604, 3, 636, 600, 600), (2047, 9, 5, 1, 1, 1), (97, 89, 13, 31, 29, 7)]:
        assert F.bits(F.bfc_formula(d1, d2, T, s1, s2, g)) == F.bits(oracle.bfc_formula(d1, d2, T, s1, s2, g)), (d1, d2, T, s1, s2, g)


def test_restated_rules():
    L = F.limits()
    assert L['TABLES'] == (1024, 4096, 16384) and L['NC_MAXD'] == 16384 // 2 - 2
    assert [F.slots_for(d) for d in (1, 510, 511, 2046, 2047, L['NC_MAXD'], L['NC_MAXD'] + 5)] == [1024, 1024, 4096, 4096, 16384, 16384, 16384]
    # the shift differs per table: the same id has another bucket in each
    assert [int(F.bucket(1, s)) for s in L['TABLES']] == [0x9E3779 >> 16, 0x9E3779 >> 14, 0x9E3779 >> 12]
    assert int(F.bucket((1 << 24) + 5, 4096)) == int(F.bucket(5, 4096))
    count, spilled = F.table_fill([1] * 0 + list(range(40)), 1024)
    assert count.sum() == 40 and count.max() <= 4
    start, deg = F.layout(np.array([[0, 0, 1, 2], [1, 2, 0, 0]]), 4)
    assert start.tolist() == [0, 10, 19, 28] and deg.tolist() == [2, 1, 1, 0]


# ------------------------------------------------------------------------------------------------ the cases reach their limits
def test_tables_at_their_largest_degree():
    """(a) all three tables, each with exactly SLOTS / 2 - 2 keys after the add; one step further is the next table."""
    L = F.limits()
    for name, slots in (('table_510', 1024), ('table_2046', 4096), ('table_nc_maxd', 16384)):
        keys, got = _table_keys(name)
        assert got == slots and len(keys) == slots // 2 - 2, name
        count, _ = F.table_fill(keys, slots)
        assert count.sum() == len(keys)
    assert len(_table_keys('table_nc_maxd')[0]) == L['NC_MAXD']
    assert F.slots_for(511) == 4096 and F.slots_for(2047) == 16384      # the second add of test_table_steps


def test_rows_of_v_cover_rounds_positions_and_orientations(reached):
    """(b) every degree of v with u first and last, at position 256 where the row is long enough, u > v every time and u < v
    for every degree and position once; rows longer than one round of the four waves; posu found in a later batch by a wave
    other than 0 (waves 1 and 3) and by wave 0 in a later round."""
    W = F.limits()['NCF_W']
    seen = set()
    for name, r in reached.items():
        if not name.startswith('row_'):
            continue
        ei, n, u, v, e6 = F.case(name)
        where = 'first' if r['posu'] == 0 else 'last' if r['posu'] == r['deg_v'] - 1 else r['posu']
        seen.add((r['deg_v'], where, u > v))
        assert name == 'row_%d_%s_%s' % (r['deg_v'], 'at256' if where == 256 else where, 'above' if u > v else 'below')
    for dv in F.ROW_DEGREES:
        assert {(dv, 'first', True), (dv, 'last', True)} <= seen
        assert any(s[0] == dv and not s[2] for s in seen)
        if dv > 256:
            assert (dv, 256, True) in seen or (dv == 257 and (dv, 'last', True) in seen)    # 257: position 256 is the last
    assert {s[1] for s in seen if not s[2]} == {'first', 'last', 256} and (257, 'last', False) in seen
    assert max(F.ROW_DEGREES) > 2 * 64 * W and 64 * W + 1 in F.ROW_DEGREES and 64 * W in F.ROW_DEGREES
    late = {r['posu_wave'] for name, r in reached.items() if name.endswith('_above') and r['posu'] >= 64}
    assert {0, 1, 3} <= late                                             # (position 256 and 512: wave 0 in a later round)
    assert reached['row_513_last_above']['posu'] == 512 and reached['row_256_last_above']['posu_wave'] == 3
    assert reached['row_65_last_above']['posu_wave'] == 1
    assert reached['row_513_first_above']['waves'] == [0, 1, 2, 3]


def test_pieces(reached):
    """(c) more pieces in a batch than one round of j0 takes; a step of 64 pieces over more than four row starts (bisection)
    and steps over one to four (the shuffle loop); rows that start off a multiple of 4."""
    L = F.limits()
    assert reached['pieces_many']['pieces'] > 64 * L['NC_Q']
    ei, n, u, v, _ = F.case('pieces_many')
    start, deg = F.layout(ei, n)
    nu = set(ei[1][ei[0] == u].tolist())
    ys = [k for k in ei[1][ei[0] == v].tolist() if k != u and k not in nu]
    assert len(ys) == 160 and all(16 <= deg[k] <= 20 for k in ys)
    assert max(reached['pieces_short']['spans']) > 32 and reached['pieces_short']['pieces'] <= 128
    spans = reached['pieces_long']['spans']
    assert max(spans) <= 4 and any(1 <= s <= 4 for s in spans) and 0 in spans and reached['pieces_long']['pieces'] >= 225
    ei, n, u, v, _ = F.case('pieces_long')
    start, deg = F.layout(ei, n)
    assert sorted(deg[k] for k in ei[1][ei[0] == v].tolist() if k != u and deg[k] > 100) == [302, 335, 412]
    for name in ('pieces_many', 'pieces_short', 'pieces_long'):
        assert reached[name]['unaligned_start'], name


def test_queue(reached):
    """(d) more look-ups in one wave's batch than the queue holds, several times over; an entry position that hits in all 64
    lanes; a piece with all four entries in the table; gamma = 600 on a counter that shares its word with a flagged slot."""
    L = F.limits()
    assert reached['queue_dense']['lookups'] >= 512 >= 4 * L['NC_QCAP']
    assert reached['queue_full_pieces']['full_positions'] >= 4 and reached['queue_full_pieces']['full_piece']
    assert reached['queue_full_pieces']['lookups'] > L['NC_QCAP']
    ei, n, u, v, e6 = F.case('gamma_600')
    assert e6[5] == 600 == e6[1] - e6[2] - 1 and 600 < 1 << 15
    keys, slots = _table_keys('gamma_600')
    count, _ = F.table_fill(keys, slots)
    deg = np.bincount(ei[0], minlength=n)
    x0 = next(k for k in keys[:-1] if deg[k] == 601)
    home = int(F.bucket(x0, slots))
    mates = [k for k in keys if int(F.bucket(k, slots)) == home]
    nv = set(ei[1][ei[0] == v].tolist())
    # two keys in the bucket and none spilling in: they hold its slots 0 and 1, the two halves of one word of slot state
    assert len(mates) == 2 and count[home] == 2 and count[home - 1] < 4 and [k for k in mates if k != x0][0] in nv


@pytest.mark.parametrize('name,slots', [('spill_1024', 1024), ('spill_4096', 4096), ('spill_16384', 16384)])
def test_spills(name, slots):
    """(e) per table: six or more keys whose home is the last bucket (the chain wraps into bucket 0), x with 4-cycles and common
    neighbours among them, and non-neighbours of u with a full home bucket in streamed rows."""
    ei, n, u, v, e6 = F.case(name)
    keys, got = _table_keys(name)
    assert got == slots
    nb = slots // 4
    home = F.bucket(keys, slots)
    count, spilled = F.table_fill(keys, slots)
    at_last = [k for k, h in zip(keys, home.tolist()) if h == nb - 1]
    at_zero = int((home == 0).sum())
    assert len(at_last) >= 6 and spilled and count[nb - 2] < 4 and count[nb - 1] == 4            # nothing spills in, the rest wraps
    assert at_zero >= 1 and count[0] == min(4, at_zero + len(at_last) - 4)
    row = lambda k: set(ei[1][ei[0] == k].tolist())
    nu, nv = row(u), row(v)
    ys = nv - nu - {u}
    xs_hit = [k for k in at_last if k not in nv and row(k) & ys]
    assert len([k for k in at_last if k in nv]) >= 2                                   # triangles through the chain
    # len(at_last) - 4 keys leave the last bucket, whichever they are; all but the keys without a 4-cycle are hits only the walk finds
    assert (len(at_last) - 4) - (len(at_last) - len(xs_hit)) >= 2
    full = {h for h in (nb - 1, 0) if count[h] == 4}
    false = [k for y in ys for k in row(y) - nu - {v} if int(F.bucket(k, slots)) in full]
    assert len(false) >= 3 and nb - 1 in {int(F.bucket(k, slots)) for k in false}
    assert e6[2] == 4 and e6[3] > 9 and e6[5] == 9                                     # T, |sq1|, gamma: each its own number
