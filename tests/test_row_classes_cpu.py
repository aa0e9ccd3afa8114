"""The census of spectral_ref.plan_family, on the CPU: every boundary of the row plan that tests/test_row_classes_gpu.py claims to
run at is asserted here from spectral_ref.row_plan; the class limits and the two geometries the family was built for are read
out of the sources; and the index arithmetic of csrc/dcr_analysis.h::walk_rows, transcribed into numpy below, is walked over the
grid of row_grid for every plan and both geometries: every row exactly once, by a whole scope of lanes."""
import os
import re

import numpy as np
import pytest

import spectral_ref
from conftest import PKG

CSRC = os.path.join(PKG, 'csrc')

# (short_lanes, turns, NODE): RowGeom<> of the spectral mat-vec and the sweep; ColRows of the column CG, which the resistance and
# diffusion mat-vecs share (under the key 'ResRows', which the ids of the parametrised tests carry)
GEOMETRIES = {'RowGeom<>': (8, 1, 1), 'ResRows': (32, 8, 8)}
MID_ROWS = 4   # medium rows a workgroup takes: a wave each


@pytest.fixture(scope='module')
def plans():
    return {name: spectral_ref.row_plan(ei, n) + (ei, n) for name, ei, n in spectral_ref.plan_family()}


def short_rows(geom):
    lanes, turns, _ = GEOMETRIES[geom]
    return 256 // lanes * turns


# ---- 1. the family is where it says it is ------------------------------------------------------------------------------------------
def test_family_hits_every_listed_boundary(plans):
    counts = {name: p[0] for name, p in plans.items()}
    for name, (nl, nm, ns) in counts.items():
        print(f'  {name}: n = {plans[name][3]}, n_long = {nl}, n_mid = {nm}, n_short = {ns} (% 8 = {ns % 8}, % 32 = {ns % 32}, % 64 = {ns % 64})')
        assert nl + nm + ns == plans[name][3] <= 4300
    assert {0, 1, 3} <= {c[0] for c in counts.values()}
    assert {0, 1, 4, 5, 8, 9} <= {c[1] for c in counts.values()}
    assert any(ns == 0 and nm > 0 for nl, nm, ns in counts.values())              # an empty short class
    assert any(nl > 0 and nm == 0 for nl, nm, ns in counts.values())              # long rows, no medium rows
    assert any(nl == 0 and nm == 0 and ns > 0 for nl, nm, ns in counts.values())  # short rows only
    placed = [ns for nl, nm, ns in counts.values() if ns > 64]   # more than a workgroup of either geometry: a real boundary
    assert {0, 1, 31} <= {ns % 32 for ns in placed}
    assert {0, 1, 7, 8, 9, 63} <= {ns % 64 for ns in placed}
    assert {0, 1, 7} <= {ns % 8 for ns in placed}
    # one graph with everything at once
    nl, nm, ns = counts['long3_mid9_short63']
    assert nl > 1 and nm > 2 * MID_ROWS and nm % MID_ROWS != 0
    assert all(ns > short_rows(g) and ns % short_rows(g) != 0 for g in GEOMETRIES)


def test_family_graphs_are_what_the_gpu_tests_rely_on(plans):
    # the class lists are not id ranges, and the long rows are not nodes 0, 1, ...
    for name in ('long3_mid9_short63', 'long1_mid0_short0', 'mid4_short8', 'mid8_short1'):
        (nl, nm, ns), rows, ei, n = plans[name]
        assert sorted(rows.tolist()) == list(range(n))
        for part in (rows[:nl], rows[nl:nl + nm], rows[nl + nm:]):
            assert np.all(np.diff(part) > 0)                                        # each class by node id
            assert part.size < 2 or part[-1] - part[0] > part.size - 1, name         # with ids of the other classes in between
        assert nl == 0 or rows[0] != 0
    # the three-long-row graph: two long rows adjacent, one adjacent to a medium row
    (nl, nm, ns), rows, ei, n = plans['long3_mid9_short63']
    names = spectral_ref.plan_nodes('long3_mid9_short63')
    adj = spectral_ref.adjacency(ei, n)
    deg = np.asarray(adj.sum(axis=1)).ravel()
    assert sorted(names[f'hub{h}'] for h in range(3)) == rows[:3].tolist()
    assert adj[names['hub0'], names['hub1']] == 1 and adj[names['hub2'], names['hub3']] == 1
    assert deg[names['hub0']] == spectral_ref.LONG_DEG + 1 and deg[names['hub3']] == spectral_ref.SHORT_DEG + 1
    assert deg[names['hub4']] == spectral_ref.LONG_DEG and names['hub4'] in rows[nl:nl + nm]
    # isolated nodes are short rows, one of them the last of the list
    for name in ('long3_mid9_short63', 'long1_mid0_short0', 'mid1_short7', 'mid8_short1'):
        (nl, nm, ns), rows, ei, n = plans[name]
        deg = np.asarray(spectral_ref.adjacency(ei, n).sum(axis=1)).ravel()
        assert (deg == 0).sum() == 2 and deg[rows[-1]] == 0 and rows[-1] == spectral_ref.plan_nodes(name)['isolated']


# ---- 2. the constants in the sources -------------------------------------------------------------------------------------------------
def constant(text, name):
    m = re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, text)
    assert m, name + ' not found'
    return int(m.group(1))


def test_limits_and_geometries_are_those_of_the_sources():
    header = open(os.path.join(CSRC, 'dcr_analysis.h')).read()
    assert constant(header, 'SP_SHORT_DEG') == spectral_ref.SHORT_DEG
    assert constant(header, 'SP_LONG_DEG') == spectral_ref.LONG_DEG
    m = re.search(r'int\s+SHORT_LANES\s*=\s*(\d+)\s*,\s*int\s+TURNS\s*=\s*(\d+)\s*,\s*int\s+NODE\s*=\s*(\d+)', header)
    assert m, 'the defaults of RowGeom not found'
    assert tuple(int(x) for x in m.groups()) == GEOMETRIES['RowGeom<>']
    m = re.search(r'blocks_of\(\s*p\.n_mid\s*,\s*(\d+)\s*\)', header)
    assert m and int(m.group(1)) == MID_ROWS, 'the medium rows of a workgroup in row_grid'
    lanes, turns, node = GEOMETRIES['ResRows']
    assert constant(header, 'COL_SHORT_LANES') == lanes and constant(header, 'COL_SHORT_ROWS') == short_rows('ResRows')
    assert re.search(r'using\s+ColRows\s*=\s*RowGeom<\s*COL_SHORT_LANES\s*,\s*COL_SHORT_ROWS\s*/\s*8\s*,\s*COL_CP\s*>', header) and turns == 8
    m = re.search(r'#\s*define\s+DCR_COL_B\s+(\d+)', header)
    assert m, 'DCR_COL_B not found'
    assert int(m.group(1)) == 2 * node   # a lane takes two columns: COL_B / 2 lanes across a node


# ---- 3. the walker's formula against the grid ------------------------------------------------------------------------------------------
def row_grid(n_long, n_mid, n_short, geom):
    """row_grid<G> of csrc/dcr_analysis.h."""
    return n_long + -(-n_mid // MID_ROWS) + -(-n_short // short_rows(geom))


def walk(n_long, n_mid, n_short, geom):
    """Lanes that reach body() per position of the plan's row list, over workgroups 0 .. grid - 1 of 256 threads.  The lines marked
    `walk_rows` are transcribed from csrc/dcr_analysis.h::walk_rows, integer for integer (C's / on the non-negative values here
    is //); positions are asserted to lie inside the list before they are counted, as the kernel's read of plan.rows must."""
    lanes, turns, _ = GEOMETRIES[geom]
    n = n_long + n_mid + n_short
    visits = np.zeros(n, dtype=np.int64)
    t = np.arange(256)
    for block in range(row_grid(n_long, n_mid, n_short, geom)):
        b_mid = block - n_long                              # walk_rows
        b_short = b_mid - (n_mid + 3) // 4                  # walk_rows
        if b_mid < 0:                                       # walk_rows
            pos = np.full(256, block)                       # walk_rows: plan.rows[blockIdx.x]
        elif b_short < 0:                                   # walk_rows
            i = b_mid * 4 + (t >> 6)                        # walk_rows
            pos = (n_long + i)[i < n_mid]                   # walk_rows: return past the end, else plan.rows[plan.n_long + i]
        else:
            alive = np.ones(256, dtype=bool)
            pos = []
            for turn in range(turns):                       # walk_rows
                i = b_short * short_rows(geom) + turn * (256 // lanes) + t // lanes   # walk_rows
                alive &= i < n_short                        # walk_rows: a lane that returns takes no later turn either
                pos.append((n_long + n_mid + i)[alive])     # walk_rows: plan.rows[plan.n_long + plan.n_mid + i]
            pos = np.concatenate(pos)
        assert pos.size == 0 or (0 <= pos.min() and pos.max() < n), (geom, block)
        np.add.at(visits, pos, 1)
    return visits


@pytest.mark.parametrize('geom', list(GEOMETRIES))
def test_walker_visits_every_row_once(plans, geom):
    lanes = GEOMETRIES[geom][0]
    for name, ((nl, nm, ns), rows, ei, n) in plans.items():
        want = np.concatenate([np.full(nl, 256), np.full(nm, 64), np.full(ns, lanes)])
        assert np.array_equal(walk(nl, nm, ns, geom), want), (name, geom)
    for ns in range(0, 3 * short_rows(geom) + 2):   # every short count across three workgroups, with and without the other classes
        for nl, nm in ((0, 0), (2, 0), (0, 3), (1, 4)):
            want = np.concatenate([np.full(nl, 256), np.full(nm, 64), np.full(ns, lanes)])
            assert np.array_equal(walk(nl, nm, ns, geom), want), (nl, nm, ns, geom)


@pytest.mark.parametrize('geom', list(GEOMETRIES))
def test_scope_lanes_take_every_slot_once_per_column(geom):
    """RowScope: lane l of a scope of LANES lanes starts at slot (l & (LANES - 1)) / NODE and steps by LANES / NODE; the NODE lanes
    of a slot are the NODE columns l % NODE."""
    short_lanes, _, node = GEOMETRIES[geom]
    for scope in (256, 64, short_lanes):
        t = np.arange(256)
        first, stride = (t & (scope - 1)) // node, scope // node   # RowScope::first(), RowScope::stride
        for degree in (0, 1, stride - 1, stride, stride + 1, 33, 2049):
            taken = np.zeros((256 // scope, degree, node), dtype=np.int64)
            for lane in t:
                slots = np.arange(first[lane], degree, stride)
                taken[lane // scope, slots, lane % node] += 1
            assert np.all(taken == 1), (geom, scope, degree)
