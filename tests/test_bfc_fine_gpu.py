"""The edge-by-edge Balanced Forman pass (csrc/dcr_bfc_nc.hip: k_nc_fine_list / k_nc_fine_list_rows, k_nc_fine_edges<SLOTS,
MODE_BFC> with nc_edge_wg) at its table, batch, piece and queue limits, on the fans of tests/bfc_fan_ref.py, whose integer
ingredients are known in closed form (tests/test_bfc_fan_ref_cpu.py proves them against the oracle and proves that every case
reaches the limit it is named after).

Every pass goes through Mirror.run (tests/pass_mirror.py): the route dcr_pass_plan gives for the graph's facts and the engine
the library reports are asserted, then the bits of the WHOLE buffer are compared with the C oracle.  On top of that the fan
edge is checked twice, G.bfc_ingredients(u, v) against the closed form and the buffer's value against the restated closing
expression of the closed form, so that a failure names the integer that is wrong.  Everything is compared by bits.

Each fan runs three ways at deg u + 1 (a leaf added to u: every edge of u changes value, a skipped one shows up as stale):
a full pass edge by edge (DCR_NC_FINE_FULL above the slot count: no dirty flags, every edge through the kernel), an incremental
pass with the list from the sweep (DCR_NC_FINE_SWEEP=1) and one with the list from the flagged rows (DCR_NC_FINE_SWEEP=0); then
once through the class kernels (DCR_NC_FINE=0: nc_edge has the same batches, piece list and queue) and once through the
edge-centric kernels (DCR_PASS=edge: an independent implementation)."""
import numpy as np
import pytest

import bfc_fan_ref as F
from pass_mirror import EDGE_CENTRIC, NC_CLASSES, NC_EDGES, Mirror

pytestmark = pytest.mark.gpu

FULL = str(1 << 30)                                   # DCR_NC_FINE_FULL: above any slot count


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


@pytest.fixture(scope='module')
def oracle():
    from oracle import c_oracle
    return c_oracle


def buffer_value(M, u, v):
    """The value the last pass left for the edge {u, v}."""
    eu, ev, cv = M.G.curvature_read()
    at = np.flatnonzero(((eu == u) & (ev == v)) | ((eu == v) & (ev == u)))
    assert at.size == 1, (u, v)
    return float(cv[at[0]])


def check_fan(M, u, v, want6, label):
    got6 = tuple(int(t) for t in M.G.bfc_ingredients(u, v))
    assert got6 == tuple(want6), (label, '(deg u, deg v, T, |sq1|, |sq2|, gamma)', got6, want6)
    got, want = buffer_value(M, u, v), F.bfc_formula(*want6)
    assert F.bits(got) == F.bits(want), (label, 'value of the fan edge', got, want, want6)


def fine_pass(M, monkeypatch, way, label):
    """One pass of the edge-by-edge kernels over the graph as it stands: 'full', or incremental with the list by 'sweep' / 'rows'."""
    if way == 'full':
        monkeypatch.setenv('DCR_NC_FINE_FULL', FULL)
        M.run('bfc', False, (NC_EDGES, False, False), label)
        monkeypatch.delenv('DCR_NC_FINE_FULL')
    else:
        assert M.last == 'bfc' and 0 < M.pending <= F.limits()['DIRTY_EDITS']
        monkeypatch.setenv('DCR_NC_FINE_SWEEP', '0' if way == 'rows' else '1')
        M.run('bfc', True, (NC_EDGES, way == 'rows', False), label)
        monkeypatch.delenv('DCR_NC_FINE_SWEEP')


# ------------------------------------------------------------------------------------------------ (a)-(e): every fan, three ways
@pytest.mark.parametrize('way', ['full', 'sweep', 'rows'])
@pytest.mark.parametrize('name', sorted(F.CASES))
def test_fan_edge_by_edge(dcr, oracle, monkeypatch, name, way):
    ei, n, u, v, e6 = F.case(name)
    leaf, want6 = n, F.with_leaf(e6)
    M = Mirror(dcr, oracle, ei, n + 1)
    if way != 'full':
        M.run('bfc', incremental=False, label=(name, 'first'))
    M.add(u, leaf)
    fine_pass(M, monkeypatch, way, (name, way))
    # the library's bound on the degrees is deg u, and with it the table the case is about
    assert M.bound == want6[0] == M.G.degree(u) and want6[0] <= F.slots_for(M.bound) // 2 - 2
    if name.startswith(('table_', 'spill_')):
        assert F.slots_for(M.bound) == {'510': 1024, '1024': 1024, '2046': 4096, '4096': 4096, 'maxd': 16384, '16384': 16384}[name.split('_')[-1]]
    if name.startswith('pieces_'):
        # the rows streamed for the fan edge are the ones whose layout the CPU test looked at: same members, same lengths
        start, deg = F.layout(ei, n)
        nu = set(M.G.neighbors(u))
        ys = [k for k in M.G.neighbors(v) if k != u and k not in nu]
        assert ys == [k for k in ei[1][ei[0] == v].tolist() if k != u and k not in nu]
        assert [M.G.degree(k) for k in ys] == [int(deg[k]) for k in ys] and any(int(start[k]) % 4 for k in ys)
    check_fan(M, u, v, want6, (name, way))


@pytest.mark.parametrize('order', [('sweep', 'rows'), ('rows', 'sweep')])
@pytest.mark.parametrize('name,limit', [('table_510', 510), ('table_2046', 2046)])
def test_table_steps(dcr, oracle, monkeypatch, name, limit, order):
    """deg u moves limit - 1 -> limit -> limit + 1 by single adds, an incremental pass behind each: the smaller table with exactly
    SLOTS / 2 - 2 keys, then the next one."""
    ei, n, u, v, e6 = F.case(name)
    assert e6[0] == limit - 1
    small, big = F.slots_for(limit), F.slots_for(limit + 1)
    assert limit == small // 2 - 2 and big == 4 * small
    M = Mirror(dcr, oracle, ei, n + 2)
    M.run('bfc', incremental=False, label=(name, 'first'))
    for step, way in enumerate(order):
        M.add(u, n + step)
        fine_pass(M, monkeypatch, way, (name, 'step', step, way))
        assert M.bound == limit + step == M.G.degree(u) and F.slots_for(M.bound) == (small, big)[step]
        check_fan(M, u, v, F.with_leaf(e6, step + 1), (name, 'step', step, way))


@pytest.mark.parametrize('engine', ['classes', 'edge-centric'])
@pytest.mark.parametrize('name', sorted(F.CASES))
def test_fan_through_the_other_kernels(dcr, oracle, monkeypatch, name, engine):
    """The same fans and comparisons: a full pass, the leaf on u, an incremental pass: DCR_NC_FINE=0 by the class kernels (exact
    flags), DCR_PASS=edge by the edge-centric kernels."""
    ei, n, u, v, e6 = F.case(name)
    if engine == 'classes':
        monkeypatch.setenv('DCR_NC_FINE', '0')
        M, want = Mirror(dcr, oracle, ei, n + 1), (NC_CLASSES, False, False)
        M.run('bfc', incremental=False, label=(name, engine, 'full'))           # (two-hop where the plan prefers it)
    else:
        M, want = Mirror(dcr, oracle, ei, n + 1, monkeypatch, 'edge'), (EDGE_CENTRIC, False, False)
        M.run('bfc', False, want, (name, engine, 'full'))
    check_fan(M, u, v, e6, (name, engine, 'full'))
    M.add(u, n)
    M.run('bfc', True, want, (name, engine, 'incremental'))
    check_fan(M, u, v, F.with_leaf(e6), (name, engine, 'incremental'))


# ------------------------------------------------------------------------------------------------ (f): degree 1 in the list kernels
@pytest.mark.parametrize('way', ['sweep', 'rows'])
def test_degree_one_under_bfc(dcr, oracle, monkeypatch, way):
    """Balanced Forman's shortcut (an endpoint of degree 1: 0.0, written by the list kernel itself when the smaller id owns the
    edge, bfc_naive.py:18-19) behind one edit per pass: two leaves of a star joined (both go from degree 1 to 2: the stored 0.0
    of their star edges must be recomputed) and parted (back to exactly 0.0), a fresh leaf on a leaf with the degree-1 endpoint
    once the larger and once the smaller id, an isolated node's first edge and its removal."""
    from dcr import synthetic
    body, nb = synthetic.powerlaw_graph(60, 3, seed=3)
    low, centre, leaves = 0, 61, list(range(62, 132))
    lonely, high, n = 132, 133, 134
    src = (body[0] + 1).tolist() + [centre] + [centre] * 70
    dst = (body[1] + 1).tolist() + [1] + leaves
    M = Mirror(dcr, oracle, synthetic.coalesced_edge_index(np.array(src), np.array(dst), n), n)
    assert [M.C.degree(k) for k in (low, lonely, high, leaves[0], centre)] == [0, 0, 0, 1, 71]
    M.run('bfc', incremental=False, label='first')
    zero = F.bits(0.0)
    assert F.bits(buffer_value(M, centre, leaves[0])) == zero

    def step(label, *fan_edges):
        fine_pass(M, monkeypatch, way, label)
        for (a, b), want6 in fan_edges:
            got = buffer_value(M, a, b)
            want = 0.0 if want6 is None else F.bfc_formula(*want6)
            assert F.bits(got) == F.bits(want), (label, a, b, got, want)

    a, b = leaves[0], leaves[1]
    M.add(a, b)
    step('two leaves joined', ((a, b), (2, 2, 1, 0, 0, 0)), ((centre, a), (71, 2, 1, 0, 0, 0)), ((centre, b), (71, 2, 1, 0, 0, 0)),
         ((centre, leaves[2]), None))
    assert buffer_value(M, centre, a) != 0.0
    M.remove(a, b)
    step('and parted', ((centre, a), None), ((centre, b), None))
    M.add(leaves[2], high)
    step('leaf on a leaf, degree 1 at the larger id', ((leaves[2], high), None), ((centre, leaves[2]), (71, 2, 0, 0, 0, 0)))
    M.add(leaves[3], low)
    step('leaf on a leaf, degree 1 at the smaller id', ((low, leaves[3]), None), ((centre, leaves[3]), (71, 2, 0, 0, 0, 0)))
    M.add(lonely, 5)
    step('first edge of an isolated node', ((lonely, 5), None))
    M.remove(lonely, 5)
    step('and removed again')
    M.remove(leaves[2], high)
    step('a leaf again', ((centre, leaves[2]), None))


# ------------------------------------------------------------------------------------------------ (g): the default
def test_default_full_pass_of_a_small_graph_goes_edge_by_edge(dcr, oracle):
    """No environment set: a full Balanced Forman pass of a graph of Cora's size (2,708 nodes, about 5,400 edges) is planned edge
    by edge, and equals the oracle."""
    import os
    from dcr import synthetic
    assert not [k for k in os.environ if k.startswith(('DCR_NC_FINE', 'DCR_PASS'))]
    ei, n = synthetic.powerlaw_graph(2708, 2, seed=7)
    M = Mirror(dcr, oracle, ei, n)
    M.run('bfc', False, (NC_EDGES, False, False), 'default')
