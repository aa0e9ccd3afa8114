"""Which kernels run a curvature pass (csrc/dcr_pass_route.h: plan_pass, through the library's dcr_pass_plan — no handle, no
environment, no GPU): the 31 recorded choices of profiles/r05_engine_choice.txt, every boundary of the rules from each side
against a transcription of the rules below, the constants of the sources, and the header alone under the address and
undefined-behaviour sanitizers."""
import ctypes
import itertools
import os
import re
import struct
import subprocess

import pytest

from conftest import PKG, REPO, load_golden

CSRC = os.path.join(PKG, 'csrc')
BFC, ONE_D, AUGMENTED, HAANTJES = 0, 1, 2, 3           # DCR_CURV_* of include/dcr.h
TWO_HOP, EDGE_CENTRIC, NC_CLASSES, NC_EDGES = 0, 1, 2, 3   # PassRoute of csrc/dcr_pass_route.h


def constant(name):
    text = open(os.path.join(CSRC, 'dcr_pass_route.h')).read()
    m = re.search(r'constexpr\s+int\s+%s\s*=\s*(\d+)\s*;' % name, text)
    assert m, name + ' not found'
    return int(m.group(1))


H2_MAXDEG, NC_MAXD, DIRTY_EDITS = constant('H2_MAXDEG'), constant('NC_MAXD'), constant('DIRTY_EDITS')


def library_plan(n, E, cap, sd2, deg, pending, impl, fine_on, full, sweep, curv, inc):
    """(route, list_by_rows, hub_supplement, t_h2, t_nc, t_edges) of dcr_pass_plan; full: None or the slots of DCR_NC_FINE_FULL,
    sweep: None, 0 or 1."""
    from dcr import _lib
    route, rows, hub = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ms = (ctypes.c_double * 3)()
    rc = _lib.lib().dcr_pass_plan(n, E, cap, sd2, deg, pending, impl, int(fine_on), int(full is not None), 0 if full is None else full,
                                  -1 if sweep is None else sweep, curv, int(inc), ctypes.byref(route), ctypes.byref(rows),
                                  ctypes.byref(hub), ms)
    assert rc == 0
    return route.value, bool(rows.value), bool(hub.value), ms[0], ms[1], ms[2]


def rules(n, E, cap, sd2, deg, pending, impl, fine_on, full, sweep, curv, inc):
    """The rules as the issue of this refactor states them, the float64 expressions in the library's operation order."""
    s = sd2 / max(n, 1)
    share = sd2 / max(n, 1) / max(n, 1)
    t_h2 = 0.120 + 1.193e-6 * n + 4.498e-9 * sd2 * (1.0 + 60.0 * share)
    t_nc = 0.127 + 0.438e-6 * E + 1.135e-9 * E * s + 0.201 * min(deg, 400) / 400.0
    t_edges = 0.012 + E * (5.0e-6 + 4.2e-9 * s)
    est = (t_h2, t_nc, t_edges)
    if curv == BFC and not inc and deg <= H2_MAXDEG and cap < 2 ** 30 and (
            impl == 3 or (impl == 0 and n >= 3000 and share <= 0.045 and not (fine_on and t_edges < t_h2) and t_h2 < t_nc)):
        return (TWO_HOP, False, False) + est
    if curv == ONE_D or impl == 1:
        return (EDGE_CENTRIC, False, False) + est
    hub = deg > NC_MAXD
    if inc and fine_on and pending <= DIRTY_EDITS:
        return (NC_EDGES, (sweep == 0) if sweep is not None else cap >= 4000000, hub) + est
    if not inc and fine_on and ((cap <= full) if full is not None else (impl == 0 and t_edges < t_nc)):
        return (NC_EDGES, False, hub) + est
    return (NC_CLASSES, False, hub) + est


def boundary_grid():
    """Every boundary of the rules from each side; the same grid, in the same order, as tests/pass_route_grid.cpp.  Two edge
    counts put the edge-by-edge estimate on either side of the other two, a million nodes the two-hop estimate above the class
    kernels' (asserted in test_grid_reaches_every_outcome)."""
    for n, over, E, deg, cap, pending, curv, impl, inc, fine_on, full, sweep in itertools.product(
            (2999, 3000, 1000000), (0, 1), (10000, 80000), (H2_MAXDEG, H2_MAXDEG + 1, NC_MAXD, NC_MAXD + 1),
            (3999999, 4000000, 2 ** 30 - 1, 2 ** 30), (DIRTY_EDITS, DIRTY_EDITS + 1), (BFC, ONE_D, AUGMENTED, HAANTJES),
            (0, 1, 2, 3), (False, True), (False, True), (None, -1, 0, 1), (None, 0, 1)):
        sd2 = float(int(0.045 * n * n)) + over   # the largest sum of squared degrees with share <= 0.045, or one more
        yield (n, E, cap, sd2, deg, pending, impl, fine_on, None if full is None else cap + full, sweep, curv, inc)


@pytest.fixture(scope='module')
def grid_plans():
    return [(case, library_plan(*case)) for case in boundary_grid()]


def test_recorded_choices_of_round_5():
    """Automatic choice, full Balanced Forman pass, every switch at its default, cap_total = 2 E: two-hop exactly where the
    probe recorded two-hop.  (sum d^2 from the file's sum d^2 / n, printed to 0.1: no estimate moves by more than 0.4 %, the
    closest call among the 31 is 1.6 %.)"""
    graphs = load_golden('pass_route_r05.json')['graphs']
    assert len(graphs) == 31
    for g in graphs:
        case = (g['n'], g['E'], 2 * g['E'], g['sum_deg2_over_n'] * g['n'], g['max_deg'], 0, 0, True, None, None, BFC, False)
        plan = library_plan(*case)
        print(f"  {g['graph']:40s} n={g['n']:8d} two-hop {plan[3]:8.4f} classes {plan[4]:8.4f} edges {plan[5]:8.4f} ms: route {plan[0]}")
        assert (plan[0] == TWO_HOP) == (g['chosen'] == 'two-hop'), g
        assert plan[0] in (TWO_HOP, NC_CLASSES, NC_EDGES) and plan[1:3] == (False, False)
        assert plan == rules(*case)


def test_every_boundary_from_each_side(grid_plans):
    for case, plan in grid_plans:
        want = rules(*case)
        assert plan[:3] == want[:3], (case, plan, want)
        assert struct.pack('3d', *plan[3:]) == struct.pack('3d', *want[3:]), (case, plan, want)   # to the last bit


def test_grid_reaches_every_outcome(grid_plans):
    """The grid is where it says it is: share on either side of 0.045, every estimate comparison both ways where the rules ask
    for it, every route and both values of both booleans."""
    for n in (2999, 3000, 1000000):
        lo = float(int(0.045 * n * n))
        assert lo / n / n <= 0.045 < (lo + 1) / n / n
    assert {p[0] for _, p in grid_plans} == {TWO_HOP, EDGE_CENTRIC, NC_CLASSES, NC_EDGES}
    assert {p[1] for _, p in grid_plans} == {False, True} and {p[2] for _, p in grid_plans} == {False, True}
    assert {p[5] < p[3] for _, p in grid_plans} == {False, True}      # edge by edge against two-hop
    assert {p[5] < p[4] for _, p in grid_plans} == {False, True}      # edge by edge against the class kernels
    assert {p[3] < p[4] for _, p in grid_plans} == {False, True}      # two-hop against the class kernels


@pytest.mark.parametrize('curv', [AUGMENTED, HAANTJES])
def test_incremental_pass_of_a_triangle_kind(curv):
    """The rows tests/test_tri_incremental_gpu.py relies on, stated as literals (not through rules()): an incremental pass of
    'augmented' / 'haantjes' never takes the two-hop route, whatever DCR_PASS says short of 'edge'; goes edge by edge up to
    DIRTY_EDITS pending edits and through the class kernels beyond; carries the hub supplement above NC_MAXD on both."""
    n, E = 100000, 500000
    sd2 = 40.0 * n                      # sparse: a full Balanced Forman pass of these facts is the two-hop engine's
    assert library_plan(n, E, 2 * E, sd2, 300, 0, 0, True, None, None, BFC, False)[0] == TWO_HOP
    for impl, pending, deg, fine_on, sweep, full in itertools.product(
            (0, 2, 3), (0, 1, DIRTY_EDITS, DIRTY_EDITS + 1, 40), (62, H2_MAXDEG, NC_MAXD, NC_MAXD + 1, 17000), (True, False),
            (None, 0, 1), (None, 0, 2 ** 40)):
        case = (n, E, 2 * E, sd2, deg, pending, impl, fine_on, full, sweep, curv, True)
        route, rows, hub = library_plan(*case)[:3]
        assert route != TWO_HOP, case
        assert route == (NC_EDGES if fine_on and pending <= DIRTY_EDITS else NC_CLASSES), case
        assert hub == (deg > NC_MAXD), case
        assert rows == (route == NC_EDGES and sweep == 0), case      # (2 E slots: below the 4 M of the automatic choice)
        assert library_plan(*case) == rules(*case)
    # by rows from 4 M slots where DCR_NC_FINE_SWEEP is unset; DCR_PASS=edge: the edge-centric kernels, no supplement
    assert library_plan(n, E, 4000000, sd2, 300, 2, 0, True, None, None, curv, True)[:3] == (NC_EDGES, True, False)
    assert library_plan(n, E, 3999999, sd2, 300, 2, 0, True, None, None, curv, True)[:3] == (NC_EDGES, False, False)
    for pending, deg in ((1, 300), (9, 300), (1, NC_MAXD + 1)):
        assert library_plan(n, E, 2 * E, sd2, deg, pending, 1, True, None, None, curv, True)[:3] == (EDGE_CENTRIC, False, False)
    # a full pass of a triangle kind is never the two-hop engine's either (DCR_PASS=h2 included)
    for impl in (0, 2, 3):
        assert library_plan(n, E, 2 * E, sd2, 300, 0, impl, True, None, None, curv, False)[0] in (NC_CLASSES, NC_EDGES)


def test_hub_supplement_flips_between_8190_and_8191():
    """Stated as literals: on both node-centric routes, full and incremental, the hub supplement is planned from a bound on the
    degrees of 8,191 and not at 8,190 (tests/test_hub_giant_limits_gpu.py moves a node across by single edits)."""
    n, E, sd2 = 20000, 60000, 3.0e8                # dense enough that no full pass is the two-hop engine's
    for curv, inc, pending, impl, full, route in (
            (BFC, False, 0, 2, None, NC_CLASSES), (BFC, False, 0, 2, 2 ** 40, NC_EDGES), (BFC, True, 1, 2, None, NC_EDGES),
            (BFC, True, DIRTY_EDITS + 1, 2, None, NC_CLASSES), (BFC, True, 1, 0, None, NC_EDGES), (AUGMENTED, False, 0, 2, None, NC_CLASSES),
            (HAANTJES, True, 1, 0, None, NC_EDGES)):
        for deg, hub in ((8190, False), (8191, True)):
            assert library_plan(n, E, 2 * E, sd2, deg, pending, impl, True, full, None, curv, inc)[:3] == (route, False, hub), (curv, inc, deg)


def test_constants_are_those_of_the_sources():
    """The limits and guards this file's transcription uses, as the sources spell them: a changed constant is a diff here."""
    assert (H2_MAXDEG, NC_MAXD, DIRTY_EDITS) == (5000, 8190, 3)
    header = open(os.path.join(CSRC, 'dcr_pass_route.h')).read()
    assert re.search(r'f\.n\s*>=\s*3000\b', header) and re.search(r'share\s*<=\s*0\.045\b', header)
    assert re.search(r'f\.cap_total\s*<\s*\(int64_t\)1\s*<<\s*30\b', header) and re.search(r'f\.cap_total\s*>=\s*4000000\b', header)
    for coefficient in ('0.120 + 1.193e-6 * n + 4.498e-9 * sd2 * (1.0 + 60.0 * share)',
                        '0.127 + 0.438e-6 * E + 1.135e-9 * E * s + 0.201 * dmax / 400.0', '0.012 + E * (5.0e-6 + 4.2e-9 * s)'):
        assert coefficient in header
    # one definition each
    for name in os.listdir(CSRC):
        if name.endswith(('.hip', '.h', '.cpp')) and name != 'dcr_pass_route.h':
            text = open(os.path.join(CSRC, name)).read()
            for const in ('H2_MAXDEG', 'NC_MAXD', 'DIRTY_EDITS'):
                assert not re.search(r'constexpr\s+int\s+%s\b' % const, text), (name, const)
    assert sorted(re.findall(r'#include\s*[<"]([^>"]+)', header)) == ['dcr.h', 'stdint.h']   # host-only: no HIP include


def test_header_alone_under_the_sanitizers(grid_plans, tmp_path):
    """tests/pass_route_grid.cpp includes the header and nothing of the library, walks the same grid and runs clean under
    -fsanitize=address,undefined (a stand-alone program: nothing is loaded into this process); its tallies are the library's."""
    exe = str(tmp_path / 'pass_route_grid')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', CSRC, '-I', os.path.join(REPO, 'include'),
                           os.path.join(REPO, 'tests', 'pass_route_grid.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == '', run.stderr
    plans = [p for _, p in grid_plans]
    bits = sum(struct.unpack('3Q', struct.pack('3d', *p[3:]))[i] for p in plans for i in range(3)) % 2 ** 64
    want = [sum(p[0] == r for p in plans) for r in range(4)] + [sum(p[1] for p in plans), sum(p[2] for p in plans), bits]
    assert [int(x) for x in run.stdout.split()] == want
