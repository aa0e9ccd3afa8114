"""A device graph and the oracle's graph behind the same edits, with the facts dcr_pass_plan takes kept on the side: every pass
asserts the route it has to take and compares the whole buffer with the oracle by bits.  Shared by tests/test_tri_incremental_gpu.py
and tests/test_bfc_fine_gpu.py."""
import ctypes
import os

import numpy as np

import tri_ref

KINDS = ('augmented', 'haantjes')
CURV = {'bfc': 0, 'augmented': 2, 'haantjes': 3}                       # DCR_CURV_* of include/dcr.h
TWO_HOP, EDGE_CENTRIC, NC_CLASSES, NC_EDGES = 0, 1, 2, 3               # PassRoute of csrc/dcr_pass_route.h
ENGINE = {TWO_HOP: 'two-hop', EDGE_CENTRIC: 'edge-centric', NC_CLASSES: 'node-centric', NC_EDGES: 'node-centric'}
PASS_IMPL = {None: 0, 'edge': 1, 'nc': 2, 'h2': 3}                     # DCR_PASS as dcr_graph_create reads it


class Mirror:
    """A device graph, the oracle's graph behind the same edits, and the facts dcr_pass_plan takes (csrc/dcr_pass_route.h:
    PassFacts) kept on the side as the library keeps them: the sum of squared degrees at creation, the bound on the degrees
    (largest degree at creation + one per added edge), the edits since the last pass and the kind of the last pass."""

    def __init__(self, dcr, oracle, ei, n, monkeypatch=None, dcr_pass=None):
        if dcr_pass is not None:                       # read once, when the graph is created (tests/test_engine_roles_gpu.py)
            monkeypatch.setenv('DCR_PASS', dcr_pass)
        else:
            assert 'DCR_PASS' not in os.environ
        self.G = dcr(ei, n)
        if dcr_pass is not None:
            monkeypatch.delenv('DCR_PASS')
        self.C = oracle.CGraph(ei, n)
        self.n, self.impl = n, PASS_IMPL[dcr_pass]
        deg = np.bincount(ei[0], minlength=n).astype(np.float64)
        assert ei.shape[1] == 2 * self.C.num_edges()   # symmetric and coalesced: ei[0] counts every degree
        self.sum_deg2, self.bound = float((deg * deg).sum()), int(deg.max())
        self.pending, self.last = 0, None

    def add(self, u, v):
        assert not self.C.has_edge(u, v)
        self.G.add_edge(u, v)
        self.C.add_edge(u, v)
        self.pending += 1
        self.bound += 1

    def remove(self, u, v):
        assert self.C.has_edge(u, v)
        self.G.remove_edge(u, v)
        self.C.remove_edge(u, v)
        self.pending += 1

    def toggle(self, u, v):
        self.remove(u, v) if self.C.has_edge(u, v) else self.add(u, v)

    def free_leaf(self, hub, lo, forbid=()):
        """The first node >= lo that is not adjacent to ``hub``."""
        return next(k for k in range(lo, self.n) if k != hub and k not in forbid and not self.C.has_edge(hub, k))

    def plan(self, ct, incremental):
        """(route, list_by_rows, hub_supplement) of dcr_pass_plan for this graph now.  The slots allocated are not exposed: twice
        the edges stands in, which decides nothing below 4,000,000 slots (every graph here is far smaller)."""
        from dcr import _lib
        fine, sweep, full = os.environ.get('DCR_NC_FINE'), os.environ.get('DCR_NC_FINE_SWEEP'), os.environ.get('DCR_NC_FINE_FULL')
        assert full is None or int(full) >= 1 << 30    # (far above any slot count here, so that the stand-in below decides nothing)
        E = self.C.num_edges()
        inc = bool(incremental) and self.last == ct    # a pass of another kind than the last is a full one
        route, rows, hub = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        ms = (ctypes.c_double * 3)()
        rc = _lib.lib().dcr_pass_plan(self.n, E, 2 * E, self.sum_deg2, self.bound, self.pending, self.impl,
                                      int(not (fine is not None and int(fine) == 0)), int(full is not None), int(full or 0),
                                      -1 if sweep is None else int(int(sweep) != 0), CURV[ct], int(inc), ctypes.byref(route),
                                      ctypes.byref(rows), ctypes.byref(hub), ms)
        assert rc == 0
        return route.value, bool(rows.value), bool(hub.value)

    def compare(self, ct, label):
        """Edge lists and value bits of the whole buffer against the oracle and, for the triangle kinds, tests/tri_ref.py."""
        G, C = self.G, self.C
        eu, ev, cv = G.curvature_read()
        ou, ov, oc = C.curv_all(ct, nthreads=8)
        assert np.array_equal(eu, ou) and np.array_equal(ev, ov), (label, 'edge list')
        refs = [('oracle', oc)]
        if ct in KINDS:
            tu, tv, tc = tri_ref.curv_all(C.to_edge_index(), self.n, ct, rows=True)
            assert np.array_equal(eu, tu) and np.array_equal(ev, tv), (label, 'edge list of tri_ref')
            refs.append(('tri_ref', tc))
        for name, want in refs:
            bad = np.flatnonzero(cv.view(np.int64) != want.view(np.int64))
            # (u, v, du, dv, got, want) of the first few stale or wrong edges; the label carries the dirty route
            assert bad.size == 0, (label, ct, name, int(bad.size), [
                (int(eu[i]), int(ev[i]), C.degree(int(eu[i])), C.degree(int(ev[i])), float(cv[i]), float(want[i])) for i in bad[:6]])
        return eu, ev, oc

    def run(self, ct, incremental=True, want=None, label=''):
        """One pass and the whole comparison.  ``want``: the (route, list_by_rows, hub_supplement) this pass has to take."""
        plan = self.plan(ct, incremental)
        label = (label, 'pending', self.pending, 'plan', plan)
        if want is not None:
            assert plan == want, label
        self.G.curvature_pass(ct, incremental=incremental)
        assert self.G.pass_engine() == ENGINE[plan[0]], label
        self.pending, self.last = 0, ct
        self.compare(ct, label)
        return plan
