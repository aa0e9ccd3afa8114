"""The device buffers of a graph and of its SDRF scratch (dcr_graph of csrc/dcr_internal.h, SdrfScratch of csrc/dcr_sdrf.hip):
closing a graph gives back every array its passes, edits and steps allocated or grew on it.  As in test_analysis_state_gpu.py the
tests read the device's free memory around repeated create / use / close cycles; the bounds come from the sizes of the arrays,
not from a run.  Buffers of a fixed few bytes (giant_acc, the queue cursors, the result block) are below what free memory shows:
they are covered by being owning members like the rest, not claimed here."""
import numpy as np
import pytest

import hub_giant_ref as R

pytestmark = pytest.mark.gpu

INF = float('inf')


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


def slack_for(deg):
    """Free slots behind a row at creation (slack_for of csrc/dcr_graph.hip)."""
    return max(8, deg // 4)


def free_memory_drop(cycle, cycles):
    """One warm-up cycle (what the runtime and the first use of every kernel keep is paid there), then the device's free memory
    before and after `cycles` more: (before, after, the drop after each cycle in MiB).  The trace tells a leak, which grows cycle by
    cycle, from a single step of the runtime's own pools."""
    import torch

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    cycle()
    before = free()
    trace = []
    for _ in range(cycles):
        cycle()
        trace.append((before - free()) >> 20)
    return before, free(), trace


def test_every_engine_and_the_sdrf_step_give_their_buffers_back(dcr, monkeypatch):
    """Per cycle one graph per engine (two-hop, node-centric, edge-centric): a full pass, an incremental pass behind two edits,
    the single-edge and the byte-count calls with their temporaries, SDRF steps on the arg-min edge with the draw on the device
    and with the candidates read back (pinned mirrors), a row filled past its slack so that the graph is laid out again, and a
    full pass on the new layout, whose slot count is beyond the margin the slot-sized arrays were allocated with.
    Bound: 16 bytes per undirected edge, the least one curv array can take (8 bytes for each of two directed slots).  Leaking
    any slot-sized array once per cycle is 20 times that or more; leaking any [n] int32 array is 20 x 0.8 MB = 16 MB against
    about 12.8 MB.
    Measured on an MI355X: in a whole run of tests/ the drop is 0 and the test passes.  As the first GPU work of a process (this
    file run alone) free memory goes down by 16,777,216 bytes once, in the second cycle, and stays there for the other nineteen
    (trace 16, 16, ..., 16 MiB), so the test fails against its 12,799,744; the commit before the buffers became owning members
    gives the same figures.  Forty-two further cycles in one process drop by nothing.  A step that happens once is something the
    runtime keeps, not a buffer lost per cycle; the bound stays where the sizes of the arrays put it."""
    from dcr import synthetic
    n = 200000
    ei, _ = synthetic.powerlaw_graph(n, 4, seed=5)
    edges = ei.shape[1] // 2
    deg = np.bincount(ei[0], minlength=n)
    w = int(np.argmin(deg))                                       # a low-degree node: its row overflows soonest
    fill = slack_for(int(deg[w])) + 4                             # (a few to spare, should an SDRF step have added one of them)
    taken = set(ei[1][ei[0] == w].tolist()) | {w}
    fresh = [k for k in range(n - 1, n - 4 * fill - 64, -1) if k not in taken]
    assert len(fresh) >= fill + 4
    pairs = [(fresh[-1], fresh[-2]), (fresh[-3], fresh[-4])]     # the two edits ahead of the incremental pass: not edges yet
    assert not np.isin(np.array([u * n + v for u, v in pairs]), ei[0].astype(np.int64) * n + ei[1]).any()
    e0 = (int(ei[0][0]), int(ei[1][0]))
    relayouts = []

    def cycle():
        for engine in ('h2', 'nc', 'edge'):
            monkeypatch.setenv('DCR_PASS', engine)                # read when the graph is created
            G = dcr(ei, n)
            G.curvature_pass('bfc')
            for u, v in pairs:
                G.add_edge(u, v)
            G.curvature_pass('bfc', incremental=True)
            G.bfc_ingredients(*e0)
            G.bfc_algorithmic_bytes()
            x, y, _ = G.argext(False)
            G.improvements(x, y, 'bfc', want_candidates=True)
            for _ in range(3):
                _, _, _, _, (x, y, _) = G.sdrf_iteration_device_draw(x, y, 'bfc', INF, 0.5, True, 50.0, incremental=True)
            for k in fresh[:fill]:
                G.add_edge(w, k)
            relayouts.append(G.degree(w) > int(deg[w]) + slack_for(int(deg[w])))  # past the row it was created with
            G.curvature_pass('bfc')
            G.close()

    before, after, trace = free_memory_drop(cycle, 20)
    bound = 16 * edges
    print(f'  free memory: {before} before, {after} after 20 cycles, dropped {before - after}; bound {bound} ({edges} edges)')
    print(f'  drop after each cycle, MiB: {trace}')
    assert all(relayouts) and len(relayouts) == 3 * 21
    assert before - after < bound


def test_hub_and_giant_paths_give_their_buffers_back(dcr):
    """The graph of test_stream_strides (one hub of 16,400 neighbours): a full pass takes the hub supplement, whose per-wave
    counters are 2,048 waves x 16,400 words x 4 bytes = 134 MB (the sizing rule of process_hub_edges), and the single-edge call
    takes the giant-edge path.  Bound: 64 MiB, under half of one counter array; the smaller arrays of these paths are not
    claimed."""
    L = R.limits()
    ei, n, info = R.stream_fan(L['NC_MAXOTHER'] + 18, L['STREAM_GRID'], L['BLOCK'], 'row')
    assert n <= 40000
    a, b = info['a'], info['b']
    assert 2048 * (L['NC_MAXOTHER'] + 18) * 4 > 2 * (64 << 20)

    def cycle():
        G = dcr(ei, n)
        G.curvature_pass('bfc')
        G.bfc_ingredients(a, b)
        G.close()

    before, after, trace = free_memory_drop(cycle, 5)
    bound = 64 << 20
    print(f'  free memory: {before} before, {after} after 5 cycles, dropped {before - after}; bound {bound}')
    print(f'  drop after each cycle, MiB: {trace}')
    assert before - after < bound
