"""Time of the sketched effective resistance of every edge (csrc/dcr_resistance_sketch.hip) beside the solve-per-edge route, wall
clock around synchronous calls, best of a few repeats after a warm-up:
  Cora-shaped   every edge at n = 2,485 (E about 5,000, synthetic source): edge_resistances(method='cg') as the parent commit has it
                (E / 16 batches) against method='sketch' at k = 64 and k = 256, the sketch with one group a launch
                (DCR_SKETCH_GROUPS=1) and with four, the calls alternating
  S100k         the bench graph (n = 100,000, E about 1 M): the sketch at k = 64 and k = 256 (one group a launch: above 65,536 nodes
                there is no other), and the cg route's time per batch from 10 batches of 16 edges, times the E / 16 batches all
                edges would take: that product is an extrapolation and is printed as one
Beside each sketch time: the CG steps of all columns, the largest true residual, sum R~ - (n - c) with its standard deviation
sqrt(2 (n - c) / k), and at Cora's shape the largest |R~ / R - 1| against the cg values with sqrt(2 / k).
usage (on an MI355X): python tools/probe_resistance_sketch.py > profiles/resistance_sketch_probe.txt"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'discrete-curvature-rewiring_amd')]
from dcr import synthetic  # noqa: E402
from dcr.graph import DcrGraph  # noqa: E402
from experiment.effective_resistance import edge_resistances, sketch_relative_std  # noqa: E402


def wall(fn, reps):
    fn()
    best = float('inf')
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def sketch_line(G, k, c, exact=None):
    (eu, ev, R), info = G.resistance_sketch(columns=k, seed=0, return_info=True)
    n = G.number_of_nodes()
    line = (f'{info["batches"]} batches, {info["steps_total"]} steps over {k} columns ({info["steps_total"] / k:.1f} a column), residual <= '
            f'{info["residual_max"]:.2e}, sum R~ - (n - c) = {R.sum() - (n - c):+.2f} (sigma <= {np.sqrt(2 * (n - c) / k):.2f})')
    if exact is not None:
        line += f', max |R~ / R - 1| = {np.abs(R / exact - 1).max():.3f} (sqrt(2 / k) = {sketch_relative_std(k):.3f})'
    return line


def cora():
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    G = DcrGraph(ei, n)
    c = G.connected_components()[0]
    E = G.number_of_edges()
    exact = edge_resistances(G)[2]
    t_cg = wall(lambda: edge_resistances(G), 3)
    print(f'Cora-shaped (preferential attachment m=2): n={n} E={E} c={c} | method=cg (parent route): {-(-E // 16)} batches {t_cg:.1f} ms',
          flush=True)
    for k in (64, 256):
        times = {1: float('inf'), 4: float('inf')}
        for rep in range(4):                       # the two group counts alternate; the first round is the warm-up
            for groups in (1, 4):
                os.environ['DCR_SKETCH_GROUPS'] = str(groups)
                t0 = time.perf_counter()
                G.resistance_sketch(columns=k, seed=0)
                if rep:
                    times[groups] = min(times[groups], (time.perf_counter() - t0) * 1e3)
        del os.environ['DCR_SKETCH_GROUPS']
        print(f'  method=sketch k={k}: 1 group a launch {times[1]:.2f} ms | 4 groups a launch {times[4]:.2f} ms ({t_cg / times[4]:.1f}x the cg '
              f'route) | {sketch_line(G, k, c, exact)}', flush=True)


def bench_graph():
    ei, n = synthetic.powerlaw_graph(100000, 10, seed=12345)
    G = DcrGraph(ei, n)
    c = G.connected_components()[0]
    E = G.number_of_edges()
    eu, ev = G.edges()
    some = np.stack([eu[:160], ev[:160]], axis=1)
    t_cg = wall(lambda: G.effective_resistance(some), 3) / 10
    batches = -(-E // 16)
    print(f'S100k (preferential attachment m=10): n={n} E={E} c={c} | method=cg: {t_cg:.2f} ms a batch of 16 edges (10 batches timed), '
          f'x {batches} batches = {t_cg * batches / 1e3:.0f} s EXTRAPOLATED, not run', flush=True)
    for k in (64, 256):
        t = wall(lambda: G.resistance_sketch(columns=k, seed=0), 2)
        print(f'  method=sketch k={k}: {t:.1f} ms ({t / (k / 16):.2f} ms a batch) | {sketch_line(G, k, c)}', flush=True)


cora()
bench_graph()
