"""Time of a FoSR iteration (csrc/dcr_fosr.hip) at Cora's shape (n = 2,485, E about 5,000, synthetic source) and on the bench graph
S100k, split by what can be timed from the call surface with the wall clock around synchronous calls:
  loop       (fosr(K, 0) - fosr(0, 0)) / K: pick, add_edge and power step of one iteration, host round trips included
  power      (fosr(0, K) - fosr(0, 0)) / K: the four launches of one power step
  order      sweep_cut on the same y: the sort the pick reuses, PLUS the sweep's edge counts and prefix scans, so an upper bound of
             the sort's share
  pick call  fosr_pick: upload of x, row plan, y, sort, pick kernel, one read
Beside them, at Cora's shape only, the dense outer-product restatement of tests/fosr_ref.py on the host (at S100k it would need
80 GB and is not run).
usage (on an MI355X): python tools/probe_fosr.py > profiles/fosr_probe.txt"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'discrete-curvature-rewiring_amd'), os.path.join(REPO, 'tests')]
from dcr import synthetic  # noqa: E402
from dcr.graph import DcrGraph  # noqa: E402


def wall(fn, reps):
    fn()
    best = float('inf')
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def run(name, ei, n, iters, dense):
    x0 = np.random.Generator(np.random.PCG64(1)).standard_normal(n)
    G = DcrGraph(ei, n)
    base = wall(lambda: G.fosr(0, 0, x0=x0), 5)
    power = (wall(lambda: G.fosr(0, iters, x0=x0), 3) - base) / iters
    x = G.fosr(0, 20, x0=x0, return_vector=True)[1]
    deg = np.bincount(ei[0], minlength=n)
    y = x / np.sqrt(deg + 1.0)
    order = wall(lambda: G.sweep_cut(y, return_order=False), 5)
    pick = wall(lambda: G.fosr_pick(x), 5)

    def loop():
        H = DcrGraph(ei, n)
        t0 = time.perf_counter()
        H.fosr(iters, 0, x0=x)
        return time.perf_counter() - t0
    loop()
    per_iter = (min(loop() for _ in range(3)) * 1e3 - base) / iters
    line = (f'{name}: n={n} E={ei.shape[1] // 2} | loop {per_iter:.3f} ms/iteration | power step {power:.3f} ms | order (sweep_cut, upper '
            f'bound of the sort) {order:.3f} ms | pick call {pick:.3f} ms')
    if dense:
        import fosr_ref
        _, d, rows = fosr_ref.degrees_and_rows(ei, n)
        t0 = time.perf_counter()
        fosr_ref.brute_minimum(fosr_ref.y_of(x, d), rows)
        line += f' | dense outer product on the host {(time.perf_counter() - t0) * 1e3:.1f} ms'
    print(line, flush=True)


run('Cora-shaped (preferential attachment m=2)', *synthetic.powerlaw_graph(2485, 2, seed=0), 50, True)
run('S100k (preferential attachment m=10)', *synthetic.powerlaw_graph(100000, 10, seed=12345), 50, False)
