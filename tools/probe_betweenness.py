"""Time of the betweenness call (csrc/dcr_betweenness.hip), wall clock around synchronous calls, best of a few repeats after a warm-up:
  Cora-shaped   every node a source at n = 2,485 (E about 5,000, synthetic source): node values alone, and with edge values
  S100k         256 sampled sources on the bench graph, node values alone, and with edge values
  rewired       all sources at Cora's shape before and after 50 FoSR edges on the same handle: the largest edge value both times
Beside each time: the batches, the largest level count, and the cost model's ceiling of gathered bytes, batches x 2 levels x
(64 + 128) x 2 E (a neighbour's 64 bytes of dist and, where a column matches, 128 of sigma; the backward sweep reads delta too, the
rows that return early are not subtracted), over the time: an upper bound of the rate.
usage (on an MI355X): python tools/probe_betweenness.py > profiles/betweenness_probe.txt"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'discrete-curvature-rewiring_amd')]
from dcr import synthetic  # noqa: E402
from dcr.graph import DcrGraph  # noqa: E402
from experiment.hop_metrics import draw_sources  # noqa: E402


def wall(fn, reps):
    fn()
    best = float('inf')
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def line(what, G, slots, sources, reps):
    P = G.num_nodes if sources is None else len(sources)
    _, info = G.betweenness(sources, return_info=True)
    t_node = wall(lambda: G.betweenness(sources), reps)
    t_edge = wall(lambda: G.betweenness(sources, edges=True), reps)
    gathered = info['batches'] * 2 * info['levels_max'] * 192 * slots
    print(f'{what}: n={G.num_nodes} E={slots // 2} {P} sources, {info["batches"]} batches, {info["levels_max"]} levels, sigma_max '
          f'{info["sigma_max"]:.3g} | nodes {t_node:.2f} ms ({t_node / P * 1e3:.1f} us a source) | nodes and edges {t_edge:.2f} ms '
          f'({t_edge / P * 1e3:.1f} us a source) | gathered at most {gathered / 1e9:.2f} GB, {gathered / t_node / 1e6:.0f} GB/s', flush=True)


def cora():
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    line('Cora-shaped (preferential attachment m=2)', DcrGraph(ei, n), ei.shape[1], None, 3)


def bench_graph():
    ei, n = synthetic.powerlaw_graph(100000, 10, seed=12345)
    line('S100k (preferential attachment m=10)', DcrGraph(ei, n), ei.shape[1], draw_sources(n, 256, seed=1), 3)


def rewired():
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    G = DcrGraph(ei, n)
    node0, (_, _, edge0) = G.betweenness(edges=True)
    t0 = time.perf_counter()
    added = G.fosr(50).shape[1]
    t_fosr = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    node1, (_, _, edge1) = G.betweenness(edges=True)
    t_after = (time.perf_counter() - t0) * 1e3
    print(f'rewired (Cora-shaped, {added} FoSR edges in {t_fosr:.1f} ms): largest edge value (ordered pairs) {edge0.max():.1f} -> '
          f'{edge1.max():.1f}, largest node value {node0.max():.1f} -> {node1.max():.1f} | all sources with edge values after the edit '
          f'{t_after:.2f} ms', flush=True)


cora()
bench_graph()
rewired()
