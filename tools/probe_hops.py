"""Time of the hop-distance search (csrc/dcr_hops.hip), wall clock around synchronous calls, best of a few repeats after a warm-up:
  Cora-shaped   every node a source at n = 2,485 (E about 5,000, synthetic source): hop_summary, and hop_distances with its rows
  S100k         256 and 4,096 sampled sources on the bench graph, hop_summary with the batch fixed at one word (64 sources a
                sweep, DCR_HOPS_W=1) against four (256 a sweep, DCR_HOPS_W=4), the two alternating
  rewired       diameter, radius and average path length at Cora's shape before and after 50 FoSR edges on the same handle
Beside each time: the levels (largest eccentricity + 1 sweeps a batch at most) and the cost model's ceiling of gathered bytes,
batches x levels x 8 W x 2 E, over the time; the rows skipped as full are not subtracted, so the rate is an upper bound.
usage (on an MI355X): python tools/probe_hops.py > profiles/hops_probe.txt"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'discrete-curvature-rewiring_amd')]
from dcr import synthetic  # noqa: E402
from dcr.graph import DcrGraph  # noqa: E402
from experiment.hop_metrics import draw_sources, hop_metrics  # noqa: E402


def wall(fn, reps):
    fn()
    best = float('inf')
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def model(P, words, levels, slots):
    batches = -(-P // (64 * words))
    return batches, batches * levels * 8 * words * slots


def cora():
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    G = DcrGraph(ei, n)
    ecc = G.hop_summary()[0]
    levels = int(ecc.max()) + 1
    t_sum = wall(lambda: G.hop_summary(), 5)
    t_rows = wall(lambda: G.hop_distances(np.arange(n)), 5)
    batches, gathered = model(n, 4, levels, ei.shape[1])
    print(f'Cora-shaped (preferential attachment m=2): n={n} E={ei.shape[1] // 2} all {n} sources, {batches} batches, diameter '
          f'{int(ecc.max())} | hop_summary {t_sum:.2f} ms | hop_distances (with the {n} x {n} rows) {t_rows:.2f} ms | gathered at most '
          f'{gathered / 1e6:.1f} MB, {gathered / t_sum / 1e6:.1f} GB/s', flush=True)


def bench_graph():
    ei, n = synthetic.powerlaw_graph(100000, 10, seed=12345)
    G = DcrGraph(ei, n)
    for P in (256, 4096):
        src = draw_sources(n, P, seed=1)
        times = {1: float('inf'), 4: float('inf')}
        results = {}
        for rep in range(4):                       # the two widths alternate; the first round is the warm-up
            for words in (1, 4):
                os.environ['DCR_HOPS_W'] = str(words)
                t0 = time.perf_counter()
                results[words] = G.hop_summary(src)
                if rep:
                    times[words] = min(times[words], (time.perf_counter() - t0) * 1e3)
        del os.environ['DCR_HOPS_W']
        assert all(np.array_equal(a, b) for a, b in zip(results[1], results[4]))
        levels = int(results[4][0].max()) + 1
        line = f'S100k (preferential attachment m=10): n={n} E={ei.shape[1] // 2} {P} sources, largest eccentricity {levels - 1}'
        for words in (1, 4):
            batches, gathered = model(P, words, levels, ei.shape[1])
            line += (f' | W={words}: {batches} batches {times[words]:.2f} ms ({times[words] / P * 1e3:.1f} us a source; gathered at most '
                     f'{gathered / 1e9:.2f} GB, {gathered / times[words] / 1e6:.0f} GB/s)')
        print(line, flush=True)


def rewired():
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    G = DcrGraph(ei, n)
    before = hop_metrics(G)
    t0 = time.perf_counter()
    added = G.fosr(50).shape[1]
    t_fosr = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    after = hop_metrics(G)
    t_metrics = (time.perf_counter() - t0) * 1e3
    print(f'rewired (Cora-shaped, {added} FoSR edges in {t_fosr:.1f} ms): diameter {before["diameter"]} -> {after["diameter"]}, radius '
          f'{before["radius"]} -> {after["radius"]}, average path length {before["average_path_length"]:.4f} -> '
          f'{after["average_path_length"]:.4f} | hop_metrics (all sources, components included) {t_metrics:.2f} ms', flush=True)


cora()
bench_graph()
rewired()
