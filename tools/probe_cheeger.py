#!/usr/bin/env python3
"""Draws per second of the Monte-Carlo Cheeger estimate, both kernel shapes (DCR_CHEEGER=sliced | lane), at S100k
(powerlaw_graph(100000, 10, seed=12345): 1M edges) and at Cora's size (powerlaw_graph(2485, 2, seed=0)).

Timed: whole synchronous calls of ``DcrGraph.cheeger_philox_values`` (device draw of the subsets, counting sweep, ratios, the
8 B per subset coming back) with the host clock, the two shapes alternating within each round, after a warm-up of every
shape and size; then ``estimate_cheeger`` with the reference's ``random`` stream (the host generates the subsets).  Kernel
times come from a profiler run of this same script (``--calls 5 --rounds 1`` under ``rocprofv3 --kernel-trace --stats``).

Usage:  python tools/probe_cheeger.py [--out FILE] [--rounds 5] [--calls 20]
"""
import argparse
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'discrete-curvature-rewiring_amd'))

from dcr import synthetic  # noqa: E402
from dcr.graph import DcrGraph  # noqa: E402
from experiment.compute_cheeger import estimate_cheeger  # noqa: E402

SHAPES = ('sliced', 'lane')


def timed_calls(G, B, calls):
    t0 = time.perf_counter()
    for i in range(calls):
        G.cheeger_philox_values(7, 0, B)
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for name, (ei, n) in (('S100k', synthetic.powerlaw_graph(100000, 10, seed=12345)),
                          ('cora-size', synthetic.powerlaw_graph(2485, 2, seed=0))):
        G = DcrGraph(ei, n)
        E = G.number_of_edges()
        say(f'# {name}: n={n} E={E}')
        want = None
        for B in (64, 1024, 4096, 16384):
            best = {}
            for shape in SHAPES:   # warm-up, and the two shapes must agree
                os.environ['DCR_CHEEGER'] = shape
                vals = G.cheeger_philox_values(7, 0, B)
                want = vals if shape == SHAPES[0] else want
                assert (vals == want).all(), 'the two kernels disagree'
                timed_calls(G, B, 2)
            for r in range(args.rounds):
                for shape in SHAPES:
                    os.environ['DCR_CHEEGER'] = shape
                    t = timed_calls(G, B, args.calls)
                    best.setdefault(shape, []).append(t)
            for shape in SHAPES:
                ts = sorted(best[shape])
                med = ts[len(ts) // 2]
                say(f'{name} B={B:6d} W={B // 64:4d} {shape:7s} call median {med * 1e6:9.1f} us (min {ts[0] * 1e6:9.1f}, max '
                    f'{ts[-1] * 1e6:9.1f})  {B / med:12.0f} draws/s  {B * E / med / 1e9:8.2f} G edge-subsets/s')
        os.environ.pop('DCR_CHEEGER', None)
        random.seed(0)
        estimate_cheeger(G, 256, batch=256)
        t0 = time.perf_counter()
        estimate_cheeger(G, 2048, batch=1024)
        dt = time.perf_counter() - t0
        say(f"{name} estimate_cheeger(rng='python', 2048 draws, batch 1024): {dt * 1e3:.1f} ms  {2048 / dt:.0f} draws/s "
            f'(host Mersenne-Twister subsets, packing and upload included)')
        t0 = time.perf_counter()
        estimate_cheeger(G, 65536, rng='philox', seed=1, batch=16384)
        dt = time.perf_counter() - t0
        say(f"{name} estimate_cheeger(rng='philox', 65536 draws, batch 16384): {dt * 1e3:.1f} ms  {65536 / dt:.0f} draws/s")
        G.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
