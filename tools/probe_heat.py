#!/usr/bin/env python3
"""What the heat kernel costs beside PageRank: ``DcrGraph.diffusion(k=128)`` with ``kernel='heat'`` (t = 5) and ``kernel='ppr'``
(alpha = 0.15), both at tol 1e-10, on one handle, alternating round by round: one batch of 16 columns and all n columns at Cora's
shape (powerlaw_graph(2485, 2, seed=0)); one batch of 16 columns and 1,600 columns of S100k (powerlaw_graph(100000, 10,
seed=12345), the bench graph), where all n columns would be 6,250 batches and are given at the measured rate per batch.

Host clock around whole calls, which are synchronous on return and end with the kept entries on the host; one warm-up of each
shape first; the median of the rounds.  The heat solve is K + 2 launches a batch with nothing read back in between, the PageRank
solve three launches a CG step and a read-back every SP_CHECK_EVERY steps: K and the CG steps are printed beside the times.

Usage:  python tools/probe_heat.py [--out FILE] [--rounds 7] [--columns 1600]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'discrete-curvature-rewiring_amd'))

from dcr import synthetic  # noqa: E402
from dcr.graph import DcrGraph  # noqa: E402

T, ALPHA, K_KEEP = 5.0, 0.15, 128


def timed(G, kernel, sources):
    t0 = time.perf_counter()
    _, _, info = G.diffusion(alpha=ALPHA, t=T, k=K_KEEP, sources=sources, kernel=kernel, return_info=True)
    return time.perf_counter() - t0, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--columns', type=int, default=1600)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def compare(G, label, sources):
        count = G.num_nodes if sources is None else len(sources)
        times = {'heat': [], 'ppr': []}
        for kernel in times:
            timed(G, kernel, sources)                     # warm-up of this shape
        for _ in range(args.rounds):
            for kernel in times:
                dt, info = timed(G, kernel, sources)
                times[kernel].append(dt)
                if kernel == 'heat':
                    terms, deficit = info['terms'], info['deficit'].max()
                else:
                    steps, residual = (info['steps'].min(), info['steps'].max()), info['residual'].max()
        mh, mp = statistics.median(times['heat']), statistics.median(times['ppr'])
        batches = (count + 15) // 16
        say(f'{label}, {count} columns ({batches} batches), k={K_KEEP}, medians of {args.rounds}: heat t={T} {1e3 * mh:.2f} ms '
            f'(K {terms}, {terms + 2} launches a batch, max deficit {deficit:.3e}, min .. max {1e3 * min(times["heat"]):.2f} .. '
            f'{1e3 * max(times["heat"]):.2f}); ppr alpha={ALPHA} {1e3 * mp:.2f} ms (CG steps {steps[0]} .. {steps[1]}, max residual '
            f'{residual:.3e}, min .. max {1e3 * min(times["ppr"]):.2f} .. {1e3 * max(times["ppr"]):.2f}); heat / ppr {mh / mp:.2f}')
        return mh, mp, batches

    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    G = DcrGraph(ei, n)
    src = np.random.default_rng(1).permutation(n)
    compare(G, f'cora-size n={n}', src[:16])
    compare(G, f'cora-size n={n}', None)

    ei, n = synthetic.powerlaw_graph(100000, 10, seed=12345)
    G = DcrGraph(ei, n)
    src = np.random.default_rng(1).permutation(n)[:args.columns]
    compare(G, f'S100k n={n}', src[:16])
    mh, mp, batches = compare(G, f'S100k n={n}', src)
    say(f'S100k all {n} columns at the rate of these {batches} batches: heat {mh / batches * (n / 16):.1f} s, ppr {mp / batches * (n / 16):.1f} s')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
