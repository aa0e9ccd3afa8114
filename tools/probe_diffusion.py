#!/usr/bin/env python3
"""What diffusion rewiring costs: ``DcrGraph.diffusion(k=128)`` at Cora's shape (powerlaw_graph(2485, 2, seed=0)) against the dense
host route a user had to take without it, and 1,600 source columns of S100k (powerlaw_graph(100000, 10, seed=12345), the bench
graph), where all nodes would be n / 16 = 6,250 batches.

The dense host route, in the same run and alternating with the device route round by round: the dense operator from the edge
list, ``numpy.linalg.inv``, then the top-k of utils/adjacency_matrix_ops.py:26-32 restated in numpy (argsort along axis 0, zero
the n - k smallest of each column, divide by the column sums).  Both start from the edge index on the host and end with the result
on the host; the device route's time includes building the graph handle.  Host clock, whole calls, after one warm-up of each.

Usage:  python tools/probe_diffusion.py [--out FILE] [--rounds 5] [--columns 1600]
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


def dense_host_route(ei, n, alpha, k):
    a = np.zeros((n, n))
    a[ei[0], ei[1]] = 1.0
    a[ei[1], ei[0]] = 1.0
    a += np.eye(n)
    s = 1.0 / np.sqrt(a.sum(axis=1))
    S = alpha * np.linalg.inv(np.eye(n) - (1.0 - alpha) * (s[:, None] * a * s[None, :]))
    S[S.argsort(axis=0)[:n - k], np.arange(n)] = 0.0
    norm = S.sum(axis=0)
    norm[norm <= 0] = 1
    return S / norm


def device_route(ei, n, alpha, k):
    return DcrGraph(ei, n).diffusion(alpha=alpha, k=k, return_info=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--columns', type=int, default=1600)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    alpha, k = 0.15, 128
    ei, n = synthetic.powerlaw_graph(2485, 2, seed=0)
    dense = dense_host_route(ei, n, alpha, k)
    edge_index, weight, info = device_route(ei, n, alpha, k)
    same = sum(np.array_equal(edge_index[0][k * j:k * j + k], np.flatnonzero(dense[:, j])) for j in range(n))
    err = np.abs(weight - dense[edge_index[0], edge_index[1]]).max()
    say(f'cora-size n={n}, alpha={alpha}, k={k}: {same} of {n} columns keep the same set as the dense route, max weight difference '
        f'{err:.3e} on all kept entries, CG steps {info["steps"].min()} .. {info["steps"].max()}, max residual {info["residual"].max():.3e}')
    t_dev, t_host = [], []
    for r in range(args.rounds):
        t0 = time.perf_counter()
        device_route(ei, n, alpha, k)
        t1 = time.perf_counter()
        dense_host_route(ei, n, alpha, k)
        t2 = time.perf_counter()
        t_dev.append(t1 - t0)
        t_host.append(t2 - t1)
        say(f'  round {r}: device {1e3 * t_dev[-1]:.1f} ms, dense host {1e3 * t_host[-1]:.1f} ms')
    md, mh = statistics.median(t_dev), statistics.median(t_host)
    say(f'cora-size medians of {args.rounds}: device {1e3 * md:.1f} ms ({n // 16 + 1} batches), dense host {1e3 * mh:.1f} ms, '
        f'ratio host / device {mh / md:.2f}')

    ei, n = synthetic.powerlaw_graph(100000, 10, seed=12345)
    G = DcrGraph(ei, n)
    src = np.random.default_rng(1).permutation(n)[:args.columns]
    G.diffusion(alpha=alpha, k=k, sources=src[:16])
    times = []
    for r in range(max(1, args.rounds // 2)):
        t0 = time.perf_counter()
        _, _, info = G.diffusion(alpha=alpha, k=k, sources=src, return_info=True)
        times.append(time.perf_counter() - t0)
    t = statistics.median(times)
    batches = (len(src) + 15) // 16
    say(f'S100k n={n}, {len(src)} columns, k={k}: {t:.3f} s ({batches} batches, {1e3 * t / batches:.2f} ms a batch, CG steps '
        f'{info["steps"].min()} .. {info["steps"].max()}, max residual {info["residual"].max():.3e}); all {n} columns at this rate: '
        f'{t / batches * (n / 16):.1f} s')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
