#!/usr/bin/env python3
"""Wall time of ``DcrGraph.sweep_cut`` and ``DcrGraph.fiedler_sweep`` at S100k (powerlaw_graph(100000, 10, seed=12345)) and S1M
(powerlaw_graph(1000000, 10, seed=12345)), next to the host route they replace on the same machine.

Timed, whole synchronous calls with the host clock, one warm-up call apart (it allocates the work buffers), then ``--calls`` more:
minimum, median and maximum are printed.
  * ``sweep_cut`` alone with a standard normal score (upload of the score, sort, edge pass, scans, arg-min, the order coming back);
  * ``fiedler_sweep`` against ``spectral_gap`` with the same seed: the difference is what the sweep costs on top of the solve;
  * the host route: ``spectral_gap(return_vector=True)``, ``to_edge_index()``, then ``tests/sweep_ref.py`` on D^-1/2 y.
Every device result is compared with ``sweep_ref`` on the same score, bit for bit, before its time is printed.  With ``--kernels``
the script starts itself once more under ``rocprofv3 --kernel-trace --stats`` (a run of its own: one ``sweep_cut`` per size after a
warm-up) and prints the per-kernel times.

Usage:  python tools/probe_sweep.py [--out FILE] [--calls 5] [--sizes 100000,1000000] [--no-host] [--sweep-only] [--kernels]
"""
import argparse
import csv
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'discrete-curvature-rewiring_amd'))
sys.path.insert(0, os.path.join(REPO, 'tests'))

from dcr import synthetic  # noqa: E402
from dcr.graph import DcrGraph  # noqa: E402
import sweep_ref  # noqa: E402


def spread(ts):
    ts = sorted(ts)
    return f'median {ts[len(ts) // 2] * 1e3:.2f} ms (min {ts[0] * 1e3:.2f}, max {ts[-1] * 1e3:.2f}) over {len(ts)} calls'


def timed(fn, calls):
    fn()
    ts, r = [], None
    for _ in range(calls):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return ts, r


def same(got, want):
    return (np.array_equal(got.order, want.order) and got.size == want.size and np.array_equal(got.counts, want.counts)
            and (got.value == want.value or (np.isinf(got.value) and np.isinf(want.value))))


def kernel_times(n0, say):
    tmp = tempfile.mkdtemp(prefix='probe_sweep_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'p', '--', sys.executable,
               os.path.abspath(__file__), '--calls', '1', '--sweep-only', '--no-host', '--sizes', str(n0)]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600).stdout
        found = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith('kernel_stats.csv')]
        if not found:
            say(f'n={n0} kernels: no kernel statistics came out of rocprofv3: {out[-400:]}')
            return
        say(f'# n={n0} kernels under rocprofv3 (two sweep_cut calls: the warm-up and one more)')
        for r in csv.DictReader(open(found[0])):
            if 'k_sweep_' not in r['Name'] and 'k_scan_' not in r['Name']:
                continue
            name = r['Name'].split('(')[0].replace('void ', '')
            say(f'n={n0} {name:36s} x{int(r["Calls"]):4d}  avg {float(r["AverageNs"]) / 1e3:8.1f} us  max {float(r["MaxNs"]) / 1e3:8.1f} us  '
                f'total {float(r["TotalDurationNs"]) / 1e6:8.3f} ms')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--sizes', default='100000,1000000')
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--sweep-only', action='store_true')
    ap.add_argument('--kernels', action='store_true')
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for n0 in (int(s) for s in args.sizes.split(',')):
        ei, n = synthetic.powerlaw_graph(n0, 10, seed=12345)
        G = DcrGraph(ei, n)
        say(f'# n={n} E={G.number_of_edges()}')
        score = np.random.Generator(np.random.PCG64(1)).standard_normal(n)
        ts, cut = timed(lambda: G.sweep_cut(score), args.calls)
        if not args.no_host:
            assert same(cut, sweep_ref.sweep(ei, n, score)), 'sweep_cut differs from the restatement'
        say(f'n={n} sweep_cut(random score): value={cut.value!r} k={cut.size}; {spread(ts)}')
        if args.sweep_only:
            G.close()
            continue
        tg, gap = timed(lambda: G.spectral_gap(), args.calls)
        tf, (gap2, fcut, fscore) = timed(lambda: G.fiedler_sweep(), args.calls)
        assert gap2 == gap, 'fiedler_sweep and spectral_gap differ'
        assert same(fcut, sweep_ref.sweep(ei, n, fscore)), 'fiedler_sweep differs from the restatement on its own score'
        say(f'n={n} spectral_gap: lambda1={gap.lambda1!r} steps={gap.steps}; {spread(tg)}')
        say(f'n={n} fiedler_sweep: value={fcut.value!r} k={fcut.size} bracket [{gap.lambda1 / 2!r}, {np.sqrt(2 * gap.lambda1)!r}]; {spread(tf)}')
        say(f'n={n} sweep on top of the solve (difference of the medians): {(sorted(tf)[len(tf) // 2] - sorted(tg)[len(tg) // 2]) * 1e3:.2f} ms')
        if not args.no_host:
            deg = np.bincount(ei[0], minlength=n).astype(np.float64)
            s = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1.0)), 0.0)

            def host():
                t0 = time.perf_counter()
                r = G.spectral_gap(return_vector=True)
                t1 = time.perf_counter()
                live = G.to_edge_index()
                t2 = time.perf_counter()
                h = sweep_ref.sweep(live, n, s * r.vector)
                return h, (t1 - t0, t2 - t1, time.perf_counter() - t2)
            th, (h, parts) = timed(host, max(1, min(args.calls, 3)))
            say(f'n={n} host route: value={h.value!r} k={h.size}; {spread(th)}; last call: solve + vector {parts[0] * 1e3:.1f} ms, '
                f'edge list {parts[1] * 1e3:.1f} ms, numpy sweep {parts[2] * 1e3:.1f} ms')
            say(f'n={n} host sweep part (edge list + numpy) / device sweep on top of the solve: '
                f'{(parts[1] + parts[2]) / max(sorted(tf)[len(tf) // 2] - sorted(tg)[len(tg) // 2], 1e-9):.1f}x; '
                f'whole host route / fiedler_sweep: {sorted(th)[len(th) // 2] / sorted(tf)[len(tf) // 2]:.2f}x')
        G.close()
    if args.kernels:
        for n0 in (int(s) for s in args.sizes.split(',')):
            kernel_times(n0, say)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
