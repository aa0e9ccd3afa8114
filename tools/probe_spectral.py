#!/usr/bin/env python3
"""Steps, restarts and wall time of ``DcrGraph.spectral_gap`` at S100k (powerlaw_graph(100000, 10, seed=12345)) and S1M
(powerlaw_graph(1000000, 10, seed=12345)), next to ``scipy.sparse.linalg.eigsh`` on the same graph and machine.

Timed: whole synchronous calls with the host clock (components, plan, upload, every Lanczos step, the vector coming back), the
first call apart (it allocates the work buffers), then the median of ``--calls`` more.  Correctness at each size: the host residual
|L y - lambda_1 y|_2 of the returned vector, recomputed with scipy.sparse (at S1M this is the only evidence: no eigsh value is
recorded for it).  With ``--kernels`` the script then starts itself once more under ``rocprofv3 --kernel-trace --stats`` (a run
of its own, one call per size, no eigsh), reads the kernel statistics and prints per-kernel times and achieved bytes/s against
the HBM roof (8 TB/s): for the mat-vec from its average time and its fixed traffic (4 B of col and 8 B of gathered z per live
slot, 44 B per row); for the two Gram-Schmidt kernels from their LONGEST launch, which is the one against a full basis when the
call took more steps than the basis has columns ((m + 1) resp. (m + 2) vectors of 8 n bytes).

Usage:  python tools/probe_spectral.py [--out FILE] [--calls 3] [--sizes 100000,1000000] [--no-eigsh] [--kernels [--stats-out CSV]]
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
import spectral_ref  # noqa: E402


HBM_ROOF = 8e12   # bytes/s


def kernel_times(n0, say, stats_out):
    """One call at size n0 in a child process under rocprofv3; per-kernel statistics and achieved bytes/s."""
    tmp = tempfile.mkdtemp(prefix='probe_spectral_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 'p', '--', sys.executable,
               os.path.abspath(__file__), '--calls', '0', '--no-eigsh', '--sizes', str(n0)]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900).stdout
        found = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith('kernel_stats.csv')]
        if not found:
            say(f'n={n0} kernels: no kernel statistics came out of rocprofv3: {out[-400:]}')
            return
        rows = [r for r in csv.DictReader(open(found[0])) if 'k_spec_' in r['Name'] or 'k_cc_' in r['Name']]
        if stats_out:
            root, ext = os.path.splitext(stats_out)
            shutil.copy(found[0], f'{root}_n{n0}{ext}')
        line = [ln for ln in out.splitlines() if 'spectral_gap: lambda1' in ln]
        steps = int(line[0].split('steps=')[1].split()[0]) if line else 0
        head = [ln for ln in out.splitlines() if ln.startswith('# n=')]
        n = int(head[0].split('n=')[1].split()[0]) if head else n0
        edges = int(head[0].split('E=')[1].split()[0]) if head else 0
        m = min(256, (4 << 30) // (8 * n))
        say(f'# n={n} kernels under rocprofv3 (one call, {steps} steps)')
        for r in rows:
            name = r['Name'].split('(')[0].replace('void ', '')
            avg, mx, calls = float(r['AverageNs']), float(r['MaxNs']), int(r['Calls'])
            extra = ''
            if 'k_spec_matvec' in name and edges:
                b = 2 * edges * 12 + 44 * n
                extra = f'  {b / 1e6:.1f} MB per launch: {b / avg * 1e9 / 1e12:.2f} TB/s ({b / avg * 1e9 / HBM_ROOF * 100:.0f}% of the HBM roof)'
            elif ('k_spec_gs_coef' in name or 'k_spec_gs_apply' in name) and steps > m:
                b = 8 * n * (m + (1 if 'coef' in name else 2))
                extra = (f'  longest launch, {m} columns, {b / 1e6:.1f} MB: {b / mx * 1e9 / 1e12:.2f} TB/s '
                         f'({b / mx * 1e9 / HBM_ROOF * 100:.0f}% of the HBM roof)')
            say(f'n={n} {name:28s} x{calls:6d}  avg {avg / 1e3:9.1f} us  max {mx / 1e3:9.1f} us  total {float(r["TotalDurationNs"]) / 1e6:9.1f} ms{extra}')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--sizes', default='100000,1000000')
    ap.add_argument('--no-eigsh', action='store_true')
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--stats-out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for n0 in (int(s) for s in args.sizes.split(',')):
        ei, n = synthetic.powerlaw_graph(n0, 10, seed=12345)
        G = DcrGraph(ei, n)
        say(f'# n={n} E={G.number_of_edges()}')
        t0 = time.perf_counter()
        r = G.spectral_gap(return_vector=True)
        first = time.perf_counter() - t0
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            r2 = G.spectral_gap(return_vector=True)
            ts.append(time.perf_counter() - t0)
            assert r2.lambda1.hex() == r.lambda1.hex() and r2.vector.tobytes() == r.vector.tobytes(), 'two calls differ'
        ts.sort()
        ts = ts or [first]
        L = spectral_ref.laplacian(ei, n)
        host_res = float(np.linalg.norm(L @ r.vector - r.lambda1 * r.vector))
        say(f'n={n} spectral_gap: lambda1={r.lambda1!r} residual={r.residual:.3e} host residual={host_res:.3e} steps={r.steps} '
            f'restarts={r.restarts} components={r.components} converged={r.converged}')
        say(f'n={n} spectral_gap: first call {first * 1e3:.1f} ms; then median {ts[len(ts) // 2] * 1e3:.1f} ms (min {ts[0] * 1e3:.1f}, '
            f'max {ts[-1] * 1e3:.1f}) over {len(ts)} calls; {ts[len(ts) // 2] / r.steps * 1e6:.1f} us per step')
        t0 = time.perf_counter()
        count, _ = G.connected_components()
        say(f'n={n} connected_components: {count} in {(time.perf_counter() - t0) * 1e3:.1f} ms')
        if not args.no_eigsh:
            import scipy.sparse.linalg
            ahat, _ = spectral_ref.normalised_adjacency(ei, n)
            t0 = time.perf_counter()
            top = np.sort(scipy.sparse.linalg.eigsh(ahat, k=count + 1, which='LA', tol=1e-10, return_eigenvectors=False))
            dt = time.perf_counter() - t0
            say(f'n={n} scipy eigsh(k={count + 1}, LA, tol=1e-10): lambda1={1.0 - top[0]!r} in {dt:.2f} s '
                f'(difference {abs(1.0 - top[0] - r.lambda1):.2e})')
        G.close()
    if args.kernels:
        for n0 in (int(s) for s in args.sizes.split(',')):
            kernel_times(n0, say, args.stats_out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
