"""Times the attention aggregation of csrc/dcr_gat.hip, forward and backward, against (a) the plain-torch backend of
models/gat.py on the GPU (index_select, scatter-max, exp, scatter-add, divide, scatter-add: what the package could do before)
and (b) dcr_spmm_csr_f32_dev at width H·C on the same CSR, which gathers the same operand rows and is the floor.

Shapes: the bench graph (100,000 nodes, 999,900 edges: 2,099,800 slots with both directions and the self-loops) at
(H, C) = (8, 8), (1, 64) and (1, 7), and a Cora-sized graph at (8, 8) and (1, 7) (the two layers of the paper's model).  The
``attn_dropout 0.6`` rows are the same calls in training with attention dropout: the keep bits are redrawn from the Philox
stream in both sweeps (per 8 slots in the gather, per slot in the expand), nothing is stored; each such call also steps the
device's call counter (one more tiny launch).  The variants run interleaved in rounds, the p = 0 and p = 0.6 paths in the
same process; each figure is the median over the rounds of the mean call time of one round, with the smallest and largest round.

    python tools/probe_gat.py [--rounds 9] [--reps 20] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'discrete-curvature-rewiring_amd')]
import torch

from dcr import _lib, synthetic
from models import gcn
from models.gat import _aggregate_torch, gat_aggregate, gat_csr
from models.gcn import _stream


def round_time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('probe_gat.py measures on the MI355X: no GPU here')
    dev = torch.device('cuda', 0)
    results = []
    for name, nodes, m, shapes in (('bench graph', 100000, 10, ((8, 8), (1, 64), (1, 7))), ('Cora-sized', 2485, 2, ((8, 8), (1, 7)))):
        ei, n = synthetic.powerlaw_graph(nodes, m, seed=12345)
        csr = gat_csr(torch.from_numpy(ei).to(dev), n)
        ones = torch.ones(csr.col.numel(), dtype=torch.float32, device=dev)
        for heads, c in shapes:
            g = torch.Generator(device=dev).manual_seed(heads * 100 + c)
            z, d_out = (torch.randn(n, heads * c, device=dev, generator=g) for _ in range(2))
            s_src, s_dst = (torch.randn(n, heads, device=dev, generator=g) for _ in range(2))
            leaves = [t.clone().requires_grad_(True) for t in (z, s_src, s_dst)]
            out_spmm = torch.empty_like(z)

            def spmm():
                _lib.check(_lib.lib().dcr_spmm_csr_f32_dev(csr.rowptr.data_ptr(), csr.col.data_ptr(), ones.data_ptr(), z.data_ptr(),
                                                           out_spmm.data_ptr(), n, heads * c, heads * c, heads * c, None, 0, _stream(z)))

            def fwd_bwd(fn, *extra):
                out = fn(*leaves, csr, 0.2, *extra)
                torch.autograd.grad(out, leaves, d_out)

            variants = {
                'hip forward': lambda: gat_aggregate(z, s_src, s_dst, csr),
                'torch forward': lambda: _aggregate_torch(z, s_src, s_dst, csr, 0.2),
                'hip forward+backward': lambda: fwd_bwd(gat_aggregate),
                'hip forward, attn_dropout 0.6': lambda: gat_aggregate(z, s_src, s_dst, csr, 0.2, 0.6, True),
                'hip forward+backward, attn_dropout 0.6': lambda: fwd_bwd(gat_aggregate, 0.6, True),
                'torch forward+backward': lambda: fwd_bwd(_aggregate_torch),
                'spmm floor': spmm,
            }
            assert gcn._AGG_BACKEND == 'hip'
            diff = float((variants['hip forward']() - variants['torch forward']()).abs().max())
            assert diff < 1e-4, diff
            for fn in variants.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    times[k].append(round_time(fn, args.reps))
            row = {'graph': name, 'nodes': n, 'slots': int(csr.rowptr[-1]), 'heads': heads, 'channels': c, 'max_abs_diff_forward': diff,
                   'us': {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for k, v in times.items()}}
            results.append(row)
            print(f"{name}, H = {heads}, C = {c}: " + '; '.join(f"{k} {t['median']:.1f} us ({t['min']:.1f}-{t['max']:.1f})"
                                                                  for k, t in row['us'].items()), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump({'rounds': args.rounds, 'reps': args.reps, 'results': results}, fh, indent=1)


if __name__ == '__main__':
    main()
