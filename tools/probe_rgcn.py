"""Times the typed aggregation pair of csrc/dcr_spmm.hip against what the package could do before it: one sweep of the typed CSR
(the gather forward, the expand backward) against R calls of dcr_spmm_csr_f32_dev on per-relation CSRs, the adds that join them
and the add (forward) or copy (backward) of the root term.

Shapes: the bench graph (100,000 nodes, 999,900 edges) with 50 added type-1 edges and with 1 % added, and a Cora-sized graph
with 50 added, each at F = 64 and F = 128.  The added edges are random non-edges from a seeded generator, both directions,
typed 1 as rewiring/fosr.py types them (FoSR itself is not timed here).  The variants run interleaved in rounds; each figure is
the median over the rounds of the mean call time of one round, with the smallest and largest round.

    python tools/probe_rgcn.py [--rounds 9] [--reps 40] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'discrete-curvature-rewiring_amd')]
import numpy as np
import torch

from dcr import _lib, synthetic
from models.gcn import _csr_from_coo, _stream
from models.rgcn import _expand_hip, _gather_hip, rgcn_norm_csr

N_REL = 2


def typed_graph(n, m, added, dev):
    ei, n = synthetic.powerlaw_graph(n, m, seed=12345)
    rng = np.random.default_rng(7)
    have = set((ei[0] * n + ei[1]).tolist())
    new = []
    while len(new) < added:
        u, v = (int(t) for t in rng.integers(0, n, 2))
        if u != v and u * n + v not in have:
            have.update((u * n + v, v * n + u))
            new.append((u, v))
    both = np.array([[u, v] for u, v in new] + [[v, u] for u, v in new], dtype=np.int64).T.reshape(2, -1)
    edge_index = torch.from_numpy(np.concatenate([ei, both], 1)).to(dev)
    edge_type = torch.cat([torch.zeros(ei.shape[1], dtype=torch.int64), torch.ones(both.shape[1], dtype=torch.int64)]).to(dev)
    return edge_index, edge_type, n


def relation_csrs(edge_index, edge_type, n):
    """Per relation: (the CSR by target, the CSR by source) with val = 1 / |N_r(i)|, as the parent commit's kernel takes them."""
    out = []
    for r in range(N_REL):
        sel = edge_type == r
        src, tgt = edge_index[0][sel], edge_index[1][sel]
        val = torch.bincount(tgt, minlength=n).float().reciprocal()[tgt]
        out.append((_csr_from_coo(tgt, src, val, n), _csr_from_coo(src, tgt, val, n)))
    return out


def spmm_into(csr, B, ldb, C, ldc, n, f, bias):
    rowptr, col, val = csr
    _lib.check(_lib.lib().dcr_spmm_csr_f32_dev(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), B.data_ptr(), C.data_ptr(), n, f, ldb,
                                               ldc, None if bias is None else bias.data_ptr(), 0, _stream(B)))


def composed_forward(rels, zall, bias, n, f):
    wide = zall.shape[1]
    out = torch.empty((n, f), dtype=torch.float32, device=zall.device)
    spmm_into(rels[0][0], zall, wide, out, f, n, f, bias)
    for r in range(1, N_REL):
        part = torch.empty_like(out)
        spmm_into(rels[r][0], zall[:, r * f:], wide, part, f, n, f, None)
        out.add_(part)
    return out.add_(zall[:, N_REL * f:])


def composed_backward(rels, grad, n, f):
    wide = (N_REL + 1) * f
    out = torch.empty((n, wide), dtype=torch.float32, device=grad.device)
    for r in range(N_REL):
        spmm_into(rels[r][1], grad, f, out[:, r * f:], wide, n, f, None)      # (the kernel writes the column block in place)
    out[:, N_REL * f:].copy_(grad)
    return out


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
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('probe_rgcn.py measures on the MI355X: no GPU here')
    dev = torch.device('cuda', 0)
    results = []
    for name, nodes, m, added in (('bench graph + 50 edges', 100000, 10, 50), ('bench graph + 1 % edges', 100000, 10, 9999),
                                  ('Cora-sized + 50 edges', 2485, 2, 50)):
        edge_index, edge_type, n = typed_graph(nodes, m, added, dev)
        csr = rgcn_norm_csr(edge_index, edge_type, n, N_REL)
        rels = relation_csrs(edge_index, edge_type, n)
        for f in (64, 128):
            g = torch.Generator(device=dev).manual_seed(f)
            zall = torch.randn(n, (N_REL + 1) * f, device=dev, generator=g)
            grad = torch.randn(n, f, device=dev, generator=g)
            bias = torch.randn(f, device=dev, generator=g)
            variants = {
                'gather': lambda: _gather_hip(csr, zall, bias, True),
                'composed forward': lambda: composed_forward(rels, zall, bias, n, f),
                'expand': lambda: _expand_hip(csr, grad, True),
                'composed backward': lambda: composed_backward(rels, grad, n, f),
            }
            # the two routes compute the same layer: sums in another order, so equal to rounding, not to the bit
            diff_f = float((variants['gather']() - variants['composed forward']()).abs().max())
            diff_b = float((variants['expand']() - variants['composed backward']()).abs().max())
            assert diff_f < 1e-4 and diff_b < 1e-4, (diff_f, diff_b)
            for fn in variants.values():
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    times[k].append(round_time(fn, args.reps))
            row = {'graph': name, 'nodes': n, 'columns': int(edge_index.shape[1]), 'type1_columns': int(edge_type.sum()), 'n_feat': f,
                   'max_abs_diff_forward': diff_f, 'max_abs_diff_backward': diff_b,
                   'us': {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for k, v in times.items()}}
            results.append(row)
            print(f"{name}, F = {f}: " + '; '.join(f"{k} {t['median']:.1f} us ({t['min']:.1f}-{t['max']:.1f})" for k, t in row['us'].items()),
                  flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump({'rounds': args.rounds, 'reps': args.reps, 'results': results}, fh, indent=1)


if __name__ == '__main__':
    main()
