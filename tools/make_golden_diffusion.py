#!/usr/bin/env python3
"""Generate tests/golden/diffusion_reference.json by RUNNING THE REFERENCE's two GDC sparsifiers, ``get_top_k_matrix`` and
``get_clipped_matrix`` of utils/adjacency_matrix_ops.py, on the dense personalised-PageRank matrix of tests/diffusion_ref.py.

The reference's module is loaded unmodified from the tree given on the command line; ``torch_geometric.data``, of which it names
``InMemoryDataset`` in annotations only, is replaced by an empty stand-in (PyG is not installed here).  Only numbers are written:
per alpha and per helper, the kept node ids of every column (the non-zeros of the helper's result) and their weights.  The
settings and what was asserted go into the .json; the arrays (22,000 numbers: ptr int32, rows int16, weights float64 per case)
into tests/golden/diffusion_reference.npz, named in the .json.  The matrix itself is not in the files:
S = diffusion_ref.ppr_matrix(resistance_ref.random_graph(300, 5), alpha).

Both helpers write into their argument, so each gets a copy.  The reference's ``argsort`` leaves the order of equal values open
and a value next to ``eps`` could fall either side of it in another solve, so the generator asserts, and records, that no column
has its k-th and (k+1)-th largest values within 1e-9 relative and that no entry lies within 1e-9 relative of eps.  Where the
requested eps trips that, the nearest value that does not is taken (steps of 1e-6) and recorded.

Usage:  python tools/make_golden_diffusion.py <path of the reference tree>
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')
sys.path.insert(0, os.path.join(REPO, 'tests'))
import diffusion_ref  # noqa: E402

GRAPH = {'random_graph': [300, 5]}
K, EPS_WANTED, GAP = 8, 0.01, 1e-9


def load_reference(tree):
    tgd = types.ModuleType('torch_geometric.data')
    tgd.InMemoryDataset = type('InMemoryDataset', (), {})
    tg = types.ModuleType('torch_geometric')
    tg.data = tgd
    sys.modules.setdefault('torch_geometric', tg)
    sys.modules.setdefault('torch_geometric.data', tgd)
    path = os.path.join(tree, 'utils', 'adjacency_matrix_ops.py')
    spec = importlib.util.spec_from_file_location('reference_adjacency_matrix_ops', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def columns_of(result, name, arrays):
    """The non-zeros of a dense result, column by column, into arrays[name + '_ptr' | '_rows' | '_weights']; returns their count."""
    jj, ii = np.nonzero(result.T)          # by column, then by node id
    arrays[name + '_ptr'] = np.concatenate([[0], np.cumsum(np.bincount(jj, minlength=result.shape[1]))]).astype(np.int32)
    arrays[name + '_rows'] = ii.astype(np.int16)
    arrays[name + '_weights'] = result[ii, jj].astype(np.float64)
    return int(ii.size)


def top_k_gap(S, k):
    """Smallest relative distance between the k-th and the (k+1)-th largest value over the columns."""
    desc = -np.sort(-S, axis=0)
    return float(np.min((desc[k - 1] - desc[k]) / desc[k - 1]))


def eps_gap(S, eps):
    return float(np.min(np.abs(S - eps)) / eps)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    ei, n = diffusion_ref.random_graph(*GRAPH['random_graph'])
    out = {'_about': 'reference utils/adjacency_matrix_ops.py: get_top_k_matrix and get_clipped_matrix applied to the dense '
                     'personalised-PageRank matrix of tests/diffusion_ref.py; kept node ids per column and their weights, in the .npz',
           'graph': GRAPH, 'num_nodes': n, 'k': K, 'gap': GAP, 'arrays': 'diffusion_reference.npz', 'cases': []}
    arrays = {}
    for i, alpha in enumerate(diffusion_ref.ALPHAS):
        S = diffusion_ref.ppr_matrix(ei, n, alpha)
        assert np.all(S > 0)
        gap_k = top_k_gap(S, K)
        assert gap_k > GAP, (alpha, gap_k)
        eps = EPS_WANTED
        for step in range(1, 2000):
            if eps_gap(S, eps) > GAP:
                break
            eps = EPS_WANTED + (step + 1) // 2 * 1e-6 * (1 if step % 2 else -1)
        gap_eps = eps_gap(S, eps)
        assert gap_eps > GAP, (alpha, eps, gap_eps)
        top = ref.get_top_k_matrix(S.copy(), k=K)
        clipped = ref.get_clipped_matrix(S.copy(), eps=eps)
        case = {'alpha': alpha, 'eps': eps, 'top_k_gap': gap_k, 'eps_gap': gap_eps, 'top_k': f'a{i}_top_k', 'clipped': f'a{i}_clipped'}
        kept = [columns_of(top, case['top_k'], arrays), columns_of(clipped, case['clipped'], arrays)]
        print(f'alpha {alpha}: top-k gap {gap_k:.3e}, eps {eps!r} gap {gap_eps:.3e}, kept {kept[0]} / {kept[1]}')
        out['cases'].append(case)
    with open(os.path.join(GOLDEN, 'diffusion_reference.json'), 'w') as f:
        json.dump(out, f, indent=1)
    np.savez_compressed(os.path.join(GOLDEN, out['arrays']), **arrays)


if __name__ == '__main__':
    main()
