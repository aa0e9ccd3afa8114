#!/usr/bin/env python3
"""Generate tests/golden/cheeger_bounds_reference.json by RUNNING THE REFERENCE's experiment/cheeger_bounds.py (build container only).

The reference's module is imported unmodified; its dataset loader, which ``cheeger_bounds`` never touches, is replaced by an empty
stand-in, and ``torch_geometric.utils.to_networkx`` by the PyG-2.0.3 restatement tools/make_golden.py uses (PyG is not installed
here).  Only numbers and names are written.  Per graph: how it is made (a generator of dcr/synthetic.py or of tests/spectral_ref.py
with its arguments, or a small edge list), the number of connected components c, the reference's two strings, the first c + 3 eigenvalues of
``scipy.linalg.eigh(nx.normalized_laplacian_matrix(G).toarray())`` as float64 hex, and ``reference_sound``: all c smallest came out
<= 0, so ``lambdas[lambdas > 0][0]`` (cheeger_bounds.py:16) IS the (c+1)-th eigenvalue and the strings are right.  When one of
the c zero eigenvalues comes out as positive rounding noise, the reference returns that noise (``reference_lambda1`` records it).

Two conditions on the file, checked here and again by tests/test_cheeger_bounds_cpu.py: at least three graphs are sound and at
least two are not (the sign of the noise is arbitrary: candidates are tried in order until that holds and all are kept), and no
recorded lambda_1 / 2 or sqrt(2 lambda_1) lies within 1e-6 relative of a rounding boundary of the ' .2e' format (such a graph
is rejected: a solver error of 1e-10 must not flip a printed digit).

The ``scale`` entry is the bench graph, powerlaw_graph(100000, 10): one component, lambda_1 from
``scipy.sparse.linalg.eigsh(tol=1e-12)`` on the normalised adjacency (no dense matrix at that size).  The 1M-node graph is not
recorded: eigsh does not finish it here in reasonable time; tools/probe_spectral.py checks it by the host residual alone.

Usage:  python tools/make_golden_cheeger_bounds.py
"""
import json
import os
import sys
import types

import networkx as nx
import numpy as np
import scipy.linalg
import scipy.sparse.linalg
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
GOLDEN = os.path.join(REPO, 'tests', 'golden')
sys.path.insert(0, os.path.join(REPO, 'discrete-curvature-rewiring_amd'))
sys.path.insert(0, os.path.join(REPO, 'tests'))
from dcr import synthetic  # noqa: E402
from dcr.data import Data  # noqa: E402
import spectral_ref  # noqa: E402


def _to_networkx(data, node_attrs=None, edge_attrs=None, to_undirected=False, remove_self_loops=False):
    """PyG 2.0.3 torch_geometric.utils.to_networkx, restated (graph part only)."""
    G = nx.Graph() if to_undirected else nx.DiGraph()
    G.add_nodes_from(range(data.num_nodes))
    for (u, v) in data.edge_index.t().tolist():
        if to_undirected and v > u:
            continue
        if remove_self_loops and u == v:
            continue
        G.add_edge(u, v)
    return G


def install_shims():
    def module(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    tgd = module('torch_geometric.data', Data=Data)
    tgu = module('torch_geometric.utils', to_networkx=_to_networkx)
    module('torch_geometric', data=tgd, utils=tgu)
    for m in [k for k in sys.modules if k.split('.')[0] == 'experiment']:
        del sys.modules[m]
    sys.path.insert(0, REF)
    module('experiment.data_loader', DataLoader=type('DataLoader', (), {}))


install_shims()
import experiment.cheeger_bounds as ref  # noqa: E402  (reference)

assert ref.__file__.startswith(REF)


def nx_edge_index(G):
    G = nx.convert_node_labels_to_integers(G)
    return synthetic.coalesced_edge_index([u for u, v in G.edges()], [v for u, v in G.edges()], G.number_of_nodes())


def candidates():
    """(name, generator spec or None, edge index or None, num_nodes)"""
    out = [('grid8x8', {'grid_graph': [8, 8]}, None, 64),
           ('powerlaw300m2', {'powerlaw_graph': [300, 2, 12345]}, None, 300),
           ('path200', {'path': [200]}, None, 200),
           ('karate', None, nx_edge_index(nx.karate_club_graph()), 34),
           ('powerlaw2485m2', {'powerlaw_graph': [2485, 2, 3]}, None, 2485),
           ('barbell20_4', {'barbell': [20, 4]}, None, 44),
           ('karate_and_cycle9', None, nx_edge_index(nx.disjoint_union(nx.karate_club_graph(), nx.cycle_graph(9))), 43),
           ('path4_isolated2', None, np.array([[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]]), 6),
           ('grid5x5', {'grid_graph': [5, 5]}, None, 25),
           ('powerlaw400m4', {'powerlaw_graph': [400, 4, 3]}, None, 400),
           ('cycle12', {'cycle': [12]}, None, 12),
           ('star6', {'star': [6]}, None, 6)]
    return out


def edge_index_of(spec, ei):
    if spec is not None:
        (fn, args), = spec.items()
        return (getattr(synthetic, fn) if hasattr(synthetic, fn) else getattr(spectral_ref, fn))(*args)[0]
    return np.asarray(ei, dtype=np.int64).reshape(2, -1)


def near_rounding_boundary(x):
    """x within 1e-6 relative of a value where ' .2e' changes its last digit."""
    e = np.floor(np.log10(x))
    m = x / 10.0 ** e * 100.0
    return abs(m - (np.floor(m) + 0.5)) / m < 1e-6


def main():
    graphs = []
    for name, spec, ei, n in candidates():
        e = edge_index_of(spec, ei)
        data = Data(edge_index=torch.from_numpy(e), num_nodes=n)
        strings = ref.cheeger_bounds(data)
        G = _to_networkx(data, to_undirected=True)
        c = nx.number_connected_components(G)
        lam = scipy.linalg.eigh(nx.normalized_laplacian_matrix(G).toarray(), eigvals_only=True)
        ref_lambda1 = float(lam[np.where(lam > 0)[0]][0])
        sound = bool(np.all(lam[:c] <= 0))
        true = float(lam[c])
        if near_rounding_boundary(true / 2) or near_rounding_boundary(np.sqrt(2 * true)):
            print(f'{name}: rejected, a bound lies on a rounding boundary of the format')
            continue
        graphs.append({'name': name, 'generator': spec, 'edge_index': None if spec is not None else e.tolist(), 'num_nodes': n,
                       'components': c, 'reference': list(strings), 'reference_lambda1': ref_lambda1.hex(),
                       'eigenvalues': [float(v).hex() for v in lam[:c + 3]], 'reference_sound': sound})
        print(f'{name}: n={n} c={c} reference={strings} returned={ref_lambda1:.4e} true={true:.10e} sound={sound}', flush=True)
    n_sound = sum(g['reference_sound'] for g in graphs)
    assert n_sound >= 3 and len(graphs) - n_sound >= 2, (n_sound, len(graphs))
    # the bench graph
    sn, sm, sseed = 100000, 10, 12345
    ei, n = synthetic.powerlaw_graph(sn, sm, seed=sseed)
    c, _ = spectral_ref.components(ei, n)
    ahat, _ = spectral_ref.normalised_adjacency(ei, n)
    top = np.sort(scipy.sparse.linalg.eigsh(ahat, k=c + 1, which='LA', tol=1e-12, return_eigenvectors=False))
    lam1 = float(1.0 - top[0])
    print(f'scale: n={n} c={c} lambda1={lam1!r}', flush=True)
    out = {'_about': 'reference experiment/cheeger_bounds.py: its two strings per graph, the first c + 3 eigenvalues of the dense '
                     'normalised Laplacian (float64 hex), and whether its "first eigenvalue > 0" is the true gap '
                     '(reference_sound) or rounding noise of a zero eigenvalue (reference_lambda1 is what it took)',
           'graphs': graphs,
           'scale': {'generator': {'powerlaw_graph': [sn, sm, sseed]}, 'num_nodes': n, 'components': c, 'lambda1': lam1.hex(),
                     'method': 'scipy.sparse.linalg.eigsh(normalised adjacency, which=LA, tol=1e-12)'}}
    with open(os.path.join(GOLDEN, 'cheeger_bounds_reference.json'), 'w') as f:
        json.dump(out, f, separators=(',', ':'))


if __name__ == '__main__':
    main()
