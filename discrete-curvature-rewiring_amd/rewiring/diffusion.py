"""Diffusion rewiring (DIGL / GDC), the method SDRF is compared against: the graph is replaced by the sparsified
personalised-PageRank matrix and the same GCN is trained on it.

The reference carries only the two sparsifiers, ``get_top_k_matrix`` and ``get_clipped_matrix``
(utils/adjacency_matrix_ops.py:26-39), on dense ``N x N`` numpy arrays; ``digl`` restates them per column on the device
(``DcrGraph.diffusion``, csrc/dcr_diffusion.hip).  The PageRank matrix they were written for has no counterpart in the
reference: it is defined in include/dcr.h, ``S = alpha (I - (1 - alpha) D~^-1/2 (A + I) D~^-1/2)^-1`` with ``D~ = D + I``.  So is
GDC's other kernel, the heat kernel ``S = exp(-t (I - D~^-1/2 (A + I) D~^-1/2))`` (``get_heat_matrix`` beside ``get_ppr_matrix``
in the code the reference's helpers were adapted from): ``kernel='heat'``."""
import copy

import torch

from dcr.data import Data
from dcr.graph import DcrGraph


def digl(data, alpha=0.15, k=128, eps=None, kernel='ppr', t=5.0):
    """The diffusion-rewired graph of ``data``, a ``Data`` (treated as undirected, as ``rewire`` treats it) or a live
    ``DcrGraph``.  Per column of ``S`` the ``k`` largest entries are kept (``get_top_k_matrix``, whose default ``k = 128`` is the
    default here), or, when ``eps`` is given, the entries ``>= eps`` (``get_clipped_matrix``, whose own default is 0.01) and ``k`` is
    not used; the kept entries of a column are divided by their sum.  ``kernel``: ``'ppr'``, the personalised-PageRank matrix at
    ``alpha``, or ``'heat'``, the heat-kernel matrix at ``t`` (``alpha`` is then not used); anything else is a ``ValueError``.

    Returns a ``Data`` with ``edge_index`` int64 ``[2, nnz]`` holding ``[i; j]`` for the kept ``S_ij`` and ``edge_attr`` float32
    ``[nnz]``, the weights, which models/gcn.py takes as they are; every other attribute of a ``Data`` argument is carried over, and
    the tensors are on the device of its ``edge_index``.  ``DcrGraph.diffusion`` returns the same in float64 with the raw values."""
    if kernel not in ('ppr', 'heat'):
        raise ValueError("kernel must be 'ppr' or 'heat'")
    if isinstance(data, DcrGraph):
        G, out, dev = data, Data(num_nodes=data.num_nodes), torch.device('cpu')
    else:
        G = DcrGraph(data.edge_index, data.num_nodes)
        out = copy.copy(data)
        out.num_nodes = data.num_nodes
        dev = data.edge_index.device if hasattr(data.edge_index, 'device') else torch.device('cpu')
    if eps is not None:
        edge_index, weight = G.diffusion(alpha=alpha, eps=eps, kernel=kernel, t=t)
    else:
        edge_index, weight = G.diffusion(alpha=alpha, k=k, kernel=kernel, t=t)
    out.edge_index = torch.from_numpy(edge_index).to(dev)
    out.edge_attr = torch.from_numpy(weight).float().to(dev)
    return out
