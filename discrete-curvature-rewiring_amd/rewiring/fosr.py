"""FoSR, first-order spectral rewiring (Karhadkar, Banerjee, Montufar, ICLR 2023), the third rewiring SDRF is compared against:
edges are added one at a time, each the pair that raises the spectral gap most to first order.

The reference has no FoSR.  The definitions are in include/dcr.h and restated in tests/fosr_ref.py; the edge is chosen on the
device in O(n log n + E) (``DcrGraph.fosr``, csrc/dcr_fosr.hip), not from the dense ``n x n`` outer product of the published code."""
import copy

import numpy as np
import torch

from dcr.data import Data
from dcr.graph import DcrGraph


def fosr(data, num_iterations, initial_power_iters=50, x0=None, seed=0):
    """The FoSR-rewired graph of ``data``, a ``Data`` (treated as undirected, as ``rewire`` treats it) or a live ``DcrGraph``
    (which is then rewired in place as well).

    Returns a ``Data`` whose ``edge_index`` int64 ``[2, M + 2 added]`` is the input's (``to_edge_index()`` of a ``DcrGraph``
    before the call) followed by ``(u, v), (v, u)`` of each added edge in the order added, and whose ``edge_type`` int64 is 0 on
    the input's entries and 1 on the added ones, for the relational models of the paper (models/rgcn.py: ``RGCN`` reads it;
    models/gcn.py trains on ``edge_index`` as it stands).  Every other attribute of a ``Data`` argument is carried over, and the
    tensors are on the device of its ``edge_index``.  Only pairs that are not yet edges are ever added (include/dcr.h)."""
    if isinstance(data, DcrGraph):
        G, out, dev = data, Data(num_nodes=data.num_nodes), torch.device('cpu')
        before = torch.from_numpy(G.to_edge_index())
    else:
        G = DcrGraph(data.edge_index, data.num_nodes)
        out = copy.copy(data)
        out.num_nodes = data.num_nodes
        before = torch.as_tensor(data.edge_index)
        dev = before.device
    added = G.fosr(num_iterations, initial_power_iters=initial_power_iters, x0=x0, seed=seed)
    both = np.stack([added, added[::-1]], axis=2).reshape(2, -1)   # (u, v), (v, u) per edge
    out.edge_index = torch.cat([before.to(torch.int64).cpu(), torch.from_numpy(both)], dim=1).to(dev)
    out.edge_type = torch.cat([torch.zeros(before.shape[1], dtype=torch.int64),
                               torch.ones(both.shape[1], dtype=torch.int64)]).to(dev)
    return out
