"""Float64 restatements of the GCN's training tail, for the tests to check the product against: Â as PyG 2.0.3 ``gcn_norm``
publishes it, the forward of models/gcn.py:32-44, the NLL loss of experiment/training_loop.py:51 and torch.optim.Adam's update.

Written from the published formulas and from the raw edge list only; nothing here imports ``models.gcn`` (the checker does not
live in what it checks).  Every function works on the device of its inputs."""
import torch


def gcn_norm_fp64(edge_index, edge_weight, n):
    """(src, dst, val) of Â = D^-1/2 (A_w + loops) D^-1/2 in float64, PyG 2.0.3 ``gcn_norm`` (flow source_to_target):

    * weights 1 when ``edge_weight`` is None;
    * ``add_remaining_self_loops(fill_value=1)``: an existing self-loop keeps its weight (one per node expected), every other
      node gets a loop of weight 1; the loops go after the other edges;
    * duplicate edges stay as they are (their entries add up in the aggregation);
    * deg = scatter_add(w, target); deg^-1/2 with inf set to 0; val = deg^-1/2[src] * w * deg^-1/2[dst].

    The aggregation is out[dst] += val * z[src]."""
    src, dst = edge_index[0].long(), edge_index[1].long()
    dev = src.device
    w = (torch.ones(src.shape[0], dtype=torch.float64, device=dev) if edge_weight is None
         else edge_weight.to(device=dev, dtype=torch.float64))
    loop = src == dst
    loop_w = torch.ones(n, dtype=torch.float64, device=dev)
    loop_w[src[loop]] = w[loop]
    nodes = torch.arange(n, device=dev)
    src = torch.cat([src[~loop], nodes])
    dst = torch.cat([dst[~loop], nodes])
    w = torch.cat([w[~loop], loop_w])
    deg = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, dst, w)
    dinv = deg.pow(-0.5)
    dinv[torch.isinf(dinv)] = 0
    return src, dst, dinv[src] * w * dinv[dst]


def dense_a_hat(edge_index, edge_weight, n):
    """Â as a dense float64 [n, n] matrix (rows = targets), duplicates summed."""
    src, dst, val = gcn_norm_fp64(edge_index, edge_weight, n)
    a = torch.zeros((n, n), dtype=torch.float64, device=val.device)
    a.index_put_((dst, src), val, accumulate=True)
    return a


def propagate(norm, z, n, chunk=4_000_000):
    """Â·z in float64 from ``gcn_norm_fp64``'s output (edge chunks bound the memory of the gathered rows)."""
    src, dst, val = norm
    z = z.double()
    out = torch.zeros((n, z.shape[1]), dtype=torch.float64, device=z.device)
    for s in range(0, src.shape[0], chunk):
        e = slice(s, s + chunk)
        out.index_add_(0, dst[e], z[src[e]] * val[e, None])
    return out


def gcn_logits(weights, x, edge_index, n, edge_weight=None, patterns=None, chunk=4_000_000):
    """log_softmax of the GCN of ``weights`` = [(W_i, b_i), ...] (any depth) in float64:
    h_{i+1} = Â·(act(h_i)·W_iᵀ) + b_i, act = relu between layers.  ``patterns``: one float64 multiplier per hidden layer
    instead of relu (the product's own activation and dropout pattern, scaled by 1 / (1 - p))."""
    norm = gcn_norm_fp64(edge_index, edge_weight, n)
    h = x.double()
    for i, (w, b) in enumerate(weights):
        if i:
            h = h * patterns[i - 1] if patterns is not None else torch.relu(h)
        h = propagate(norm, h @ w.double().t(), n, chunk) + b.double()
    return torch.log_softmax(h, dim=1)


def nll_fp64(o, y, ignore_index=-100):
    """F.nll_loss(log_softmax(o), y) in float64 from the RAW outputs ``o`` [m, C], with ``ignore_index`` rows left out of
    the mean: (loss, d loss / d o, the column sums of that gradient = the bias gradient)."""
    o = o.double()
    keep = y != ignore_index
    m = int(keep.sum())
    lp = torch.log_softmax(o, dim=1)
    yk = torch.where(keep, y, torch.zeros_like(y)).long()
    picked = lp.gather(1, yk[:, None]).squeeze(1)
    loss = -(picked * keep).sum() / m
    grad = torch.softmax(o, dim=1)
    grad[torch.arange(o.shape[0], device=o.device), yk] -= 1.0
    grad = grad * keep[:, None] / m
    return loss, grad, grad.sum(0)


def adam_fp64(p, g, m, v, t, lr, betas, eps, weight_decay):
    """One torch.optim.Adam step (amsgrad off, maximize off, L2 weight decay added to the gradient) at step count ``t``
    (1 for the first step), float64; returns (p, m, v)."""
    b1, b2 = betas
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if weight_decay:
        g = g + weight_decay * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps), m, v


def hand_built_graph(seed=0):
    """(edge_index int64 [2, E], edge_weight float32 [E], n) of a small directed graph with every case Â has to get right:
    non-unit positive weights; self-loops of weight != 1 already in the input; a node whose only entry is a zero-weight
    self-loop (deg = 0: its row of Â is empty in value, the layer's output there is the bias alone); a duplicated edge;
    isolated nodes; a node of in-degree 95 and one of 96 (rows of 96 and 97 entries with the self-loop, either side of the
    aggregation kernels' long-row threshold of 96)."""
    g = torch.Generator().manual_seed(seed)
    n = 300
    src, dst = [], []
    src += list(range(1, 96)); dst += [0] * 95                 # node 0: in-degree 95
    src += list(range(101, 197)); dst += [100] * 96            # node 100: in-degree 96
    r = torch.randint(200, 290, (2, 400), generator=g)
    r = r[:, r[0] != r[1]]
    src += r[0].tolist(); dst += r[1].tolist()
    src += [201, 201]; dst += [202, 202]                       # a duplicated edge
    src += [203, 204, 96]; dst += [203, 204, 96]               # self-loops already there (weights set below)
    src += [290]; dst += [290]                                 # node 290: a zero-weight self-loop and nothing else
    w = 0.2 + 2.8 * torch.rand(len(src), generator=g)           # positive, non-unit
    w[-4:-1] = torch.tensor([2.5, 0.3, 4.0])
    w[-1] = 0.0
    return torch.tensor([src, dst], dtype=torch.int64), w.float(), n      # (nodes 197..199 and 291..299: isolated)


def weighted_powerlaw_graph(n=3000, m=3, seed=7):
    """A power-law graph (dcr.synthetic) with positive non-unit weights and self-loops of random weight on every 50th node."""
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(n, m, seed=seed)
    ei = torch.from_numpy(ei)
    loops = torch.arange(0, n, 50)
    ei = torch.cat([ei, torch.stack([loops, loops])], 1)
    g = torch.Generator().manual_seed(seed)
    return ei, (0.1 + 3.0 * torch.rand(ei.shape[1], generator=g)).float(), n
