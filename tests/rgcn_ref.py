"""Dense fp64 restatement of the R-GCN layer and of a whole RGCN, from the definition alone (Schlichtkrull et al. eq. 2 with
c_{i,r} = |N_r(i)|, the mean aggregation of torch_geometric's RGCNConv):

    out_i = x_i·W_root + b + Σ_r (1/|N_r(i)|) Σ_{(j->i) of type r} x_j·W_r

|N_r(i)| = the number of columns of edge_index = [source; target] with target i and type r (a duplicated column counts twice, a
self-loop is an ordinary edge of its type, a relation without an edge into i contributes nothing).  Shares no code with
models/rgcn.py: one dense n x n matrix per relation, no CSR, no typed blocks."""
import torch


def relation_means(edge_index, edge_type, num_nodes, num_relations):
    """M[r, i, j] = (columns j -> i of type r) / |N_r(i)|, zero rows where |N_r(i)| = 0; float64 [R, n, n]."""
    ei = torch.as_tensor(edge_index).cpu().long()
    et = torch.as_tensor(edge_type).cpu().long()
    m = torch.zeros(num_relations, num_nodes, num_nodes, dtype=torch.float64)
    for k in range(ei.shape[1]):
        m[int(et[k]), int(ei[1, k]), int(ei[0, k])] += 1.0
    deg = m.sum(2, keepdim=True)
    return torch.where(deg > 0, m / deg.clamp(min=1.0), torch.zeros_like(m))


def layer(x, means, weight, root, bias):
    """One layer on float64 operands: weight [R, in, out], root [in, out] or None, bias [out] or None."""
    out = torch.zeros(x.shape[0], weight.shape[2], dtype=torch.float64)
    for r in range(means.shape[0]):
        out = out + means[r] @ (x @ weight[r])
    if root is not None:
        out = out + x @ root
    if bias is not None:
        out = out + bias
    return out


def logits(params, x, means):
    """log_softmax of the stacked layers, ReLU between them (dropout 0); ``params``: one (weight, root, bias) per layer."""
    h = x
    for i, (weight, root, bias) in enumerate(params):
        h = layer(h, means, weight, root, bias)
        if i < len(params) - 1:
            h = torch.relu(h)
    return torch.log_softmax(h, dim=1)


def model_reference(state_dict, x, edge_index, edge_type, num_relations, y, mask):
    """(log-probabilities, {state-dict key: gradient}) in float64 of loss = nll_loss(log_probs[mask], y[mask]) for the RGCN whose
    ``state_dict`` (keys ``layers.{i}.weight`` / ``.root`` / ``.bias``) is given."""
    n_layers = 1 + max(int(k.split('.')[1]) for k in state_dict)
    leaves = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in state_dict.items()}
    params = [(leaves[f'layers.{i}.weight'], leaves.get(f'layers.{i}.root'), leaves.get(f'layers.{i}.bias')) for i in range(n_layers)]
    means = relation_means(edge_index, edge_type, x.shape[0], num_relations)
    lp = logits(params, x.detach().cpu().double(), means)
    mask, y = torch.as_tensor(mask).cpu(), torch.as_tensor(y).cpu()
    loss = torch.nn.functional.nll_loss(lp[mask], y[mask])
    loss.backward()
    return lp.detach(), {k: v.grad for k, v in leaves.items()}
