"""GPU parity of the GCN path at the two BASELINE.json configurations that had no test:

  configs[3]  Citeseer shape (N = 2,120, F = 3,703, hidden 64, 6 classes; hyper-parameters utils/hyperparams.py 'Citeseer')
              on a graph that has been through rewire('bfc', 84, 0.22, 180): logits and gradients within 1e-5 of a
              dense fp64 evaluation of models/gcn.py:32-44 with GCNConv's published formula;
  configs[4]  S1M (N = 1,000,000, E = 10 M, F = 256, hidden 128, 16 classes) on the REWIRED graph (round 4: three SDRF
              iterations, edge list equal to the C oracle's, tests/golden/sdrf_s1m_oracle.json): logits within 1e-5 of an fp64 evaluation
              (edge-list scatter, written here, independent of the product's CSR builder) on every row, and the
              row-partitioned two-rank model equal to the single-process one on sampled rows.

GCNConv is third-party (torch_geometric 2.0.3, absent from the reference tree and from this image): the fp64 restatement
of its formula is the check (parity unpinned by the reference itself)."""
import os

import numpy as np
import pytest
import torch

from gcn_fp64 import gcn_logits

pytestmark = pytest.mark.gpu


def _fp64_logits(weights, x, edge_index, n, chunk=4_000_000, edge_weight=None):
    """log_softmax(Â·relu(Â·(X·W1ᵀ) + b1)·W2ᵀ + b2) in float64, Â = D^-1/2 (A + I) D^-1/2 from the raw edge list (with
    ``edge_weight`` and the self-loops PyG's gcn_norm keeps: tests/gcn_fp64.py)."""
    return gcn_logits(weights, x, edge_index, n, edge_weight=edge_weight, chunk=chunk)


def test_citeseer_shape_on_a_rewired_graph_logits_and_gradients():
    from dcr import synthetic
    from dcr.data import Data, Dataset
    from models.gcn import GCN
    from rewiring.rewire import rewire
    from utils.hyperparams import hyperparams
    hp = hyperparams['Citeseer']
    n, n_feat, n_cls = 2120, 3703, 6
    ei, n = synthetic.powerlaw_graph(n, 2, seed=12345)
    np.random.seed(0)
    rewired = rewire(Data(edge_index=torch.from_numpy(ei), num_nodes=n), 'bfc', hp['max_iterations'], hp['removal_bound'],
                     hp['tau'])
    assert rewired.shape[1] != ei.shape[1] or not np.array_equal(rewired.numpy(), ei)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(n, n_feat, generator=g) < 0.0086).float()           # ~32 words per document, row-normalised
    x = x / x.sum(1, keepdim=True).clamp_min(1.0)
    y = torch.randint(0, n_cls, (n,), generator=g)
    train_mask = torch.rand(n, generator=g) < 0.3
    data = Data(x=x, edge_index=rewired, y=y, num_nodes=n, train_mask=train_mask).to('cuda')
    torch.manual_seed(1)
    model = GCN(Dataset(data, n_cls), hidden=[hp['hidden_dim']] * hp['hidden_depth'], dropout=hp['dropout']).cuda()
    model.eval()                                                        # (dropout off: a deterministic comparison)
    logits = model(data)
    loss = torch.nn.functional.nll_loss(logits[data.train_mask], data.y[data.train_mask])
    loss.backward()
    ref_w = [(l.lin.weight.detach().clone().double().requires_grad_(), l.bias.detach().clone().double().requires_grad_())
             for l in model.layers]
    want = _fp64_logits(ref_w, data.x, data.edge_index, n)
    torch.nn.functional.nll_loss(want[data.train_mask], data.y[data.train_mask]).backward()
    assert (logits.detach().double() - want.detach()).abs().max().item() < 1e-5
    for layer, (w, b) in zip(model.layers, ref_w):
        assert (layer.lin.weight.grad.double() - w.grad).abs().max().item() < 1e-5
        assert (layer.bias.grad.double() - b.grad).abs().max().item() < 1e-5


_S1M_REWIRED = {}


def _s1m_inputs(dev, ei=None):
    """configs[4] as BASELINE.json words it: the 1M-node / 10M-edge graph REWIRED (rewire('bfc', ...) with the loop parameters of
    tests/golden/sdrf_s1m_oracle.json: three iterations, tau = 163, bound 0.95, numpy seed 0), checked against the edge list the
    C oracle recorded for the same run (SHA-256 of the int64 edge_index), then the features.  ``ei``: that edge list, already
    checked (the two-rank workers get it from their parent)."""
    import hashlib
    import json
    from dcr import synthetic
    if ei is None:
        ei = _S1M_REWIRED.get('edge_index')   # (rewired once per session, kept in memory: nothing written outside the repository)
    if ei is None:
        from dcr.data import Data
        from rewiring.rewire import rewire
        fix = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sdrf_s1m_oracle.json')))
        raw, _ = synthetic.powerlaw_graph(fix['graph']['n'], fix['graph']['m'], seed=fix['graph']['seed'])
        np.random.seed(fix['numpy_seed'])
        ei = rewire(Data(edge_index=torch.from_numpy(raw), num_nodes=fix['graph']['n']), 'bfc', len(fix['iterations']),
                    fix['removal_bound'], fix['tau']).numpy()
        assert hashlib.sha256(np.ascontiguousarray(ei).tobytes()).hexdigest() == fix['final']['edge_index_sha256']
        assert ei.shape[1] // 2 == fix['final']['edges'] != raw.shape[1] // 2
        _S1M_REWIRED['edge_index'] = ei
    n = 1_000_000
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(n, 256, device=dev, generator=g)
    return torch.from_numpy(ei).to(dev), n, x


def _training_step_against_fp64(ei, n, x, n_cls, hidden, p, frac_train, tol=1e-5, route='dense'):
    """One training step (experiment/training_loop.py:48-54: model.train(), NLL on the training rows, backward) through the
    one-kernel first layer + the row-selected aggregation: logits of the training rows and dW1, db1, dW2, db2 against a float64
    evaluation from the raw edge list, <= tol of the largest reference entry.  The float64 side uses the product's OWN
    activation pattern (sign of the float32 pre-activation AND the keep mask of the same dropout call): a pre-activation within
    float32 rounding of zero would otherwise sit on the other side of the ReLU in float64, and one such row moves an entry of
    dW1 by ~1e-3 of its size (a few dozen of the 128 M elements at S1M do)."""
    import ctypes
    from dcr import _lib
    from dcr.data import Data, Dataset
    from models import gcn
    from models.gcn import GCN, _ReluDropoutFn
    dev = x.device
    g = torch.Generator(device=dev).manual_seed(4)
    y = torch.randint(0, n_cls, (n,), device=dev, generator=g)
    train_rows = torch.nonzero(torch.rand(n, device=dev, generator=g) < frac_train).flatten()
    data = Data(x=x, edge_index=ei, y=y, num_nodes=n)
    torch.manual_seed(2)
    model = GCN(Dataset(data, n_cls), hidden=[hidden], dropout=p).to(dev)
    with torch.no_grad():
        model.layers[0].bias.uniform_(-0.1, 0.1)
    model.train()
    assert gcn.first_layer_fused_ok(x, model.act_fn, model.layers[0], model.layers[1].lin)
    sparse = model.layers[0].sparse_input(x) is not None        # few non-zeros: Â·(X·W1ᵀ) over them, then the activation kernel
    assert sparse == (route == 'sparse'), (route, sparse)
    calls = {'n': 0}
    fn = gcn._SparseFirstFn if sparse else gcn._FirstLayerFn
    real = fn.apply

    def counting(*a):
        calls['n'] += 1
        return real(*a)
    fn.apply = staticmethod(counting)
    try:
        ctr = gcn._dropout_counter(dev)
        c0 = ctr.clone()
        logp = model(data, rows=train_rows)                     # (the last aggregation at the rows the loss reads: the epoch's route)
    finally:
        fn.apply = real
    assert calls['n'] == 1                                      # the first layer went through the route under test
    torch.nn.functional.nll_loss(logp, y[train_rows]).backward()
    got = {name: q.grad.double() for name, q in model.named_parameters()}
    # the product's activation pattern: the float32 pre-activation from the same kernel on the same inputs, the keep mask of
    # dropout call c0 from the stand-alone kernel (same Philox counters and bit layout: tests/test_gcn.py pins that)
    feats = x.shape[1]
    w1, b1, w2 = model.layers[0].lin.weight.detach(), model.layers[0].bias.detach(), model.layers[1].lin.weight.detach()
    if sparse:
        with torch.no_grad():
            pre = gcn._SparseFirstFn.apply(w1, b1, model.layers[0].sparse_input(x), model.layers[0]._cache_csr)
    else:
        ax = model.layers[0]._ax
        words = ctypes.c_int64()
        _lib.check(_lib.lib().dcr_relu_dropout_bits_words(n * hidden, ctypes.byref(words)))
        bits = torch.zeros(words.value, dtype=torch.int64, device=dev)
        pre = torch.empty(n, hidden, device=dev)
        z = torch.empty(n, n_cls, device=dev)
        ctr.copy_(c0)
        cur = torch.cuda.current_stream(dev).cuda_stream
        ws = gcn._first_layer_workspace(dev, cur, n, feats, hidden)
        _lib.check(_lib.lib().dcr_first_layer_fwd_ws_f32_dev(ax.data_ptr(), ax.stride(0), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), pre.data_ptr(),
                                                             z.data_ptr(), None, n_cls, bits.data_ptr(), None, n, feats, hidden, n_cls, p,
                                                             torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, 0, ctr.data_ptr(),
                                                             None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(),
                                                             ctypes.c_void_p(cur)))
        del bits, z
    ctr.copy_(c0)
    keep = _ReluDropoutFn.apply(torch.ones(n, hidden, device=dev), p) != 0
    pattern = ((pre > 0) & keep).double() / (1.0 - p)
    del pre, keep
    ref = [(l.lin.weight.detach().clone().double().requires_grad_(), l.bias.detach().clone().double().requires_grad_())
           for l in model.layers]
    (rw1, rb1), (rw2, rb2) = ref
    src, dst = ei[0], ei[1]
    loops = torch.arange(n, device=dev)
    src, dst = torch.cat([src, loops]), torch.cat([dst, loops])
    deg = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, dst, torch.ones_like(dst, dtype=torch.float64))
    val = deg.pow(-0.5)[src] * deg.pow(-0.5)[dst]

    def propagate(t, chunk=4_000_000):
        out = torch.zeros((n, t.shape[1]), dtype=torch.float64, device=dev)
        for s0 in range(0, src.shape[0], chunk):
            e = slice(s0, s0 + chunk)
            out = out.index_add(0, dst[e], t[src[e]] * val[e, None])
        return out
    with torch.no_grad():
        ax64 = propagate(x.double())                        # Â·X (a constant of the run: no gradient flows into it)
    h = (ax64 @ rw1.t() + rb1) * pattern
    out = torch.log_softmax(propagate(h @ rw2.t()) + rb2, dim=1)[train_rows]
    torch.nn.functional.nll_loss(out, y[train_rows]).backward()
    assert (logp.detach().double() - out.detach()).abs().max().item() < tol
    want = {'layers.0.lin.weight': rw1.grad, 'layers.0.bias': rb1.grad, 'layers.1.lin.weight': rw2.grad, 'layers.1.bias': rb2.grad}
    for name, w in want.items():
        err, scale = (got[name] - w).abs().max().item(), w.abs().max().item()
        assert got[name].shape == w.shape and err <= tol * scale, (name, err, scale)


def test_s1m_training_step_gradients_against_fp64():
    """configs[4], one training step at N = 1M on the rewired graph (round 5: the one-kernel backward had never been compared
    with anything at this size)."""
    dev = torch.device('cuda', 0)
    ei, n, x = _s1m_inputs(dev)
    _training_step_against_fp64(ei, n, x, 16, 128, 0.5, 0.1)


@pytest.mark.parametrize('route', ['dense', 'sparse'])
@pytest.mark.parametrize('name,n,n_feat,n_cls', [('Citeseer', 2120, 3703, 6), ('Cora', 2485, 1433, 7)])
def test_reference_dataset_shapes_training_step_through_the_one_kernel_first_layer(name, n, n_feat, n_cls, route, monkeypatch):
    """configs[3] (round 5): the reference's own dataset shapes — Citeseer 3,703 -> 64 -> 6, Cora 1,433 -> 128 -> 7, hidden widths,
    dropout and rewiring parameters from utils/hyperparams.py — take the one-kernel first layer (W1 streamed through LDS in K
    chunks; before, the GEMM library): a training step on the REWIRED graph, logits and all four gradients <= 1e-5 of a float64
    evaluation.  Features: a row-normalised bag of words of Planetoid's density (the datasets themselves are not in the image)."""
    from dcr import synthetic
    from dcr.data import Data
    from rewiring.rewire import rewire
    from utils.hyperparams import hyperparams
    hp = hyperparams[name]
    ei, n = synthetic.powerlaw_graph(n, 2, seed=12345)
    np.random.seed(0)
    rewired = rewire(Data(edge_index=torch.from_numpy(ei), num_nodes=n), 'bfc', hp['max_iterations'], hp['removal_bound'], hp['tau'])
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(n, n_feat, generator=g) < 0.0086).float()
    x = x / x.sum(1, keepdim=True).clamp_min(1.0)
    # route 'dense': the K-chunked MFMA kernel on Â·X (DCR_SPARSE_X=0); 'sparse' (the default for such features): Â·(X·W1ᵀ) over
    # the non-zeros of X, then the fused activation kernel — "measure both orders and keep the faster" (bench.py reports both)
    monkeypatch.setenv('DCR_SPARSE_X', '0' if route == 'dense' else '0.1')
    _training_step_against_fp64(rewired.cuda(), n, x.cuda(), n_cls, hp['hidden_dim'], hp['dropout'], 0.3, route=route)


def _s1m_worker(rank, world, port, rows_path, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        dist.all_gather_into_tensor(torch.empty(8, device='cuda'), torch.ones(4, device='cuda'))
    except Exception as e:  # noqa: BLE001  (this torch build's gloo cannot move device tensors)
        ret[rank] = ('unsupported', str(e))
        dist.destroy_process_group()
        return
    from dcr.data import Data, Dataset
    from models.gcn import GCN
    from models.gcn_dp import ShardedGCN
    dev = torch.device('cuda', 0)
    saved = torch.load(rows_path)
    ei, n, x = _s1m_inputs(dev, saved['edge_index'].numpy())
    torch.manual_seed(2)
    model = GCN(Dataset(Data(x=x, edge_index=ei, num_nodes=n), 16), hidden=[128], dropout=0.5).to(dev)
    sh = ShardedGCN(model, ei, n)
    sh.eval()
    with torch.no_grad():
        local = sh(sh.shard(x))
    rows, want = saved['rows'].to(dev), saved['logits'].to(dev)
    where = torch.full((n,), -1, dtype=torch.int64, device=dev)      # position of a node inside this rank's block, or -1
    where[sh.owned] = torch.arange(sh.owned.shape[0], device=dev)
    mine = where[rows] >= 0
    err = (local[where[rows[mine]]] - want[mine]).abs().max().item() if bool(mine.any()) else 0.0
    ret[rank] = (err, int(mine.sum()))
    dist.destroy_process_group()


def test_s1m_logits_fp64_check_and_two_rank_equality(tmp_path):
    import socket
    import torch.multiprocessing as mp
    from dcr.data import Data, Dataset
    from models.gcn import GCN
    dev = torch.device('cuda', 0)
    ei, n, x = _s1m_inputs(dev)
    torch.manual_seed(2)
    model = GCN(Dataset(Data(x=x, edge_index=ei, num_nodes=n), 16), hidden=[128], dropout=0.5).to(dev)
    model.eval()
    with torch.no_grad():
        got = model(Data(x=x, edge_index=ei, num_nodes=n))
        want = _fp64_logits([(l.lin.weight, l.bias) for l in model.layers], x, ei, n)
    err = (got.double() - want).abs().max().item()
    assert err < 1e-5, err
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(9))[:2000]
    rows_path = str(tmp_path / 'rows.pt')
    torch.save({'rows': rows, 'logits': got[rows.to(dev)].cpu(), 'edge_index': ei.cpu()}, rows_path)
    del got, want, model, x, ei
    torch.cuda.empty_cache()
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ret = mp.Manager().dict()
    mp.spawn(_s1m_worker, args=(2, port, rows_path, ret), nprocs=2, join=True)
    assert len(ret) == 2
    if any(v[0] == 'unsupported' for v in ret.values()):
        pytest.skip(f'gloo cannot move device tensors in this torch build: {dict(ret)}')
    assert sum(v[1] for v in ret.values()) == 2000
    for rank, (e, cnt) in ret.items():
        assert e < 1e-5, (rank, e, cnt)   # same kernels on a row block: the first-layer GEMM tiles differently, hence not 0
