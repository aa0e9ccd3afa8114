"""experiment/adam.py::OneLaunchAdam (dcr_adam_step_f32_dev) against torch.optim.Adam's update rule in float64
(tests/gcn_fp64.py::adam_fp64): 1, 8, 9 and 17 tensors (one, two and three launches per step, the step counter rewound
between them) beside a zero-element tensor, a parameter without a gradient, more than 262,144 elements (the grid-stride path past
1,024 workgroups), 300 steps (the bias correction into its tail); a captured step replayed against eager steps; and a run
saved and resumed, from its own state or from torch.optim.Adam's, and torch.optim.Adam resumed from its state."""
import io

import pytest
import torch

from gcn_fp64 import adam_fp64

pytestmark = pytest.mark.gpu

LR, BETAS, EPS = 0.01, (0.9, 0.999), 1e-8


def _shapes(n_tensors):
    """``n_tensors`` tensors the kernel updates (the 8th brings the total past 262,144 elements), then a zero-element tensor and
    one more (whose gradient the callers may leave None)."""
    shapes = [(37, 19), (64,), (5, 3), (130,), (7, 7, 3), (1,), (2,), (300, 1001)]
    return [shapes[i] if i < 8 else (11 + i, 4) for i in range(n_tensors)] + [(0,), (33,)]


def _build(n_tensors, seed=6, cls=None, **kw):
    from experiment.adam import OneLaunchAdam
    g = torch.Generator(device='cuda').manual_seed(seed)
    ps = [(torch.randn(*s, device='cuda', generator=g) * 0.1).requires_grad_(True) for s in _shapes(n_tensors)]
    half = (len(ps) + 1) // 2
    groups = [{'params': ps[:half], 'weight_decay': 5e-3}]
    if ps[half:]:
        groups.append({'params': ps[half:], 'weight_decay': 0.0})
    return ps, (cls or OneLaunchAdam)(groups, lr=LR, betas=BETAS, eps=EPS, **kw)


def _grads(ps, g, skip=None):
    return [None if i == skip else torch.randn(p.shape, device='cuda', generator=g) for i, p in enumerate(ps)]


@pytest.mark.parametrize('n_tensors', [1, 8, 9, 17])
def test_one_launch_adam_against_fp64(n_tensors):
    ps, opt = _build(n_tensors)
    skip = len(ps) - 1                                               # a parameter whose grad stays None
    assert sum(p.numel() for p in ps) > 262_144 or n_tensors < 8
    ref = [[p.detach().double().clone(), torch.zeros_like(p, dtype=torch.float64), torch.zeros_like(p, dtype=torch.float64)]
           for p in ps]
    wds = [gr['weight_decay'] for gr in opt.param_groups for _ in gr['params']]
    g = torch.Generator(device='cuda').manual_seed(9)
    p_skip = ps[skip].detach().clone()
    for t in range(1, 301):
        grads = _grads(ps, g, skip)
        for p, gr in zip(ps, grads):
            p.grad = gr
        opt.step()
        for r, gr, wd in zip(ref, grads, wds):
            if gr is not None:
                r[0], r[1], r[2] = adam_fp64(r[0], gr, r[1], r[2], t, LR, BETAS, EPS, wd)
        if t in (1, 2, 10, 100, 300):
            assert float(opt._step) == t
            for i, (p, r) in enumerate(zip(ps, ref)):
                if i == skip or p.numel() == 0:
                    continue
                st = opt.state[p]
                # float32 against float64: the moments stay within a few roundings of their size, the parameters drift by
                # at most a rounding of the step and of the parameter per step
                gmax = max(1.0, r[1].abs().max().item())
                assert (st['exp_avg'].double() - r[1]).abs().max().item() <= 2e-6 * gmax * (1 + t / 100), (t, i)
                assert (st['exp_avg_sq'].double() - r[2]).abs().max().item() <= 4e-6 * max(1.0, r[2].abs().max().item()) * (1 + t / 100), (t, i)
                err = (p.detach().double() - r[0]).abs().max().item()
                assert err <= t * (4e-6 * LR + 2e-7 * max(1.0, r[0].abs().max().item())), (t, i, err)
    assert torch.equal(ps[skip].detach(), p_skip) and not opt.state.get(ps[skip])


def test_captured_step_equals_eager_steps_nine_tensors():
    ps_c, opt_c = _build(9)
    ps_e, opt_e = _build(9)
    g = torch.Generator(device='cuda').manual_seed(4)
    seq = [_grads(ps_c, g) for _ in range(6)]
    static = [torch.zeros_like(p) for p in ps_c]
    for p, s in zip(ps_c, static):
        p.grad = s
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s, src in zip(static, seq[0]):
            s.copy_(src)
        opt_c.step()                                 # (eager: the state comes into being)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        opt_c.step()
    for k in range(1, 6):
        for s, src in zip(static, seq[k]):
            s.copy_(src)
        graph.replay()
    torch.cuda.synchronize()
    for k in range(6):
        for p, gr in zip(ps_e, seq[k]):
            p.grad = gr.clone()
        opt_e.step()
    assert float(opt_c._step) == float(opt_e._step) == 6.0
    for a, b in zip(ps_c, ps_e):
        assert torch.equal(a, b)
        assert torch.equal(opt_c.state[a]['exp_avg'], opt_e.state[b]['exp_avg'])
        assert torch.equal(opt_c.state[a]['exp_avg_sq'], opt_e.state[b]['exp_avg_sq'])


def _saved(opt, ps):
    buf = io.BytesIO()
    torch.save({'opt': opt.state_dict(), 'params': [p.detach().clone() for p in ps]}, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


@pytest.mark.parametrize('n_tensors', [4, 9])
def test_resumed_run_equals_the_uninterrupted_run(n_tensors):
    from experiment.adam import OneLaunchAdam
    g = torch.Generator(device='cuda').manual_seed(5)
    ps, opt = _build(n_tensors)
    seq = [_grads(ps, g) for _ in range(12)]
    for k in range(12):
        for p, gr in zip(ps, seq[k]):
            p.grad = gr.clone()
        opt.step()
    ps2, opt2 = _build(n_tensors)
    for k in range(5):
        for p, gr in zip(ps2, seq[k]):
            p.grad = gr.clone()
        opt2.step()
    emitted = opt2.state_dict()['state']
    assert len({id(s['step']) for s in emitted.values()}) == len(emitted) == len(ps2)      # one tensor per parameter
    assert all(s['step'] is not opt2._step for s in emitted.values())
    saved = _saved(opt2, ps2)
    assert all(float(s['step']) == 5.0 for s in saved['opt']['state'].values())
    ps3 = [t.clone().requires_grad_(True) for t in saved['params']]
    half = (len(ps3) + 1) // 2
    opt3 = OneLaunchAdam([{'params': ps3[:half], 'weight_decay': 5e-3}, {'params': ps3[half:], 'weight_decay': 0.0}],
                         lr=LR, betas=BETAS, eps=EPS)
    opt3.load_state_dict(saved['opt'])
    assert float(opt3._step) == 5.0
    for k in range(5, 12):
        for p, gr in zip(ps3, seq[k]):
            p.grad = gr.clone()
        opt3.step()
    assert float(opt3._step) == 12.0
    for a, b in zip(ps, ps3):
        assert torch.equal(a, b)


def test_resume_from_torch_adam_state():
    from experiment.adam import OneLaunchAdam
    g = torch.Generator(device='cuda').manual_seed(7)
    ps_t, opt_t = _build(9, cls=torch.optim.Adam)
    seq = [_grads(ps_t, g) for _ in range(10)]
    for k in range(4):
        for p, gr in zip(ps_t, seq[k]):
            p.grad = gr.clone()
        opt_t.step()
    saved = _saved(opt_t, ps_t)
    ps_o = [t.clone().requires_grad_(True) for t in saved['params']]
    half = (len(ps_o) + 1) // 2
    opt_o = OneLaunchAdam([{'params': ps_o[:half], 'weight_decay': 5e-3}, {'params': ps_o[half:], 'weight_decay': 0.0}],
                          lr=LR, betas=BETAS, eps=EPS)
    opt_o.load_state_dict(saved['opt'])
    assert float(opt_o._step) == 4.0 and all(gr['capturable'] for gr in opt_o.param_groups)
    for k in range(4, 10):
        for p, q, gr in zip(ps_t, ps_o, seq[k]):
            p.grad, q.grad = gr.clone(), gr.clone()
        opt_t.step()
        opt_o.step()
    assert float(opt_o._step) == 10.0
    for p, q in zip(ps_t, ps_o):
        if p.numel() == 0:
            continue
        assert (p - q).abs().max().item() <= 2e-6 * max(1.0, p.abs().max().item())
        assert (opt_t.state[p]['exp_avg'] - opt_o.state[q]['exp_avg']).abs().max().item() <= 1e-6
        assert (opt_t.state[p]['exp_avg_sq'] - opt_o.state[q]['exp_avg_sq']).abs().max().item() <= 1e-6


def test_torch_adam_resumes_from_one_launch_adam_state():
    """The other way round: torch.optim.Adam (the default optimiser) loads a OneLaunchAdam state and continues within float32
    rounding of OneLaunchAdam itself — every parameter's 'step' advances once per step, not once per parameter sharing it."""
    g = torch.Generator(device='cuda').manual_seed(8)
    ps_o, opt_o = _build(9)
    seq = [_grads(ps_o, g) for _ in range(10)]
    for k in range(4):
        for p, gr in zip(ps_o, seq[k]):
            p.grad = gr.clone()
        opt_o.step()
    saved = _saved(opt_o, ps_o)
    ps_t = [t.clone().requires_grad_(True) for t in saved['params']]
    half = (len(ps_t) + 1) // 2
    opt_t = torch.optim.Adam([{'params': ps_t[:half], 'weight_decay': 5e-3}, {'params': ps_t[half:], 'weight_decay': 0.0}],
                             lr=LR, betas=BETAS, eps=EPS)
    opt_t.load_state_dict(saved['opt'])      # (the saved groups bring capturable=True with them: the counters stay on the device)
    for k in range(4, 10):
        for p, q, gr in zip(ps_o, ps_t, seq[k]):
            p.grad, q.grad = gr.clone(), gr.clone()
        opt_o.step()
        opt_t.step()
    assert float(opt_o._step) == 10.0
    assert all(float(opt_t.state[q]['step']) == 10.0 for q in ps_t)
    for p, q in zip(ps_o, ps_t):
        if p.numel() == 0:
            continue
        assert (p - q).abs().max().item() <= 2e-6 * max(1.0, p.abs().max().item())
        assert (opt_o.state[p]['exp_avg'] - opt_t.state[q]['exp_avg']).abs().max().item() <= 1e-6
