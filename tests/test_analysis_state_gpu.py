"""The analysis buffers of a graph (AnalysisState of csrc/dcr_analysis.h): destroying a graph gives back every buffer the analysis
calls grew on it.  No solve needs to converge here: the test reads the device's free memory."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dcr():
    from dcr.graph import DcrGraph
    return DcrGraph


def test_destroy_gives_every_buffer_back(dcr):
    import torch
    from dcr import synthetic
    n = 20000
    ei, _ = synthetic.powerlaw_graph(n, 2, seed=11)
    rng = np.random.default_rng(6)
    pairs = rng.integers(0, n, size=(32, 2))
    s64 = rng.choice(n, 64, replace=False)
    x = rng.standard_normal(n)

    def cycle():
        G = dcr(ei, n)
        G.resistance_sketch(columns=64, edges=True, pairs=pairs, tol=1e-6, max_steps=16)
        G.ppr(s64[:32], max_steps=16)
        G.hop_summary(s64)
        G.betweenness(sources=s64[:16], edges=True)
        G.spectral_gap(max_steps=24)
        G.fosr_pick(x)
        G.close()

    sketch_workspace = 4 * 6 * n * 16 * 8     # bytes of one cycle's largest buffer: four groups of six [n][16] float64 vectors
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)   # cut short on purpose
        cycle()                               # what the runtime and the first use of every kernel keep is paid here
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        for _ in range(20):
            cycle()
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
    print(f'  free memory: {before} before, {after} after 20 cycles, dropped {before - after}; one sketch workspace {sketch_workspace}')
    assert before - after < sketch_workspace
