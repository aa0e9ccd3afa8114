"""bench.py --dump-outputs: the files it writes (float32 / float64 .npy), their contents, and the fixed sample above the size
cap, on a stand-in for the SDRF run (no GPU: dump_outputs only reads the graph through to_edge_index / curvature_read)."""
import os

import numpy as np

import bench


class _Graph:
    def __init__(self, n, n_edges, seed=0):
        rng = np.random.default_rng(seed)
        self.n = n
        self.u = rng.integers(0, n, n_edges).astype(np.int32)
        self.v = rng.integers(0, n, n_edges).astype(np.int32)
        self.cv = rng.standard_normal(n_edges)

    def number_of_nodes(self):
        return self.n

    def to_edge_index(self):
        return np.stack([np.concatenate([self.u, self.v]), np.concatenate([self.v, self.u])]).astype(np.int64)

    def curvature_read(self):
        return self.u.copy(), self.v.copy(), self.cv.copy()


class _Run:
    def __init__(self, G, last):
        self.G, self.last = G, last


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_what_the_last_step_left(tmp_path):
    G = _Graph(1000, 5000)
    bench.dump_outputs(str(tmp_path), _Run(G, (3, 7, 42)))
    got = _load(str(tmp_path))
    assert sorted(got) == ['curvature', 'edge_index', 'last_step']
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got['edge_index'], G.to_edge_index())
    assert np.array_equal(got['curvature'], np.stack([G.u, G.v, G.cv]))
    assert got['curvature'].dtype == np.float64
    assert got['last_step'].tolist() == [3.0, 7.0, 42.0]


def test_dump_over_the_cap_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 64 << 10)
    G = _Graph(1000, 20000)
    a, b = tmp_path / 'a', tmp_path / 'b'
    np.random.seed(5)
    state = np.random.get_state()
    bench.dump_outputs(str(a), _Run(G, (None, None, None)))
    assert np.array_equal(np.random.get_state()[1], state[1])   # the SDRF draw's stream is left alone
    bench.dump_outputs(str(b), _Run(G, (None, None, None)))
    ga, gb = _load(str(a)), _load(str(b))
    assert sum(os.path.getsize(os.path.join(str(a), f)) for f in os.listdir(str(a))) <= (64 << 10) + 3 * 256
    for k in ga:
        assert np.array_equal(ga[k], gb[k], equal_nan=True)
    full = np.stack([G.u, G.v, G.cv])
    cols = ga['curvature']
    assert 0 < cols.shape[1] < full.shape[1]
    # every sampled column is a column of the full array, in their order
    pos = [int(np.flatnonzero((full[0] == c[0]) & (full[1] == c[1]) & (full[2] == c[2]))[0]) for c in cols.T[:50]]
    assert pos == sorted(pos)
    assert np.isnan(ga['last_step']).all()
