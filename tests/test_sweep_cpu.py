"""The sweep cut without a GPU: tests/sweep_ref.py (what the GPU tests compare with, bit for bit) against a brute-force count by
set membership, the four graphs of DESIGN §4.7's table from a dense eigh, and the call surface."""
import os
import re

import numpy as np
import pytest

import spectral_ref
import sweep_ref
from conftest import REPO


def small_graphs():
    rng = np.random.Generator(np.random.PCG64(11))
    out = [spectral_ref.path(2), spectral_ref.path(5), spectral_ref.star(7), spectral_ref.cycle(9), spectral_ref.complete(6),
           spectral_ref.barbell(4, 3)]
    for n in (3, 8, 12, 12):
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < 0.35]
        out.append(spectral_ref._und(pairs, n) if pairs else (np.zeros((2, 0), dtype=np.int64), n))
    out.append((np.zeros((2, 0), dtype=np.int64), 4))   # no edges: every value inf
    return out


@pytest.mark.parametrize('definition', ['reference', 'conductance'])
def test_difference_arrays_equal_brute_force(definition):
    rng = np.random.Generator(np.random.PCG64(5))
    for ei, n in small_graphs():
        for score in (rng.standard_normal(n), rng.integers(0, 3, n).astype(np.float64), np.zeros(n),
                      np.where(np.arange(n) % 2 == 0, -0.0, 0.0), -np.arange(n, dtype=np.float64)):
            a, b = sweep_ref.sweep(ei, n, score, definition), sweep_ref.brute(ei, n, score, definition)
            assert a.value == b.value or (np.isinf(a.value) and np.isinf(b.value))
            assert a.size == b.size and np.array_equal(a.counts, b.counts) and np.array_equal(a.order, b.order)
            assert a.profile.tobytes() == b.profile.tobytes()
            assert a.profile.shape == (n - 1,) and a.counts.sum() == sweep_ref.undirected_edges(ei)[0].shape[0]


def test_keyed_edges_are_the_unique_rows():
    """sweep_ref.undirected_edges with the node count takes a sort of a * n + b in place of np.unique(axis=0) (which costs seconds
    on half a million nodes): the same arrays on every graph of this file, on an edge index with both directions, loops and
    repeats in any order, and the old code where the key cannot be used."""
    rng = np.random.Generator(np.random.PCG64(17))
    graphs = small_graphs() + [case[1] for case in sweep_ref.table_graphs()]
    assert len(graphs) >= 15
    for ei, n in graphs:
        messy = np.concatenate([ei[:, ::-1], ei[::-1], np.tile(np.arange(n), (2, 1)), ei[:, :3]], axis=1)[:, rng.permutation(2 * ei.shape[1] + n + min(3, ei.shape[1]))]
        for edges in (ei, messy):
            want = sweep_ref.undirected_edges(edges)
            got = sweep_ref.undirected_edges(edges, n)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype == np.int64 and np.array_equal(g, w)
        assert np.array_equal(want[0], sweep_ref.undirected_edges(ei)[0]) and np.array_equal(want[1], sweep_ref.undirected_edges(ei)[1])
    ei, n = spectral_ref.path(5)
    for unusable in (0, 3, 2 ** 31):   # no nodes, an id outside, a key past int64
        got = sweep_ref.undirected_edges(ei, unusable)
        assert np.array_equal(got[0], np.arange(4)) and np.array_equal(got[1], np.arange(1, 5))


def test_order_rules():
    score = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e308, -1e308, 0.0])
    assert sweep_ref.order_of(score).tolist() == [3, 7, 5, 0, 1, 8, 4, 6, 2]
    with pytest.raises(ValueError):
        sweep_ref.order_of(np.array([0.0, np.nan]))
    r = sweep_ref.sweep(np.zeros((2, 0), dtype=np.int64), 4, np.arange(4.0))
    assert np.isinf(r.value) and r.size == 1
    with pytest.raises(ValueError):
        sweep_ref.sweep(np.zeros((2, 0), dtype=np.int64), 1, np.zeros(1))


@pytest.mark.parametrize('case', sweep_ref.table_graphs(), ids=lambda c: c[0])
def test_table_from_dense_eigh(case):
    name, (ei, n), left, phi, best_k, right = case
    lam, score = sweep_ref.fiedler_score(ei, n)
    r = sweep_ref.sweep(ei, n, score, 'conductance')
    print(name, 'lambda1/2', lam / 2, 'sweep', r.value, 'k', r.size, 'sqrt(2 lambda1)', np.sqrt(2 * lam))
    assert lam / 2 < r.value < np.sqrt(2 * lam)
    assert abs(lam / 2 - left) <= 5e-3 * left and abs(np.sqrt(2 * lam) - right) <= 5e-3 * right   # the table prints 3-4 digits
    assert abs(r.value - phi) <= 5e-4 * phi
    if best_k is not None:
        assert r.size == best_k
    if name == 'barbell20_4':
        assert r.value == 1 / 385 and r.counts.tolist() in ([192, 1, 0, 192], [192, 0, 1, 192])


def test_call_surface():
    from dcr import _lib
    from dcr.graph import DcrGraph, SweepCut
    assert {'dcr_sweep_cut', 'dcr_fiedler_sweep'} <= set(_lib.SIGNATURES)
    header = open(os.path.join(REPO, 'include', 'dcr.h')).read()
    declared = set(re.findall(r'\b(dcr_[a-z0-9_]+)\s*\(', header))
    assert {'dcr_sweep_cut', 'dcr_fiedler_sweep'} <= declared and 'dcr_sweep_result' in header
    assert SweepCut._fields == ('value', 'size', 'counts', 'order', 'profile')
    assert callable(DcrGraph.sweep_cut) and callable(DcrGraph.fiedler_sweep)
    from experiment.cheeger_bounds import cheeger_sweep
    assert callable(cheeger_sweep)
