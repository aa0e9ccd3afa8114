"""Device-resident graph handle: the host-side mirror of the slice of
``networkx.Graph`` the reference's curvature / SDRF code uses
(rewiring/sdrf_no_cuda.py:20-68, curvature/bfc_naive.py:7-52)."""
import ctypes
import warnings
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib

CURV = {'bfc': 0, '1d': 1, 'augmented': 2, 'haantjes': 3}


def curv_code(curv_type):
    try:
        return CURV[curv_type]
    except KeyError:
        # classical_curvatures.py:28 raises a bare Exception with this text
        raise Exception(f'Method {curv_type} not available.')


def _as_numpy_edge_index(edge_index):
    if hasattr(edge_index, 'detach'):
        edge_index = edge_index.detach().cpu().numpy()
    ei = np.ascontiguousarray(np.asarray(edge_index), dtype=np.int64)
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise ValueError('edge_index must have shape [2, M]')
    return ei


CHEEGER_DEFINITIONS = {'reference': 0, 'conductance': 1}

# what DcrGraph.spectral_gap returns; ``vector`` is None unless it was asked for
SpectralGap = namedtuple('SpectralGap', ['lambda1', 'residual', 'steps', 'restarts', 'components', 'converged', 'vector'],
                         defaults=[None])

# what DcrGraph.sweep_cut returns: the best prefix S_size of the order, its value, counts = int64 [4] (in, lo, hi, out);
# ``order`` / ``profile`` are None unless asked for
SweepCut = namedtuple('SweepCut', ['value', 'size', 'counts', 'order', 'profile'])


# pairs of one batch of DcrGraph.effective_resistance: COL_B (DCR_COL_B) of the column CG in csrc/dcr_analysis.h
RESISTANCE_BATCH = 16
# columns of one batch of DcrGraph.ppr, DcrGraph.heat and DcrGraph.diffusion: the same COL_B
DIFFUSION_BATCH = 16
# ranks one LDS window of the FoSR pick covers on a row above 2,048 neighbours: FSR_WINDOW of csrc/dcr_fosr.hip
FOSR_WINDOW = 4096


def pack_members(members, num_nodes):
    """(uint64 words [n, W], number of subsets) from bool ``[B, n]`` or from the packed words themselves."""
    m = np.asarray(members)
    if m.ndim != 2:
        raise ValueError('members must be bool [B, n] or uint64 [n, W]')
    if m.dtype == np.uint64:
        if m.shape[0] != num_nodes or m.shape[1] < 1:
            raise ValueError('packed members must have shape [num_nodes, W] with W >= 1')
        return np.ascontiguousarray(m), 64 * m.shape[1]
    if m.dtype != np.bool_:
        raise ValueError('members must be bool [B, n] or uint64 [n, W]')
    B = m.shape[0]
    if B < 1 or m.shape[1] != num_nodes:
        raise ValueError('bool members must have shape [B, num_nodes] with B >= 1')
    W = (B + 63) // 64
    bits = np.zeros((num_nodes, 64 * W), dtype=np.uint8)
    bits[:, :B] = m.T
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder='little')).view('<u8').reshape(num_nodes, W), B


def _with_outside(counts3, num_edges):
    out = np.empty((counts3.shape[0], 4), dtype=np.int64)
    out[:, :3] = counts3
    out[:, 3] = num_edges - counts3.sum(axis=1)
    return out


class _HostBlock:
    """Carrier of an ``__array_interface__`` for a library-owned host buffer."""
    __slots__ = ('__array_interface__',)


def _host_view(ptr, n, typestr):
    """numpy view of n elements at a ctypes pointer.  (``np.ctypeslib.as_array(ptr, shape)`` builds a new ctypes array
    type for every distinct n, ~0.3 ms per call: more than the improvement kernels take.)"""
    blk = _HostBlock()
    blk.__array_interface__ = {'data': (ctypes.cast(ptr, ctypes.c_void_p).value, False), 'shape': (int(n),),
                               'typestr': typestr, 'version': 3}
    return np.asarray(blk)

class DcrGraph:
    """Undirected simple graph on nodes 0..n-1 living in HBM.

    Construction follows ``to_networkx(data, to_undirected=True)``
    (sdrf_no_cuda.py:20): pairs with dst <= src are kept, in order; adjacency
    rows keep insertion order, which fixes ``G.edges`` order and every
    first-extremum tie-break of the SDRF loop.
    """

    def __init__(self, edge_index, num_nodes, device=0):
        ei = _as_numpy_edge_index(edge_index)
        src = np.ascontiguousarray(ei[0])
        dst = np.ascontiguousarray(ei[1])
        self._h = ctypes.c_void_p()
        self.num_nodes = int(num_nodes)
        rc = lib().dcr_graph_create(int(device), self.num_nodes, src.shape[0],
                                    src.ctypes.data_as(_lib._i64p), dst.ctypes.data_as(_lib._i64p),
                                    ctypes.byref(self._h))
        if rc != 0:
            h, self._h = self._h, ctypes.c_void_p()
            msg = lib().dcr_last_error().decode()
            if h:
                lib().dcr_graph_destroy(h)
            if rc == -1:
                raise ValueError(msg)
            raise _lib.DcrError(f'libdcr_hip error {rc}: {msg}')

    @classmethod
    def from_data(cls, data, device=0):
        return cls(data.edge_index, data.num_nodes, device=device)

    def close(self):
        if getattr(self, '_h', None):
            lib().dcr_graph_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- container -----------------------------------------------------------------
    def number_of_nodes(self):
        return self.num_nodes

    def number_of_edges(self):
        out = ctypes.c_int64()
        check(lib().dcr_graph_num_edges(self._h, ctypes.byref(out)))
        return out.value

    def add_edge(self, u, v):
        check(lib().dcr_graph_add_edge(self._h, int(u), int(v)))

    def remove_edge(self, u, v):
        check(lib().dcr_graph_remove_edge(self._h, int(u), int(v)))

    def has_edge(self, u, v):
        out = ctypes.c_int()
        check(lib().dcr_graph_has_edge(self._h, int(u), int(v), ctypes.byref(out)))
        return bool(out.value)

    def degree(self, u):
        out = ctypes.c_int32()
        check(lib().dcr_graph_degree(self._h, int(u), ctypes.byref(out)))
        return out.value

    def neighbors(self, u):
        d = self.degree(u)
        buf = np.empty(max(d, 1), dtype=np.int32)
        n = ctypes.c_int64()
        check(lib().dcr_graph_neighbors(self._h, int(u), buf.shape[0], buf.ctypes.data_as(_lib._i32p),
                                        ctypes.byref(n)))
        return buf[:n.value].tolist()

    def edges(self):
        """(u, v) arrays in ``G.edges`` order."""
        ne = self.number_of_edges()
        eu = np.empty(ne, dtype=np.int32)
        ev = np.empty(ne, dtype=np.int32)
        check(lib().dcr_graph_edges(self._h, eu.ctypes.data_as(_lib._i32p), ev.ctypes.data_as(_lib._i32p)))
        return eu, ev

    def to_edge_index(self):
        """``from_networkx(G).edge_index`` as int64 numpy [2, 2E] (sdrf_no_cuda.py:68)."""
        out = np.empty((2, 2 * self.number_of_edges()), dtype=np.int64)
        check(lib().dcr_graph_export_edge_index(self._h, out.ctypes.data_as(_lib._i64p)))
        return out

    # ---- curvature -------------------------------------------------------------------
    def curvature_pass(self, curv_type='bfc', incremental=False):
        fn = lib().dcr_curvature_pass_incremental if incremental else lib().dcr_curvature_pass
        check(fn(self._h, curv_code(curv_type)))

    def curvature_pass_argmin(self, curv_type='bfc', incremental=False):
        """One pass, then the first minimum in ``G.edges`` order: (u, v, value), one host synchronisation."""
        u, v, val = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        check(lib().dcr_curvature_pass_argmin(self._h, curv_code(curv_type), int(bool(incremental)), ctypes.byref(u),
                                              ctypes.byref(v), ctypes.byref(val)))
        return u.value, v.value, val.value

    def curvature_read(self):
        ne = self.number_of_edges()
        cv = np.empty(ne, dtype=np.float64)
        eu = np.empty(ne, dtype=np.int32)
        ev = np.empty(ne, dtype=np.int32)
        check(lib().dcr_curvature_read(self._h, cv.ctypes.data_as(_lib._f64p), eu.ctypes.data_as(_lib._i32p),
                                       ev.ctypes.data_as(_lib._i32p)))
        return eu, ev, cv

    def curvature_all(self, curv_type='bfc'):
        self.curvature_pass(curv_type)
        return self.curvature_read()

    def curvature_edge(self, u, v, curv_type='bfc'):
        out = ctypes.c_double()
        check(lib().dcr_curvature_edge(self._h, int(u), int(v), curv_code(curv_type), ctypes.byref(out)))
        return out.value

    def bfc_ingredients(self, u, v):
        out = np.empty(6, dtype=np.int64)
        check(lib().dcr_bfc_ingredients(self._h, int(u), int(v), out.ctypes.data_as(_lib._i64p)))
        return out

    def argext(self, want_max, exclude=None):
        u, v, val = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        eu, ev = (-1, -1) if exclude is None else (int(exclude[0]), int(exclude[1]))
        check(lib().dcr_argext(self._h, int(bool(want_max)), eu, ev, ctypes.byref(u), ctypes.byref(v),
                               ctypes.byref(val)))
        return u.value, v.value, val.value

    def improvements(self, x, y, curv_type='bfc', want_candidates=False):
        """Returns (improvements view, ci, cj); the arrays are views of library-owned pinned
        buffers, valid until the next call on this graph."""
        n = ctypes.c_int64()
        pi, pci, pcj = _lib._f64p(), _lib._i32p(), _lib._i32p()
        check(lib().dcr_improvements(self._h, int(x), int(y), curv_code(curv_type), int(bool(want_candidates)),
                                     ctypes.byref(n), ctypes.byref(pi), ctypes.byref(pci), ctypes.byref(pcj)))
        if n.value == 0:
            e = np.empty(0, dtype=np.float64)
            return e, np.empty(0, dtype=np.int32), np.empty(0, dtype=np.int32)
        imp = _host_view(pi, n.value, '<f8')
        ci = cj = None
        if want_candidates:
            ci = _host_view(pci, n.value, '<i4')
            cj = _host_view(pcj, n.value, '<i4')
        return imp, ci, cj

    def improvements_count(self, x, y, curv_type='bfc'):
        """Run the improvement pipeline but leave the values on the device (tau = inf path)."""
        n = ctypes.c_int64()
        check(lib().dcr_improvements(self._h, int(x), int(y), curv_code(curv_type), 0, ctypes.byref(n), None, None,
                                     None))
        return n.value

    def improvements_argmax(self):
        out = ctypes.c_int64()
        check(lib().dcr_improvements_argmax(self._h, ctypes.byref(out)))
        return out.value

    def candidate_at(self, index):
        i, j = ctypes.c_int32(), ctypes.c_int32()
        check(lib().dcr_candidate_at(self._h, int(index), ctypes.byref(i), ctypes.byref(j)))
        return i.value, j.value

    def sdrf_tail(self, add, do_remove, removal_bound):
        k, l = (-1, -1) if add is None else (int(add[0]), int(add[1]))
        removed = (ctypes.c_int32 * 2)(-1, -1)
        mx = ctypes.c_double()
        check(lib().dcr_sdrf_tail(self._h, k, l, int(bool(do_remove)), float(removal_bound), removed,
                                  ctypes.byref(mx)))
        rem = None if removed[0] < 0 else (removed[0], removed[1])
        return rem, mx.value

    def sdrf_tail_at(self, cand_index, do_remove, removal_bound):
        """``sdrf_tail`` with the edge to add given by its index in the last candidate list; returns
        (added pair, removed pair or None, stale maximum)."""
        added = (ctypes.c_int32 * 2)(-1, -1)
        removed = (ctypes.c_int32 * 2)(-1, -1)
        mx = ctypes.c_double()
        check(lib().dcr_sdrf_tail_at(self._h, int(cand_index), int(bool(do_remove)), float(removal_bound), added, removed,
                                     ctypes.byref(mx)))
        rem = None if removed[0] < 0 else (removed[0], removed[1])
        return (added[0], added[1]), rem, mx.value

    def sdrf_tail_at_pass_argmin(self, cand_index, do_remove, removal_bound, curv_type='bfc', incremental=False):
        """``sdrf_tail_at`` and the next iteration's ``curvature_pass_argmin`` with one host synchronisation; returns
        (added pair, removed pair or None, (u, v, value) of the next first minimum)."""
        added = (ctypes.c_int32 * 2)(-1, -1)
        removed = (ctypes.c_int32 * 2)(-1, -1)
        u, v, val = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        check(lib().dcr_sdrf_tail_at_pass_argmin(self._h, int(cand_index), int(bool(do_remove)), float(removal_bound),
                                                 curv_code(curv_type), int(bool(incremental)), added, removed,
                                                 ctypes.byref(u), ctypes.byref(v), ctypes.byref(val)))
        rem = None if removed[0] < 0 else (removed[0], removed[1])
        return (added[0], added[1]), rem, (u.value, v.value, val.value)

    def sdrf_iteration_device_draw(self, x, y, curv_type, tau, uniform, do_remove, removal_bound, incremental=False):
        """One loop iteration for the edge (x, y) with the draw on the device and one host synchronisation
        (``dcr_sdrf_iteration_device_draw``); returns (status, candidates, added pair, removed pair or None, (u, v, value) of the
        next first minimum).  status != 0: nothing was edited (1: the draw was left undecided, 2: no candidates)."""
        status, n_cand = ctypes.c_int(), ctypes.c_int64()
        added = (ctypes.c_int32 * 2)(-1, -1)
        removed = (ctypes.c_int32 * 2)(-1, -1)
        u, v, val = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        check(lib().dcr_sdrf_iteration_device_draw(self._h, int(x), int(y), curv_code(curv_type), float(tau), float(uniform),
                                                   int(bool(do_remove)), float(removal_bound), int(bool(incremental)),
                                                   ctypes.byref(status), ctypes.byref(n_cand), added, removed,
                                                   ctypes.byref(u), ctypes.byref(v), ctypes.byref(val)))
        rem = None if removed[0] < 0 else (removed[0], removed[1])
        return status.value, n_cand.value, (added[0], added[1]), rem, (u.value, v.value, val.value)

    # ---- Monte-Carlo Cheeger estimate (experiment/compute_cheeger.py) ------------------------------------------------
    def cheeger_counts(self, members):
        """Edge counts of many node subsets at once, read-only on the graph.  ``members``: bool ``[B, n]`` (row = subset) or
        the packed words themselves, uint64 ``[n, W]`` (bit k of word w of node v = v is in subset 64 w + k; B = 64 W).
        Returns int64 ``[B, 4]`` = (in, lo, hi, out) over the undirected edges a < b: both ends inside, only a, only b,
        neither (compute_cheeger.py:32-45: boundary_size = lo, vol(S) = 2 in, vol(G - S) = 2 out)."""
        words, B = pack_members(members, self.num_nodes)
        out = np.empty((64 * words.shape[1], 3), dtype=np.int64)
        check(lib().dcr_cheeger_counts(self._h, words.ctypes.data, words.shape[1], out.ctypes.data_as(_lib._i64p)))
        return _with_outside(out[:B], self.number_of_edges())

    def cheeger_philox_counts(self, seed, first, count):
        """The same for subsets ``first .. first + count - 1`` of the Philox family of ``seed`` (include/dcr.h), drawn on
        the device; ``first`` a multiple of 64."""
        out = np.empty((max(int(count), 0), 3), dtype=np.int64)
        check(lib().dcr_cheeger_philox_counts(self._h, int(seed), int(first), int(count), out.ctypes.data_as(_lib._i64p)))
        return _with_outside(out, self.number_of_edges())

    def cheeger_philox_values(self, seed, first, count, definition='reference'):
        """Their ratios as float64 ``[count]``: ``'reference'`` lo / min(2 in, 2 out), ``'conductance'`` (lo + hi) /
        min(2 in + lo + hi, 2 out + lo + hi); inf where the smaller volume is zero."""
        out = np.empty(max(int(count), 0), dtype=np.float64)
        check(lib().dcr_cheeger_philox_values(self._h, int(seed), int(first), int(count), CHEEGER_DEFINITIONS[definition],
                                              out.ctypes.data_as(_lib._f64p)))
        return out

    def cheeger_philox_members(self, seed, first, words):
        """The device-drawn membership words ``first / 64 .. first / 64 + words - 1`` as uint64 ``[n, words]``."""
        out = np.empty((self.num_nodes, max(int(words), 0)), dtype=np.uint64)
        check(lib().dcr_cheeger_philox_members(self._h, int(seed), int(first), int(words), out.ctypes.data))
        return out

    # ---- spectral gap (experiment/cheeger_bounds.py) -------------------------------------------------------------------
    def connected_components(self):
        """(count, labels int32 ``[n]``): the label of a node is the smallest node id of its component; an isolated node is
        a component.  Computed on the device over the live adjacency."""
        labels = np.empty(self.num_nodes, dtype=np.int32)
        count = ctypes.c_int64()
        check(lib().dcr_connected_components(self._h, labels.ctypes.data_as(_lib._i32p), ctypes.byref(count)))
        return count.value, labels

    def spectral_gap(self, tol=1e-10, max_steps=20000, max_basis=None, seed=0, return_vector=False):
        """The smallest eigenvalue of the normalised Laplacian above its null space (cheeger_bounds.py:13-16 as it is meant:
        the (c+1)-th smallest with c components), by deflated Lanczos on the device (csrc/dcr_spectral.hip).  Returns a
        ``SpectralGap``; ``converged`` says that the true residual of the returned pair is <= ``tol`` (a ``RuntimeWarning``
        when it is not).  ``ValueError`` on a graph without edges.  ``vector``: the unit eigenvector in node order."""
        opts = _lib.SpectralOpts(float(tol), int(max_steps), 0 if max_basis is None else int(max_basis), int(seed))
        res = _lib.SpectralResult()
        vec = np.empty(self.num_nodes, dtype=np.float64) if return_vector else None
        check(lib().dcr_spectral_gap(self._h, ctypes.byref(opts), ctypes.byref(res),
                                     vec.ctypes.data_as(_lib._f64p) if return_vector else None))
        if not res.converged:
            warnings.warn(f'spectral_gap: residual {res.residual:.3e} above tol {float(tol):.3e} after {res.steps} steps',
                          RuntimeWarning, stacklevel=2)
        return SpectralGap(res.lambda1, res.residual, res.steps, res.restarts, res.components, bool(res.converged), vec)

    # ---- sweep cut (csrc/dcr_sweep.hip) ----------------------------------------------------------------------------------
    def _sweep_result(self, res, order, profile):
        counts3 = np.array([[res.n_in, res.n_lo, res.n_hi]], dtype=np.int64)
        return SweepCut(res.value, int(res.size), _with_outside(counts3, self.number_of_edges())[0], order, profile)

    def sweep_cut(self, score, definition='conductance', return_order=True, return_profile=False):
        """The best prefix of the nodes ordered ascending by ``(score, node id)`` (``-0.0 == +0.0``; ``np.lexsort((ids,
        np.where(score == 0, 0.0, score)))``): S_k = the first k nodes, k = 1 .. n - 1, valued by ``definition`` as in
        ``cheeger_philox_values``; the smallest value and the smallest k that has it.  Sorted, counted and minimised on the
        device over the live adjacency, read-only on the graph.  Returns a ``SweepCut``; ``order`` int32 ``[n]`` (the node at
        each position), ``profile`` float64 ``[n - 1]`` (the value of every prefix).  ``ValueError`` on a NaN, a score of
        the wrong length or fewer than two nodes."""
        x = np.ascontiguousarray(np.asarray(score, dtype=np.float64))
        if x.ndim != 1 or x.shape[0] != self.num_nodes:
            raise ValueError(f'score must have shape [{self.num_nodes}]')
        res = _lib.SweepResult()
        order = np.empty(self.num_nodes, dtype=np.int32) if return_order else None
        profile = np.empty(max(self.num_nodes - 1, 0), dtype=np.float64) if return_profile else None
        check(lib().dcr_sweep_cut(self._h, x.ctypes.data_as(_lib._f64p), CHEEGER_DEFINITIONS[definition], ctypes.byref(res),
                                  order.ctypes.data_as(_lib._i32p) if return_order else None,
                                  profile.ctypes.data_as(_lib._f64p) if return_profile else None))
        return self._sweep_result(res, order, profile)

    def fiedler_sweep(self, definition='conductance', tol=1e-10, max_steps=20000, max_basis=None, seed=0):
        """``spectral_gap`` and the sweep of its eigenvector in D^-1/2 scaling in one call, the vector never leaving the device:
        ``(SpectralGap, SweepCut, score)``, ``score`` float64 ``[n]`` the numbers that were ordered.  With ``'conductance'``
        ``lambda1 / 2 <= h <= SweepCut.value <= sqrt(2 lambda1)``: the set ``order[:size]`` certifies the upper bound.  The
        same ``RuntimeWarning`` as ``spectral_gap`` when the solver did not converge."""
        opts = _lib.SpectralOpts(float(tol), int(max_steps), 0 if max_basis is None else int(max_basis), int(seed))
        gap, res = _lib.SpectralResult(), _lib.SweepResult()
        order = np.empty(self.num_nodes, dtype=np.int32)
        score = np.empty(self.num_nodes, dtype=np.float64)
        check(lib().dcr_fiedler_sweep(self._h, ctypes.byref(opts), CHEEGER_DEFINITIONS[definition], ctypes.byref(gap),
                                      ctypes.byref(res), order.ctypes.data_as(_lib._i32p), score.ctypes.data_as(_lib._f64p)))
        if not gap.converged:
            warnings.warn(f'fiedler_sweep: residual {gap.residual:.3e} above tol {float(tol):.3e} after {gap.steps} steps',
                          RuntimeWarning, stacklevel=2)
        return (SpectralGap(gap.lambda1, gap.residual, gap.steps, gap.restarts, gap.components, bool(gap.converged), None),
                self._sweep_result(res, order, None), score)

    # ---- effective resistance (csrc/dcr_resistance.hip) -------------------------------------------------------------------
    def effective_resistance(self, pairs, tol=1e-10, max_steps=20000, return_info=False):
        """Effective resistance R(u, v) = (e_u - e_v)^T L^+ (e_u - e_v), L = D - A, of each pair of ``pairs`` (array-like
        ``[P, 2]``) on the live graph, as float64 ``[P]``: ``RESISTANCE_BATCH`` conjugate-gradient solves at a time on the device,
        read-only on the graph.  The value is the LOWER bound ``2 c^T y - y^T L' y`` of include/dcr.h: never above R (whatever
        ``max_steps``), and within ``residual ** 2 / lambda_1`` of it.  0.0 for u == v and inf across components, both decided
        without a solve.  ``return_info``: also a dict of ``residual`` (float64, the true ``|c - L' y|``), ``steps`` (int32) and
        ``converged`` (bool: ``residual <= tol |c|``, ``|c|^2 = 1 / deg u + 1 / deg v``; True where no solve was needed).
        ``RuntimeWarning`` when a pair did not converge; ``ValueError`` on an endpoint outside the graph."""
        pr = np.asarray(pairs)
        if pr.size == 0:
            pr = pr.reshape(0, 2)
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise ValueError('pairs must have shape [P, 2]')
        if pr.size and (pr.min() < -2 ** 31 or pr.max() >= 2 ** 31):
            raise ValueError('pair endpoint outside 0 .. num_nodes - 1')
        u = np.ascontiguousarray(pr[:, 0], dtype=np.int32)
        v = np.ascontiguousarray(pr[:, 1], dtype=np.int32)
        P = u.shape[0]
        lower, residual = np.empty(P, dtype=np.float64), np.empty(P, dtype=np.float64)
        steps = np.empty(P, dtype=np.int32)
        opts = _lib.ResistanceOpts(float(tol), int(max_steps))
        check(lib().dcr_effective_resistance(self._h, u.ctypes.data_as(_lib._i32p), v.ctypes.data_as(_lib._i32p), P, ctypes.byref(opts),
                                             lower.ctypes.data_as(_lib._f64p), residual.ctypes.data_as(_lib._f64p),
                                             steps.ctypes.data_as(_lib._i32p)))
        converged = np.ones(P, dtype=bool)
        solved = np.flatnonzero(np.isfinite(lower) & (u != v))
        if solved.size:
            nodes = np.unique(np.concatenate([u[solved], v[solved]]))
            deg = np.zeros(self.num_nodes, dtype=np.float64)
            if nodes.size <= 64:
                deg[nodes] = [self.degree(int(x)) for x in nodes]
            else:
                deg = np.bincount(np.concatenate(self.edges()), minlength=self.num_nodes).astype(np.float64)
            cnorm = np.sqrt(1.0 / deg[u[solved]] + 1.0 / deg[v[solved]])
            converged[solved] = residual[solved] <= float(tol) * cnorm
        if not converged.all():
            worst = residual[~converged].max()
            warnings.warn(f'effective_resistance: {int((~converged).sum())} of {P} pairs above tol {float(tol):.3e} after '
                          f'{int(max_steps)} steps (largest residual {worst:.3e})', RuntimeWarning, stacklevel=2)
        if return_info:
            return lower, {'residual': residual, 'steps': steps, 'converged': converged}
        return lower

    # ---- sketched effective resistance (csrc/dcr_resistance_sketch.hip) -------------------------------------------------
    def resistance_sketch(self, columns=256, seed=0, pairs=None, edges=True, tol=1e-6, max_steps=20000, return_info=False):
        """The sketched effective resistance ``R~(u, v) = 1/k sum_j (z_j[u] - z_j[v])^2``, ``L z_j = B^T q_j`` for ``k = columns``
        Rademacher sign vectors q_j drawn from ``seed`` (include/dcr.h has the rule): unbiased, with a relative standard deviation
        of at most ``sketch_relative_std(columns) = sqrt(2 / columns)`` for every edge and pair at once, from one set of ``columns``
        conjugate-gradient solves, ``RESISTANCE_BATCH`` a batch, read-only on the live graph.  With ``edges=True`` returns
        ``(eu, ev, R)``, ``eu, ev`` being ``self.edges()`` and ``R`` float64 ``[E]`` in that order; with ``pairs`` (array-like
        ``[P, 2]``) float64 ``[P]``, 0.0 for u == v and inf across components; with both ``((eu, ev, R), pair_values)``.
        ``return_info``: a dict is appended with ``residual`` (float64 ``[columns]``, the true residual of each column's solve),
        ``columns``, ``batches``, ``steps_total``, ``residual_max`` and ``converged`` (bool ``[columns]``: ``residual <= 2 tol
        sqrt(2 E)``.  A column stops at ``tol |s * b_j|`` and ``|s * b_j|^2 = sum_w b_j[w]^2 / deg w <= 2 E``, so a column that
        fails this has not converged; the norms themselves are not returned).  ``RuntimeWarning`` when a column fails it;
        ``ValueError`` on an endpoint outside the graph."""
        if not edges and pairs is None:
            raise ValueError('nothing asked for: edges=False and no pairs')
        P = 0
        u = v = pair_out = None
        if pairs is not None:
            pr = np.asarray(pairs)
            if pr.size == 0:
                pr = pr.reshape(0, 2)
            if pr.ndim != 2 or pr.shape[1] != 2:
                raise ValueError('pairs must have shape [P, 2]')
            if pr.size and (pr.min() < -2 ** 31 or pr.max() >= 2 ** 31):
                raise ValueError('pair endpoint outside 0 .. num_nodes - 1')
            u = np.ascontiguousarray(pr[:, 0], dtype=np.int32)
            v = np.ascontiguousarray(pr[:, 1], dtype=np.int32)
            P = u.shape[0]
            pair_out = np.empty(max(P, 1), dtype=np.float64)
        if not -2 ** 31 <= int(columns) < 2 ** 31:
            raise ValueError('columns must be >= 1')
        opts = _lib.SketchOpts(int(columns), int(seed) & (2 ** 64 - 1), float(tol), int(max_steps))
        eu = ev = edge = None
        if edges:
            eu, ev = self.edges()
            edge = np.empty(max(eu.shape[0], 1), dtype=np.float64)
        residual = np.empty(max(int(columns), 1), dtype=np.float64)
        info = _lib.SketchInfo()
        check(lib().dcr_resistance_sketch(self._h, ctypes.byref(opts), edge.ctypes.data_as(_lib._f64p) if edges else None,
                                          u.ctypes.data_as(_lib._i32p) if P else None, v.ctypes.data_as(_lib._i32p) if P else None, P,
                                          pair_out.ctypes.data_as(_lib._f64p) if P else None, residual.ctypes.data_as(_lib._f64p),
                                          ctypes.byref(info)))
        residual = residual[:int(columns)]
        converged = residual <= 2.0 * float(tol) * np.sqrt(2.0 * self.number_of_edges())   # False for a NaN
        if not converged.all():
            warnings.warn(f'resistance_sketch: {int((~converged).sum())} of {int(columns)} columns above tol {float(tol):.3e} after '
                          f'{int(max_steps)} steps (largest residual {info.residual_max:.3e})', RuntimeWarning, stacklevel=2)
        out = ()
        if edges:
            out += ((eu, ev, edge[:eu.shape[0]]),)
        if pairs is not None:
            out += (pair_out[:P],)
        if return_info:
            out += ({'residual': residual, 'converged': converged, 'columns': int(info.columns), 'batches': int(info.batches),
                     'steps_total': int(info.steps_total), 'residual_max': float(info.residual_max)},)
        return out[0] if len(out) == 1 else out

    def resistance_sketch_rhs(self, seed, batch):
        """The device-drawn right-hand sides ``b_j = B^T q_j`` of the 16 columns of batch ``batch``, as float64 ``[n, 16]`` of
        integers (for the tests)."""
        out = np.empty((self.num_nodes, RESISTANCE_BATCH), dtype=np.float64)
        check(lib().dcr_resistance_sketch_rhs(self._h, int(seed) & (2 ** 64 - 1), int(batch), out.ctypes.data_as(_lib._f64p)))
        return out

    # ---- PageRank diffusion (csrc/dcr_diffusion.hip) ----------------------------------
    def _sources(self, sources):
        src = np.asarray(sources)
        if src.size == 0:
            src = src.reshape(0)
        if src.ndim != 1:
            raise ValueError('sources must be one-dimensional')
        if src.size and (src.min() < 0 or src.max() >= self.num_nodes):
            raise ValueError('source outside 0 .. num_nodes - 1')
        return np.ascontiguousarray(src, dtype=np.int32)

    @staticmethod
    def _warn_unconverged(what, converged, residual, tol, max_steps):
        if not converged.all():
            warnings.warn(f'{what}: {int((~converged).sum())} of {converged.size} columns above tol {float(tol):.3e} after '
                          f'{int(max_steps)} steps (largest residual {residual[~converged].max():.3e})', RuntimeWarning, stacklevel=3)

    def ppr(self, sources, alpha=0.15, tol=1e-10, max_steps=20000, return_info=False):
        """Columns of the personalised-PageRank matrix ``S = alpha (I - (1 - alpha) D~^-1/2 (A + I) D~^-1/2)^-1`` of the live graph
        (``D~ = D + I``; include/dcr.h has the definition), as float64 ``[len(sources), n]``: row ``i`` is column ``sources[i]``.
        ``DIFFUSION_BATCH`` conjugate-gradient solves at a time on the device, read-only on the graph.  ``return_info``: also a
        dict of ``residual`` (float64, the true ``|alpha e_j - M x|``; every entry is within ``residual / alpha`` of S's), ``steps``
        (int32) and ``converged`` (bool: ``residual <= tol alpha``).  ``RuntimeWarning`` when a column did not converge;
        ``ValueError`` on a source outside the graph or ``alpha`` outside (0, 1)."""
        src = self._sources(sources)
        P = src.shape[0]
        out = np.empty((P, self.num_nodes), dtype=np.float64)
        residual, steps = np.empty(P, dtype=np.float64), np.empty(P, dtype=np.int32)
        opts = _lib.DiffusionOpts(float(alpha), float(tol), int(max_steps))
        check(lib().dcr_ppr_columns(self._h, src.ctypes.data_as(_lib._i32p), P, ctypes.byref(opts), out.ctypes.data_as(_lib._f64p),
                                    residual.ctypes.data_as(_lib._f64p), steps.ctypes.data_as(_lib._i32p)))
        converged = residual <= float(tol) * float(alpha)
        self._warn_unconverged('ppr', converged, residual, tol, max_steps)
        if return_info:
            return out, {'residual': residual, 'steps': steps, 'converged': converged}
        return out

    HEAT_MAX_TERMS = 4096   # the default of dcr_heat_opts

    def _heat_converged(self, src, deficit, tol):
        """deficit <= tol sqrt(deg_j + 1) per column; src None stands for all nodes."""
        nodes = np.arange(self.num_nodes) if src is None else src
        if nodes.size <= 64:
            deg = np.array([self.degree(int(v)) for v in nodes], dtype=np.float64)
        else:
            deg = np.bincount(np.concatenate(self.edges()), minlength=self.num_nodes).astype(np.float64)[nodes]
        return deficit <= float(tol) * np.sqrt(deg + 1.0)

    def heat(self, sources, t=5.0, tol=1e-10, max_terms=None, return_info=False):
        """Columns of the heat-kernel matrix ``S = exp(-t (I - D~^-1/2 (A + I) D~^-1/2))`` of the live graph (``D~ = D + I``,
        ``0 < t <= 256``; include/dcr.h has the definition), as float64 ``[len(sources), n]``: row ``i`` is the Taylor partial sum
        ``e^-t sum_{k <= K} t^k / k! H^k e_j`` of column ``sources[i]``, with ``K`` the smallest count whose tail
        ``sum_{k > K} e^-t t^k / k!`` is at most ``tol / 2`` (``max_terms`` where that is lower; default 4096).  Every term is
        non-negative, so the result is an entrywise lower bound of ``S``.  ``return_info``: also a dict of ``deficit`` (float64,
        ``sqrt(deg_j + 1) - sum_i sqrt(deg_i + 1) x_i``: ``0 <= S_ij - x_i <= deficit / sqrt(deg_i + 1)``), ``terms`` (``K``) and
        ``converged`` (bool: ``deficit <= tol sqrt(deg_j + 1)``).  ``RuntimeWarning`` when the sum was cut short; ``ValueError`` on
        a source outside the graph or ``t`` outside (0, 256]."""
        if not 0.0 < float(t) <= 256.0:
            raise ValueError('t must lie in (0, 256]')
        src = self._sources(sources)
        P = src.shape[0]
        max_terms = self.HEAT_MAX_TERMS if max_terms is None else int(max_terms)
        out = np.empty((P, self.num_nodes), dtype=np.float64)
        deficit, terms = np.empty(P, dtype=np.float64), ctypes.c_int64(0)
        opts = _lib.HeatOpts(float(t), float(tol), max_terms)
        check(lib().dcr_heat_columns(self._h, src.ctypes.data_as(_lib._i32p), P, ctypes.byref(opts), out.ctypes.data_as(_lib._f64p),
                                     deficit.ctypes.data_as(_lib._f64p), ctypes.byref(terms)))
        converged = self._heat_converged(src, deficit, tol)
        self._warn_unconverged('heat', converged, deficit, tol, terms.value)
        if return_info:
            return out, {'deficit': deficit, 'terms': int(terms.value), 'converged': converged}
        return out

    def diffusion(self, alpha=0.15, k=None, eps=None, sources=None, return_info=False, tol=1e-10, max_steps=20000, kernel='ppr', t=5.0,
                  max_terms=None):
        """The sparsified personalised-PageRank matrix of the live graph (DIGL / GDC): per column ``j`` of ``S`` (``ppr``) either
        the ``k`` largest entries (larger value first, among equal bits the smaller node id first; everything where ``k >= n``)
        or the entries ``>= eps``, as the reference's ``get_top_k_matrix`` / ``get_clipped_matrix``
        (utils/adjacency_matrix_ops.py:26-39) select them, divided by the sum of the column's kept entries.  Exactly one of ``k``
        and ``eps`` must be given.  ``sources``: the columns, default all nodes.  Solve and selection run on the device; no n x n
        array exists on either side.

        Returns ``(edge_index, weight)``: int64 ``[2, nnz]`` holding ``[i; j]`` and float64 ``[nnz]``, grouped by column in the
        order of ``sources`` and by ``i`` ascending within a column.  ``return_info``: also a dict of ``value`` (the raw
        ``S_ij``), ``ptr`` (int64 ``[columns + 1]``), ``residual``, ``steps`` and ``converged`` per column as ``ppr`` has them.

        ``kernel='heat'``: ``S`` is the heat-kernel matrix of ``heat`` at ``t`` (``tol``, ``max_terms`` as there; ``alpha`` and
        ``max_steps`` are not used) and the dict holds ``deficit`` and ``terms`` as ``heat`` has them in place of ``residual`` and
        ``steps``.  Any other ``kernel`` than ``'ppr'`` and ``'heat'`` is a ``ValueError``."""
        if kernel not in ('ppr', 'heat'):
            raise ValueError("kernel must be 'ppr' or 'heat'")
        heat = kernel == 'heat'
        if (k is None) == (eps is None):
            raise ValueError('exactly one of k and eps must be given')
        n = self.num_nodes
        src = None if sources is None else self._sources(sources)
        P = n if src is None else src.shape[0]
        if heat:
            opts = _lib.HeatOpts(float(t), float(tol), self.HEAT_MAX_TERMS if max_terms is None else int(max_terms))
            call, terms = lib().dcr_heat_sparsify, ctypes.c_int64(0)
        else:
            opts = _lib.DiffusionOpts(float(alpha), float(tol), int(max_steps))
            call = lib().dcr_diffusion_sparsify
        mode = 0 if eps is None else 1
        if mode == 0 and int(k) < 1:
            raise ValueError('k must be >= 1')
        ptr = np.zeros(P + 1, dtype=np.int64)
        residual, steps = np.empty(P, dtype=np.float64), np.empty(P, dtype=np.int32)
        # top-k: the size is known.  threshold: a slab of columns at a time into room for all of their entries
        slab = P if mode == 0 else max(16, min(P, (1 << 23) // max(n, 1)) // 16 * 16)
        rows, weights, values = [], [], []
        for first in range(0, P, max(slab, 1)):
            count = min(slab, P - first)
            cap = count * (min(int(k), n) if mode == 0 else n)
            row, weight, value = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.float64), np.empty(cap, dtype=np.float64)
            part_ptr = np.zeros(count + 1, dtype=np.int64)
            nnz = ctypes.c_int64()
            part_src = np.arange(first, first + count, dtype=np.int32) if src is None else src[first:first + count]
            whole = src is None and count == n
            check(call(self._h, None if whole else part_src.ctypes.data_as(_lib._i32p), count, ctypes.byref(opts),
                       mode, int(k) if mode == 0 else 0, float(eps) if mode == 1 else 0.0,
                       part_ptr.ctypes.data_as(_lib._i64p), cap, row.ctypes.data_as(_lib._i32p),
                       weight.ctypes.data_as(_lib._f64p), value.ctypes.data_as(_lib._f64p), residual[first:].ctypes.data_as(_lib._f64p),
                       ctypes.byref(terms) if heat else steps[first:].ctypes.data_as(_lib._i32p), ctypes.byref(nnz)))
            ptr[first + 1:first + count + 1] = ptr[first] + part_ptr[1:]
            rows.append(row[:nnz.value])
            weights.append(weight[:nnz.value])
            values.append(value[:nnz.value])
        row = np.concatenate(rows) if rows else np.empty(0, dtype=np.int32)
        weight = np.concatenate(weights) if weights else np.empty(0, dtype=np.float64)
        value = np.concatenate(values) if values else np.empty(0, dtype=np.float64)
        cols = np.arange(n, dtype=np.int64) if src is None else src.astype(np.int64)
        edge_index = np.stack([row.astype(np.int64), np.repeat(cols, np.diff(ptr))])
        if heat:
            converged = self._heat_converged(src, residual, tol)
            self._warn_unconverged('diffusion', converged, residual, tol, terms.value)
            if return_info:
                return edge_index, weight, {'value': value, 'ptr': ptr, 'deficit': residual, 'terms': int(terms.value), 'converged': converged}
            return edge_index, weight
        converged = residual <= float(tol) * float(alpha)
        self._warn_unconverged('diffusion', converged, residual, tol, max_steps)
        if return_info:
            return edge_index, weight, {'value': value, 'ptr': ptr, 'residual': residual, 'steps': steps, 'converged': converged}
        return edge_index, weight

    # ---- FoSR (csrc/dcr_fosr.hip) -------------------------------------------------------
    def _vector(self, x, what):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        if x.ndim != 1 or x.shape[0] != self.num_nodes:
            raise ValueError(f'{what} must have shape [{self.num_nodes}]')
        return x

    def fosr_pick(self, x, return_y=False):
        """The edge FoSR would add for the vector ``x`` (float64 ``[n]``): with ``y = x / sqrt(deg + 1)``, the pair ``(u, v)`` of
        distinct non-adjacent nodes with the smallest ``y[u] * y[v]``, as ``(u, v, product)``; ``None`` where every pair is an edge.
        include/dcr.h states which of several minimal pairs it is.  Chosen on the device in O(n log n + E), read-only on the
        graph.  ``return_y``: also the ``y`` that was ordered (then ``(pick or None, y)``).  ``ValueError`` on a NaN, a vector of the
        wrong length or fewer than two nodes."""
        x = self._vector(x, 'x')
        u, v, found, product = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int(), ctypes.c_double()
        y = np.empty(self.num_nodes, dtype=np.float64) if return_y else None
        check(lib().dcr_fosr_pick(self._h, x.ctypes.data_as(_lib._f64p), ctypes.byref(u), ctypes.byref(v), ctypes.byref(product),
                                  y.ctypes.data_as(_lib._f64p) if return_y else None, ctypes.byref(found)))
        pick = (u.value, v.value, product.value) if found.value else None
        return (pick, y) if return_y else pick

    def fosr(self, num_iterations, initial_power_iters=50, x0=None, seed=0, return_vector=False):
        """FoSR, first-order spectral rewiring (Karhadkar et al., ICLR 2023), on the live graph: ``initial_power_iters`` power
        steps on ``x0`` (default: the Philox vector of ``seed``), then ``num_iterations`` times ``fosr_pick``, ``add_edge`` and one
        power step with the new degrees.  Returns the added edges in order as int64 ``[2, added]``; ``added`` is smaller than
        ``num_iterations`` where no free pair was left or the iterate vanished.  ``return_vector``: also the final iterate.

        Unlike the published code, which falls back to an existing edge or a self-loop when every free product is positive,
        only pairs that are not yet edges are candidates.  MUTATES the graph.  ``ValueError`` on a graph without edges."""
        x0 = None if x0 is None else self._vector(x0, 'x0')
        opts = _lib.FosrOpts(int(num_iterations), int(initial_power_iters), int(seed))
        room = max(int(num_iterations), 1)
        u, v = np.empty(room, dtype=np.int32), np.empty(room, dtype=np.int32)
        added = ctypes.c_int64()
        x = np.empty(self.num_nodes, dtype=np.float64) if return_vector else None
        check(lib().dcr_fosr(self._h, ctypes.byref(opts), None if x0 is None else x0.ctypes.data_as(_lib._f64p),
                             u.ctypes.data_as(_lib._i32p), v.ctypes.data_as(_lib._i32p), ctypes.byref(added),
                             x.ctypes.data_as(_lib._f64p) if return_vector else None))
        edges = np.stack([u[:added.value], v[:added.value]]).astype(np.int64)
        return (edges, x) if return_vector else edges

    # ---- hop distances (csrc/dcr_hops.hip) ------------------------------------------------
    def _hops(self, sources, max_hops, want_dist):
        src = None if sources is None else self._sources(sources)
        P = self.num_nodes if src is None else src.shape[0]
        if max_hops is not None and not 0 <= int(max_hops) < 2 ** 31:
            raise ValueError('max_hops must be None or lie in 0 .. 2^31 - 1')
        opts = _lib.HopsOpts(-1 if max_hops is None else int(max_hops))
        dist = np.empty((P, self.num_nodes), dtype=np.int32) if want_dist else None
        ecc, reached, total = np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int64), np.empty(P, dtype=np.int64)
        check(lib().dcr_hop_distances(self._h, None if src is None else src.ctypes.data_as(_lib._i32p), P, ctypes.byref(opts),
                                      dist.ctypes.data_as(_lib._i32p) if want_dist else None, ecc.ctypes.data_as(_lib._i32p),
                                      reached.ctypes.data_as(_lib._i64p), total.ctypes.data_as(_lib._i64p)))
        return dist, ecc, reached, total

    def hop_distances(self, sources, max_hops=None):
        """Hop distances on the live graph as int32 ``[len(sources), n]``: row ``i`` holds the number of edges of a shortest path
        from ``sources[i]`` to every node, ``-1`` where there is none (another component) or it is longer than ``max_hops``.
        Breadth-first search on the device, up to 256 sources a sweep of the adjacency (include/dcr.h has the rule), read-only on
        the graph; the rows come back a batch at a time, so the returned array is the only ``P x n`` object.  Duplicated sources
        are legal.  ``ValueError`` on a source outside the graph."""
        return self._hops(sources, max_hops, True)[0]

    def hop_summary(self, sources=None, max_hops=None):
        """``(ecc, reached, total)`` per source (int32, int64, int64 ``[len(sources)]``; ``sources=None``: every node): the
        largest distance reached, the number of nodes within ``max_hops`` (the source included: the ball size; the component's
        size without a limit) and the sum of their distances.  An isolated source gives ``(0, 1, 0)``, and so does every source at
        ``max_hops=0``.  The search of ``hop_distances`` without its rows: no distance row exists on either side."""
        return self._hops(sources, max_hops, False)[1:]

    # ---- betweenness centrality (csrc/dcr_betweenness.hip) ---------------------------------
    def betweenness(self, sources=None, edges=False, return_info=False):
        """Betweenness of the live graph as raw sums over ``sources`` (``None``: every node) of Brandes' dependencies: float64
        ``node[n]``, and with ``edges=True`` ``(node, (eu, ev, edge))`` where ``eu, ev`` are ``self.edges()`` and ``edge[E]`` the
        edge values in that order.  With every node a source this is the ordered-pair convention, twice
        ``networkx.betweenness_centrality(G, normalized=False)`` and ``edge_betweenness_centrality`` of an undirected graph;
        endpoints are not counted, other components contribute nothing, a duplicated source counts twice (include/dcr.h has the
        rule; ``experiment/betweenness.py`` the networkx scalings).  16 sources a batch on the device, about ``2 * levels`` sweeps
        of the adjacency a batch, read-only on the graph, the same bits on every call.  ``return_info``: a dict is appended with
        ``levels_max``, ``batches`` and ``sigma_max``, the largest number of shortest paths of a pair; above ``2 ** 53`` the path
        counts were rounded.  ``ValueError`` on a source outside the graph; ``DcrError`` where a path count leaves the float64
        range."""
        src = None if sources is None else self._sources(sources)
        P = self.num_nodes if src is None else src.shape[0]
        node = np.empty(self.num_nodes, dtype=np.float64)
        eu = ev = edge = None
        if edges:
            eu, ev = self.edges()
            edge = np.empty(max(eu.shape[0], 1), dtype=np.float64)
        info = _lib.BetweennessInfo()
        check(lib().dcr_betweenness(self._h, None if src is None else src.ctypes.data_as(_lib._i32p), P, node.ctypes.data_as(_lib._f64p),
                                    edge.ctypes.data_as(_lib._f64p) if edges else None, ctypes.byref(info)))
        out = (node, (eu, ev, edge[:eu.shape[0]])) if edges else (node,)
        if return_info:
            out += ({'levels_max': int(info.levels_max), 'batches': int(info.batches), 'sigma_max': float(info.sigma_max)},)
        return out[0] if len(out) == 1 else out

    # ---- measurement hooks ------------------------------------------------------------
    def profile_reset(self):
        check(lib().dcr_profile_reset(self._h))

    def profile_read(self):
        ms, cnt = ctypes.c_double(), ctypes.c_int64()
        check(lib().dcr_profile_read(self._h, ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    def pass_engine(self):
        """Which kernels ran the last curvature pass (all produce the same bits)."""
        out = ctypes.c_int()
        check(lib().dcr_pass_engine(self._h, ctypes.byref(out)))
        return {0: 'two-hop', 1: 'edge-centric', 2: 'node-centric'}.get(out.value, 'none')

    def h2_stats(self):
        """Diagnostics of the last two-hop pass: candidates listed for the triangle kernel per pool, block-class units that
        took that probe path, units of class M and of the split class, units on the retry list."""
        out = (ctypes.c_int32 * 6)()
        check(lib().dcr_h2_stats(self._h, out))
        return {'ncand': (out[0], out[1]), 'fallback': out[2], 'units_m': out[3], 'units_split': out[4], 'retry': out[5]}

    def h2_launch_info(self):
        """How the last curvature pass call ran the two-hop pass: times it was launched (0: another engine ran), and whether
        the last launch carried the retry stage and the triangle stage."""
        out = (ctypes.c_int32 * 5)()
        check(lib().dcr_h2_launch_info(self._h, out))
        return {'launches': out[0], 'retry_stage': bool(out[1]), 'triangle_stage': bool(out[2])}

    def h2_head_info(self):
        """The heads of the two-hop launches ``h2_launch_info`` counts: how many of them ran the weight kernel (the node weights
        were not kept from the last pass) and the stand-alone clear (the full head, not the two plan kernels alone)."""
        out = (ctypes.c_int32 * 5)()
        check(lib().dcr_h2_launch_info(self._h, out))
        return {'weight_kernels': out[3], 'clear_kernels': out[4]}

    def h2_weight_check(self):
        """Nodes whose kept two-hop weight differs from a recomputation from the rows (-1: no weights are kept yet)."""
        out = ctypes.c_int64()
        check(lib().dcr_h2_weight_check(self._h, ctypes.byref(out)))
        return out.value

    def bfc_algorithmic_bytes(self, one_sided=False):
        """SURVEY §8(d) bytes of one BFC pass; ``one_sided``: only the cheaper difference set's rows per edge."""
        out = ctypes.c_double()
        fn = lib().dcr_bfc_algorithmic_bytes_one_sided if one_sided else lib().dcr_bfc_algorithmic_bytes
        check(fn(self._h, ctypes.byref(out)))
        return out.value
