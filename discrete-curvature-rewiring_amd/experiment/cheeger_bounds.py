"""Spectral bracket of the Cheeger constant — call surface of the reference's experiment/cheeger_bounds.py:11-21.

``cheeger_bounds(data)`` returns the reference's two strings, ``lambda_1 / 2`` and ``sqrt(2 lambda_1)`` formatted ``' .2e'``:
the bracket ``lambda_1 / 2 <= h <= sqrt(2 lambda_1)`` of the constant ``experiment/compute_cheeger.py`` estimates.

  reference line                                here
  :12    to_networkx                            DcrGraph.from_data  (as compute_cheeger.py uploads it), or a live DcrGraph
  :13    normalized_laplacian_matrix, dense     never formed: I + D^-1/2 A D^-1/2 applied to vectors over the live adjacency
  :15    scipy.linalg.eigh, O(N^3)              DcrGraph.spectral_gap  (csrc/dcr_spectral.hip: deflated Lanczos in fp64, accepted
                                                on the true residual of the eigenpair)
  :16    lambdas[lambdas > 0][0]                the (c+1)-th smallest eigenvalue, c = connected components  (see below)
  :18-21 left, right, the two strings           the same float64 expressions and format

One deviation, on purpose.  Line :16 takes the first eigenvalue that floating point left strictly positive.  The normalised
Laplacian has exactly c zero eigenvalues, c the number of connected components (an isolated node counts as one: networkx gives
it a zero row), and ``eigh`` returns them as noise of either sign around 1e-16.  Whenever one of them comes out positive the
reference returns that noise: ``(' 3.11e-16', ' 3.53e-08')`` for two K20 joined by a path of four nodes, whose gap is 1.03e-3.  What
the line means is the smallest eigenvalue above the null space, and that is what is computed here; on every graph where all c
noise values come out <= 0 the strings are the reference's own (``tests/golden/cheeger_bounds_reference.json`` records for each
of its graphs which case it is, ``reference_sound``).  A graph without edges has no positive eigenvalue: ``ValueError`` here,
``IndexError`` in the reference.

``cheeger_sweep(data)`` is the certificate for that bracket, and has no counterpart in the reference.  The bracket is two numbers; the
constructive half of Cheeger's inequality gives a set: order the nodes by the eigenvector of lambda_1 in D^-1/2 scaling, take the
prefix of that order with the smallest conductance, and ``lambda_1 / 2 <= h <= conductance <= sqrt(2 lambda_1)``.  Eigenvector,
sort, edge counts of every prefix and the arg-min stay on the device (``DcrGraph.fiedler_sweep``, csrc/dcr_sweep.hip); neither the
vector nor the edge list comes back to the host.

No dataset loop and no pickles here: the reference's ``__main__`` (:24-39) reads edge lists saved by earlier runs.
"""
import math


def _graph(data):
    from dcr.graph import DcrGraph
    return data if isinstance(data, DcrGraph) else DcrGraph.from_data(data)


def cheeger_bounds_values(data, **solver):
    """``(left, right, lambda1)`` as floats: ``lambda1 / 2``, ``sqrt(2 lambda1)`` and the spectral gap itself.
    :param data: a ``Data``, or a live ``DcrGraph``.
    :param solver: keyword arguments of ``DcrGraph.spectral_gap`` (``tol``, ``max_steps``, ``max_basis``, ``seed``).
    """
    unknown = set(solver) - {'tol', 'max_steps', 'max_basis', 'seed'}
    if unknown:
        raise TypeError(f'unknown solver arguments: {sorted(unknown)}')
    lambda1 = _graph(data).spectral_gap(**solver).lambda1
    return lambda1 / 2, math.sqrt(2 * lambda1), lambda1


def format_bounds(left, right):
    """cheeger_bounds.py:21."""
    return f'{left: .2e}', f'{right: .2e}'


def cheeger_bounds(data):
    left, right, _ = cheeger_bounds_values(data)
    return format_bounds(left, right)


def cheeger_sweep(data, definition='conductance', **solver):
    """``(value, members, lambda1)``: the best sweep cut of the Fiedler order, ``members`` a bool ``[n]`` array holding the side of
    smaller volume, and the spectral gap.  ``'conductance'``: (lo + hi) / min(vol S, vol V - S), for which ``lambda1 / 2 <= value <=
    sqrt(2 lambda1)``.  ``'reference'``: compute_cheeger.py's own ratio, lo / min(2 in, 2 out); it is not symmetric in the
    orientation of the order (``lo`` counts only the edges whose SMALLER endpoint is inside), so both x and -x are swept and the
    smaller value is returned.
    :param data: a ``Data``, or a live ``DcrGraph``.
    :param solver: keyword arguments of ``DcrGraph.spectral_gap`` (``tol``, ``max_steps``, ``max_basis``, ``seed``).
    """
    import numpy as np
    unknown = set(solver) - {'tol', 'max_steps', 'max_basis', 'seed'}
    if unknown:
        raise TypeError(f'unknown solver arguments: {sorted(unknown)}')
    G = _graph(data)
    gap, cut, score = G.fiedler_sweep(definition=definition, **solver)
    if definition == 'reference':
        other = G.sweep_cut(-score, definition=definition)
        if other.value < cut.value:
            cut = other
    members = np.zeros(G.number_of_nodes(), dtype=bool)
    members[cut.order[:cut.size]] = True
    n_in, _, _, n_out = (int(c) for c in cut.counts)
    if n_in > n_out:   # vol S - vol (V - S) = 2 (in - out) under either definition
        members = ~members
    return cut.value, members, gap.lambda1
