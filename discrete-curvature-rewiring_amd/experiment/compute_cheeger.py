"""Monte-Carlo estimate of the Cheeger constant — call surface of the reference's experiment/compute_cheeger.py:19-64.

Same names, same signatures, same results: ``estimate_cheeger(data, iterations)`` returns bit for bit what the reference
returns for the same state of Python's global ``random`` stream, and leaves that stream where the reference leaves it.

  reference line                            here
  :55    to_networkx                        DcrGraph.from_data  (as rewiring/sdrf_no_cuda.py uploads it), or a live DcrGraph
  :59    random_subset, n x randint(0, 1)   mt_members: the same Mersenne-Twister outputs taken in bulk through numpy
  :60    G.subgraph, deepcopy, edge loop    DcrGraph.cheeger_counts  (csrc/dcr_cheeger.hip: every draw of a batch in one
                                            sweep of the rows, three integers per draw)
  :45    b / m                              one float64 division of those integers

What the reference computes has two quirks, kept under ``definition='reference'`` (the default):
  * boundary_size (:32-37) counts an edge (i, j) of ``G.edges`` only when i is inside and j outside; ``G.edges`` yields each
    edge once with i < j, so cut edges whose LARGER endpoint is inside are not counted: about half the cut;
  * both volumes are taken on induced subgraphs (:60 ``G.subgraph(S)``, :42-44 ``G`` minus ``S``), i.e. twice the number of
    edges inside each side, not the sum of the members' degrees in G.
``definition='conductance'`` is the textbook quantity instead: every cut edge over the smaller of the two true-degree
volumes, what ``networkx.conductance(G, S)`` returns.

No plotting and no dataset loop here: the reference's ``__main__`` (:67-118) draws figures from pickles of earlier runs.
"""
from random import getstate, randint, setstate

import numpy as np

_DEFINITIONS = ('reference', 'conductance')
_RNGS = ('python', 'philox')


# ---- the reference's helpers on networkx graphs (host code; estimate_cheeger does not go through them) -----------------
def random_subset(nodes):
    """compute_cheeger.py:19-24: every node of ``nodes``, in iteration order, is kept iff its ``randint(0, 1)`` is 0."""
    return {node for node in nodes if randint(0, 1) == 0}


def vol(S):
    """compute_cheeger.py:27-29: sum of the degrees of the graph ``S``."""
    return sum(d for _, d in S.degree())


def boundary_size(G, S):
    """compute_cheeger.py:32-37: edges (i, j) of ``G.edges`` with i in ``S`` and j not in it (one-sided, see above)."""
    inside = S.nodes
    return sum(1 for i, j in G.edges if i in inside and j not in inside)


def cheeger_S(G, S):
    """compute_cheeger.py:40-45 without the deep copy: vol(G - S) is twice the edges with neither end in ``S``."""
    inside = S.nodes
    outside_edges = sum(1 for i, j in G.edges if i not in inside and j not in inside)
    m = min(vol(S), 2 * outside_edges)
    return float('inf') if m == 0 else boundary_size(G, S) / m


# ---- Python's randint(0, 1) stream in bulk ---------------------------------------------------------------------------
def _numpy_twin():
    """A numpy MT19937 bit generator in the state of Python's global ``random`` stream, and the rest of that state."""
    version, internal, gauss_next = getstate()
    if version != 3:
        raise RuntimeError(f'unknown random.getstate() version {version}')
    bg = np.random.MT19937()
    bg.state = {'bit_generator': 'MT19937', 'state': {'key': np.array(internal[:-1], dtype=np.uint32), 'pos': internal[-1]}}
    return bg, version, gauss_next


def _hand_back(bg, version, gauss_next):
    st = bg.state['state']
    setstate((version, tuple(int(k) for k in st['key']) + (int(st['pos']),), gauss_next))


def mt_members(count, num_nodes):
    """bool ``[count, num_nodes]``: the subsets ``count`` successive calls of ``random_subset(range(num_nodes))`` would draw
    from Python's global ``random`` stream, which is advanced exactly as those calls would advance it.

    ``randint(0, 1)`` is ``_randbelow(2)``: ``getrandbits(2)``, the top two bits of one 32-bit Mersenne-Twister output, drawn
    again while the value is 2 or 3.  So an output with its top bit set is skipped, and any other decides one node: member
    iff bit 30 is clear.  numpy's MT19937 produces the same outputs from the same 624 words."""
    need = int(count) * int(num_nodes)
    out = np.empty(need, dtype=np.bool_)
    if need == 0:
        return out.reshape(int(count), int(num_nodes))
    bg, version, gauss_next = _numpy_twin()
    have = 0
    while have < need:
        rem = need - have
        # outputs are accepted with probability 1/2: take a block that ends short of the goal by about 5.6 standard
        # deviations, and the last stretch twice (once to see where the goal falls, once to stop exactly there)
        m = 2 * rem - int(8 * np.sqrt(rem)) if rem > 4096 else 0
        saved = bg.state
        if m > 0:
            raw = bg.random_raw(m)
            acc = raw[raw < 0x80000000]
            if acc.shape[0] <= rem:
                out[have:have + acc.shape[0]] = acc < 0x40000000
                have += acc.shape[0]
                continue
            bg.state = saved
        raw = bg.random_raw(2 * rem + 64)
        ok = raw < 0x80000000
        pos = np.flatnonzero(ok)
        if pos.shape[0] < rem:
            out[have:have + pos.shape[0]] = raw[pos] < 0x40000000
            have += pos.shape[0]
            continue
        bg.state = saved
        raw = bg.random_raw(int(pos[rem - 1]) + 1)
        out[have:] = raw[raw < 0x80000000] < 0x40000000
        have = need
    _hand_back(bg, version, gauss_next)
    return out.reshape(int(count), int(num_nodes))


# ---- ratios ------------------------------------------------------------------------------------------------------------
def values_from_counts(counts, definition='reference'):
    """float64 ratios from int64 ``[B, 4]`` (in, lo, hi, out): one IEEE division of two exactly represented integers per
    subset (what Python's ``b / m`` gives, compute_cheeger.py:45); inf where the smaller volume is zero."""
    c = np.asarray(counts, dtype=np.int64)
    if definition == 'reference':
        num = c[:, 1]
        den = 2 * np.minimum(c[:, 0], c[:, 3])
    elif definition == 'conductance':
        num = c[:, 1] + c[:, 2]
        den = 2 * np.minimum(c[:, 0], c[:, 3]) + num
    else:
        raise ValueError(f"definition must be one of {_DEFINITIONS}, not {definition!r}")
    vals = np.full(c.shape[0], np.inf)
    np.divide(num, den, out=vals, where=den != 0)
    return vals


def estimate_cheeger(data, iterations, *, rng='python', seed=None, definition='reference', batch=1024):
    """
    MC estimator of the Cheeger constant
    :param data: graph data for which to estimate the Cheeger constant (a ``Data``, or a live ``DcrGraph``).
    :param iterations: number of iterations.
    :param rng: 'python': the reference's subsets, from the global ``random`` stream; 'philox': subsets 0 .. iterations - 1
        of the device's Philox family of ``seed`` (independent of ``batch``).
    :param definition: 'reference' (the module docstring's two quirks) or 'conductance'.
    :param batch: subsets per launch.
    :return: Cheeger constant estimation, and the list of every draw's value.
    """
    if rng not in _RNGS:
        raise ValueError(f"rng must be one of {_RNGS}, not {rng!r}")
    if definition not in _DEFINITIONS:
        raise ValueError(f"definition must be one of {_DEFINITIONS}, not {definition!r}")
    iterations, batch = int(iterations), int(batch)
    if iterations < 0:
        raise ValueError('iterations must not be negative')
    if batch < 1:
        raise ValueError('batch must be at least 1')
    if rng == 'philox' and seed is None:
        raise ValueError("rng='philox' needs a seed")
    from dcr.graph import DcrGraph
    G = data if isinstance(data, DcrGraph) else DcrGraph.from_data(data)
    n = G.number_of_nodes()
    all_results = []
    if rng == 'philox':
        step = (batch + 63) // 64 * 64   # subsets are drawn 64 to a word; which launch computes a subset changes nothing
        for first in range(0, iterations, step):
            all_results.extend(G.cheeger_philox_values(seed, first, min(step, iterations - first), definition).tolist())
    else:
        for first in range(0, iterations, batch):
            counts = G.cheeger_counts(mt_members(min(batch, iterations - first), n))
            all_results.extend(values_from_counts(counts, definition).tolist())
    return min(all_results, default=float('inf')), all_results
