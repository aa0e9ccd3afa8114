"""The sizes at which the sweep, diffusion and FoSR kernels change their control flow, and the graphs the GPU tests use there (host
only).  The constants are read out of csrc/*.hip and csrc/dcr_analysis.h, the launch arithmetic of sweep_buffers, diffusion_batches
and row_grid is restated in Python, and tests/test_scale_thresholds_cpu.py asserts that every size named here sits just past the
boundary it is there for.  The graphs are built with array operations only: a Python loop over half a million nodes costs more
than the kernels under test."""
import os
import re

import numpy as np

from conftest import PKG

CSRC = os.path.join(PKG, 'csrc')


# ---- constants of the sources --------------------------------------------------------------------------------------------------
def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, name):
    m = re.search(r'constexpr\s+(?:int|int64_t)\s+%s\s*=\s*(\d+)\s*;' % name, text)
    assert m, name + ' not found'
    return int(m.group(1))


def constants():
    """Every constant the sizes below depend on, by the name it has in the sources ('SW_MAX_TILES' and 'SW_KEYS_BLOCKS' have
    none there: they are the literals of sweep_buffers and of the launch of k_sweep_keys)."""
    sweep, dif, fosr, header = (source(f) for f in ('dcr_sweep.hip', 'dcr_diffusion.hip', 'dcr_fosr.hip', 'dcr_analysis.h'))
    c = {name: constant(sweep, name) for name in ('SW_SCAN_BLOCK', 'SW_VALUE_BLOCKS', 'SW_TILE')}
    m = re.search(r'if\s*\(n\s*>\s*(\d+)\s*\*\s*SW_TILE\)\s*tile\s*=\s*\(\(n\s*\+\s*(\d+)\)\s*/\s*(\d+)\s*\+\s*63\)\s*/\s*64\s*\*\s*64\s*;', sweep)
    assert m, 'the tile rule of sweep_buffers not found'
    assert int(m.group(1)) == int(m.group(3)) == int(m.group(2)) + 1
    c['SW_MAX_TILES'] = int(m.group(1))
    m = re.search(r'k_sweep_keys,\s*dim3\(std::min\(blocks_of\(n\),\s*(\d+)u\)\)', sweep)
    assert m, 'the grid cap of k_sweep_keys not found'
    c['SW_KEYS_BLOCKS'] = int(m.group(1))
    assert re.search(r'k_sweep_value,\s*dim3\(std::min\(blocks_of\(n - 1\),\s*\(unsigned\)SW_VALUE_BLOCKS\)\)', sweep), 'the grid of k_sweep_value'
    assert re.search(r'nb_table\s*=\s*\(int\)blocks_of\(table_len,\s*SW_SCAN_BLOCK\)', sweep) and re.search(r'table_len\s*=\s*\(int64_t\)256\s*\*\s*P->tiles', sweep)
    assert re.search(r'nb_diff\s*=\s*\(int\)blocks_of\(n,\s*SW_SCAN_BLOCK\)', sweep)
    for name in ('DIF_B', 'DIF_UPDATE_BLOCKS', 'DIF_MAX_GROUPS', 'DIF_GROUP_NODES', 'DIF_SHORT_LANES', 'DIF_SHORT_ROWS'):
        c[name] = constant(dif, name)
    assert re.search(r'DIF_CP\s*=\s*DIF_B\s*/\s*2\s*;', dif)
    assert re.search(r'nb_el\s*=\s*\(int\)std::min<int64_t>\(DIF_UPDATE_BLOCKS,\s*blocks_of\(n\s*\*\s*DIF_CP\)\)', dif)
    assert re.search(r'std::min<int64_t>\(std::min<int64_t>\(DIF_MAX_GROUPS,\s*batches\),\s*DIF_GROUP_NODES\s*/\s*std::max<int64_t>\(n,\s*1\)\)', dif)
    c['FSR_DOT_BLOCKS'] = constant(fosr, 'FSR_DOT_BLOCKS')
    assert re.search(r'k_fosr_dot,\s*dim3\(std::min\(blocks_of\(n\),\s*\(unsigned\)FSR_DOT_BLOCKS\)\)', fosr)
    c['SP_SHORT_DEG'], c['SP_LONG_DEG'] = constant(header, 'SP_SHORT_DEG'), constant(header, 'SP_LONG_DEG')
    m = re.search(r'int\s+SHORT_LANES\s*=\s*(\d+)\s*,\s*int\s+TURNS\s*=\s*(\d+)\s*,\s*int\s+NODE\s*=\s*(\d+)', header)
    assert m, 'the defaults of RowGeom not found'
    lanes, turns, _ = (int(x) for x in m.groups())
    assert re.search(r'using\s+SweepRows\s*=\s*RowGeom<>\s*;', sweep) and re.search(r'using\s+FsrRows\s*=\s*RowGeom<>\s*;', fosr)
    c['SHORT_ROWS'] = 256 // lanes * turns            # short rows a workgroup of k_sweep_edges, k_fosr_matvec and k_fosr_pick takes
    m = re.search(r'blocks_of\(\s*p\.n_mid\s*,\s*(\d+)\s*\)', header)
    assert m, 'the medium rows of a workgroup in row_grid'
    c['MID_ROWS'] = int(m.group(1))
    assert re.search(r'using\s+DifRows\s*=\s*RowGeom<DIF_SHORT_LANES,\s*DIF_SHORT_ROWS\s*/\s*8,\s*DIF_CP>\s*;', dif)
    return c


CLOSING_STRIDE = 256   # threads of the workgroup that closes the partials: `i += 256`, `c += 256` in every closing loop


def blocks_of(n, per=256):
    return -(-n // per)


def sweep_buffers(n, c):
    """(tile, tiles, nb_table, nb_diff) of csrc/dcr_sweep.hip::sweep_buffers."""
    tile = c['SW_TILE']
    if n > c['SW_MAX_TILES'] * c['SW_TILE']:
        tile = (blocks_of(n, c['SW_MAX_TILES']) + 63) // 64 * 64
    tiles = blocks_of(n, tile)
    return tile, tiles, blocks_of(256 * tiles, c['SW_SCAN_BLOCK']), blocks_of(n, c['SW_SCAN_BLOCK'])


def value_grid(n, c):
    """(workgroups of k_sweep_value, grid-stride trips of its first thread)."""
    grid = min(blocks_of(n - 1), c['SW_VALUE_BLOCKS'])
    return grid, blocks_of(n - 1, grid * 256)


def keys_trips(n, c):
    return blocks_of(n, min(blocks_of(n), c['SW_KEYS_BLOCKS']) * 256)


def diffusion_batches(n, P, c):
    """(groups, nb_el, grid-stride trips of the element-wise kernels) of csrc/dcr_diffusion.hip::diffusion_batches."""
    cp = c['DIF_B'] // 2
    nb_el = min(c['DIF_UPDATE_BLOCKS'], blocks_of(n * cp))
    batches = blocks_of(P, c['DIF_B'])
    groups = max(1, min(c['DIF_MAX_GROUPS'], batches, c['DIF_GROUP_NODES'] // max(n, 1)))
    return groups, nb_el, blocks_of(n * cp, nb_el * 256)


def row_grid(counts, c):
    """row_grid<RowGeom<>> of csrc/dcr_analysis.h for (n_long, n_mid, n_short)."""
    nl, nm, ns = counts
    return nl + blocks_of(nm, c['MID_ROWS']) + blocks_of(ns, c['SHORT_ROWS'])


def dot_trips(n, c):
    return blocks_of(n, min(blocks_of(n), c['FSR_DOT_BLOCKS']) * 256)


# ---- the sizes of the GPU tests: tests/test_scale_thresholds_cpu.py says which boundary each is there for ---------------------------
SORT_SIZES = (524_289, 2_097_152 + 1_025, 4_194_305)    # the sort alone: graphs of a single edge
WHOLE_SMALL, WHOLE_LARGE = 70_001, 524_289              # the whole sweep call
WHOLE_CARRY = 524_288 + 1_500                           # the same with prefixes that READ the 257th block of the scans
DIFFUSION_SIDE, DIFFUSION_P = 182, 17                   # a 182 x 182 lattice, then hubs and isolated nodes
GROUPS_SIDE, GROUPS_P = 100, 6 * 16 + 5                 # groups limited by n
SMALL_GROUPS_P = 8 * 16                                 # groups 2 .. 7 on long3_mid9_short63
FOSR_SMALL, FOSR_LARGE = WHOLE_SMALL, 262_145 + 37      # picks; the power step and the loop


# ---- graphs --------------------------------------------------------------------------------------------------------------------
def _edge_index(lo, hi, n):
    """Both directions of the distinct pairs lo < hi, sorted by (source, target) as spectral_ref._und leaves them."""
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    key = np.unique((lo * n + hi)[lo < hi])
    lo, hi = key // n, key % n
    both = np.sort(np.concatenate([lo * n + hi, hi * n + lo]))
    return np.stack([both // n, both % n])


def _hub_pairs(rng, hubs, pool):
    """hubs: (node, neighbours) pairs; the neighbours are drawn without repetition from 0 .. pool - 1."""
    lo = [np.full(d, node, dtype=np.int64) for node, d in hubs]
    hi = [rng.choice(pool, size=d, replace=False).astype(np.int64) for _, d in hubs]
    return lo, hi


TAIL = 1_000   # nodes at the end of the path that no chord reaches


def chord_graph(n, chords, isolated, hubs=(), seed=0):
    """A path over nodes 0 .. m - 1, m = n - isolated, plus `chords` random chords a node and, per (node, degree) of `hubs`, that
    many random neighbours; the `isolated` nodes have the highest ids (the end of the short rows' list).  Chords and hubs stay
    among the first m - TAIL nodes: the last TAIL nodes of the path hang on one edge, so with the node id as score the best
    prefix is k = m - TAIL (one cut edge), which the last workgroups of k_sweep_value find.  (edge_index, n)."""
    m = n - isolated
    pool = m - TAIL
    rng = np.random.Generator(np.random.PCG64(seed))
    step = np.arange(m - 1, dtype=np.int64)
    hub_lo, hub_hi = _hub_pairs(rng, hubs, pool)
    lo = np.concatenate([step, rng.integers(0, pool, chords * m)] + hub_lo)
    hi = np.concatenate([step + 1, rng.integers(0, pool, chords * m)] + hub_hi)
    return _edge_index(lo, hi, n), n


_GRAPHS = {}


def whole_small():
    """70,001 nodes: a row above 2,048 (node 40,000), rows between 33 and 2,048, three isolated nodes at the end."""
    if 'small' not in _GRAPHS:
        hubs = ((40_000, 2_500), (7, 40), (1_000, 64), (33_333, 700), (68_990, 1_900))
        _GRAPHS['small'] = chord_graph(WHOLE_SMALL, 4, 3, hubs, seed=70)
    return _GRAPHS['small']


def whole_large():
    """524,289 nodes, about four chords a node, 37 isolated nodes at the highest ids."""
    if 'large' not in _GRAPHS:
        _GRAPHS['large'] = chord_graph(WHOLE_LARGE, 4, 37, seed=524)
    return _GRAPHS['large']


def whole_carry():
    """whole_large with 1,499 more nodes.  At 524,289 nodes the scans' 257th block holds element n - 1 alone, the count of the
    whole node set, which no prefix reads; here it holds 1,500 counts, of which k_sweep_value reads 1,499."""
    if 'carry' not in _GRAPHS:
        _GRAPHS['carry'] = chord_graph(WHOLE_CARRY, 4, 37, seed=525)
    return _GRAPHS['carry']


def fosr_large():
    """262,145 nodes on a path with a chord a node, then 37 isolated nodes."""
    if 'fosr' not in _GRAPHS:
        _GRAPHS['fosr'] = chord_graph(FOSR_LARGE, 1, 37, seed=262)
    return _GRAPHS['fosr']


def single_edge(n):
    """The graph of the sort-alone tests: the sort does not read it."""
    return np.array([[0, 1], [1, 0]], dtype=np.int64), n


def lattice_graph(side, hub_degrees, isolated, chords=0, seed=0):
    """A side x side lattice (row-major), then one node per entry of hub_degrees joined to that many random lattice nodes, then
    `isolated` nodes; `chords` random chords on the lattice in all.  (edge_index, n, names): names has 'hub<i>', 'corner',
    'isolated' (the first of them) and 'last'."""
    m = side * side
    n = m + len(hub_degrees) + isolated
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = np.arange(m, dtype=np.int64).reshape(side, side)
    hub_lo, hub_hi = _hub_pairs(rng, [(m + i, d) for i, d in enumerate(hub_degrees)], m)
    lo = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel(), rng.integers(0, m, chords)] + hub_lo)
    hi = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel(), rng.integers(0, m, chords)] + hub_hi)
    names = {f'hub{i}': m + i for i in range(len(hub_degrees))}
    names.update(corner=0, isolated=m + len(hub_degrees), last=n - 1)
    return _edge_index(lo, hi, n), n, names


def diffusion_large():
    """33,124 lattice nodes, a hub of 2,100, four medium rows, four isolated nodes: n = 33,133 > 32,768.  No chords and no
    heavier medium rows: they triple the fill of the sparse LU that tests/test_diffusion_gpu.py compares with (0.6 s as it is)."""
    if 'dif' not in _GRAPHS:
        _GRAPHS['dif'] = lattice_graph(DIFFUSION_SIDE, (2_100, 33, 40, 64, 300), 4, seed=33)
    return _GRAPHS['dif']


def diffusion_groups():
    """10,000 lattice nodes, a hub, two medium rows, three isolated nodes: 65,536 // n = 6 groups."""
    if 'groups' not in _GRAPHS:
        _GRAPHS['groups'] = lattice_graph(GROUPS_SIDE, (2_100, 50, 400), 3, chords=100, seed=10)
    return _GRAPHS['groups']


def degrees(edge_index, n):
    return np.bincount(np.asarray(edge_index)[0], minlength=n)


def class_counts(deg, c):
    """(n_long, n_mid, n_short) of csrc/dcr_analysis.hip::classify_rows."""
    nl, ns = int((deg > c['SP_LONG_DEG']).sum()), int((deg <= c['SP_SHORT_DEG']).sum())
    return nl, deg.shape[0] - nl - ns, ns
