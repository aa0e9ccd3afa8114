"""The sizes at which the sweep, diffusion, FoSR, resistance and hop kernels change their control flow, and the graphs the GPU tests
use there (host only).  The constants are read out of csrc/*.hip and csrc/dcr_analysis.h, the launch arithmetic of sweep_buffers,
diffusion_batches, resistance_batches, the hop count and row_grid is restated in Python, and tests/test_scale_thresholds_cpu.py
asserts that every size named here sits just past the boundary it is there for.  The graphs are built with array operations
only: a Python loop over half a million nodes costs more than the kernels under test."""
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
    for name in ('DIF_MAX_GROUPS', 'DIF_GROUP_NODES'):
        c[name] = constant(dif, name)
    assert re.search(r'nb_el\s*=\s*\(int\)std::min<int64_t>\(COL_UPDATE_BLOCKS,\s*blocks_of\(n\s*\*\s*COL_CP\)\)', dif), 'nb_el of diffusion_batches'
    assert re.search(r'nb_mv\s*=\s*\(int\)row_grid<ColRows>\(plan\)', dif)
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
    c.update(column_and_hops_constants())
    c.update(sketch_constants())
    return c


def sketch_constants():
    """The constants of csrc/dcr_resistance_sketch.hip that the sizes of tests/test_resistance_sketch_limits_gpu.py depend on;
    the group rule and the grid of k_sketch_pairs are asserted to be spelled as sketch_groups and sketch_pair_grid restate them."""
    skt = source('dcr_resistance_sketch.hip')
    c = {name: constant(skt, name) for name in ('SKT_MAX_GROUPS', 'SKT_GROUP_NODES', 'SKT_PAIR_BLOCKS')}
    assert re.search(r'int64_t\s+cap\s*=\s*SKT_MAX_GROUPS\s*;', skt), 'the cap of sketch_groups'
    assert re.search(r'std::max<int64_t>\(1,\s*std::min<int64_t>\(std::min<int64_t>\(cap,\s*batches\),\s*SKT_GROUP_NODES\s*/\s*'
                     r'std::max<int64_t>\(n,\s*1\)\)\)', skt), 'the rule of sketch_groups'
    assert re.search(r'first\s*<\s*batches;\s*first\s*\+=\s*R\.groups\)', skt) and re.search(
        r'ng\s*=\s*\(int\)std::min<int64_t>\(R\.groups,\s*batches\s*-\s*first\)', skt), 'the launches of dcr_resistance_sketch'
    assert re.search(r'k_sketch_pairs,\s*dim3\(std::min\(blocks_of\(P\s*\*\s*COL_CP\),\s*\(unsigned\)SKT_PAIR_BLOCKS\)\)', skt), 'the grid of k_sketch_pairs'
    assert re.search(r'e\s*=\s*\(int64_t\)blockIdx\.x\s*\*\s*256\s*\+\s*threadIdx\.x;\s*e\s*<\s*total;\s*e\s*\+=\s*\(int64_t\)gridDim\.x\s*\*\s*256\)', skt) \
        and re.search(r'total\s*=\s*P\s*\*\s*COL_CP\s*;', skt) and re.search(r'i\s*=\s*e\s*/\s*COL_CP\s*;', skt), 'the loop of k_sketch_pairs'
    return c


def column_and_hops_constants():
    """The constants of the column CG in csrc/dcr_analysis.h, which the resistance and diffusion solves share, and of
    csrc/dcr_hops.hip, that DIFFUSION_SIDE, RESISTANCE_SIZE, HOPS_SMALL and HOPS_LARGE depend on ('COL_B' is the default of
    '#define DCR_COL_B', which is what the library is built with)."""
    header, res, hops = source('dcr_analysis.h'), source('dcr_resistance.hip'), source('dcr_hops.hip')
    c = {name: constant(header, name) for name in ('COL_UPDATE_BLOCKS', 'COL_SHORT_LANES', 'COL_SHORT_ROWS')}
    m = re.search(r'#ifndef\s+DCR_COL_B\s*\n\s*#define\s+DCR_COL_B\s+(\d+)', header)
    assert m, 'the default of DCR_COL_B not found'
    c['COL_B'] = int(m.group(1))
    assert re.search(r'constexpr\s+int\s+COL_B\s*=\s*DCR_COL_B\s*;', header) and re.search(r'constexpr\s+int\s+COL_CP\s*=\s*COL_B\s*/\s*2\s*;', header)
    c['COL_CP'] = c['COL_B'] // 2
    assert re.search(r'nb_el\s*=\s*\(int\)std::min<int64_t>\(COL_UPDATE_BLOCKS,\s*blocks_of\(n\s*\*\s*COL_CP\)\)', res), 'nb_el of resistance_batches'
    assert re.search(r'nb_mv\s*=\s*\(int\)row_grid<ColRows>\(plan\)', res)
    assert re.search(r'using\s+ColRows\s*=\s*RowGeom<COL_SHORT_LANES,\s*COL_SHORT_ROWS\s*/\s*8,\s*COL_CP>\s*;', header)
    assert len(re.findall(r'e\s*<\s*total;\s*e\s*\+=\s*\(int64_t\)gridDim\.x\s*\*\s*256\)', header)) == 4, 'the four grid-stride loops over n * COL_CP'
    assert re.search(r'i\s*<\s*count;\s*i\s*\+=\s*256\s*/\s*COL_CP\)', header), 'the stride of the column close_partials'
    c['HOP_COUNT_BLOCKS'] = constant(hops, 'HOP_COUNT_BLOCKS')
    assert re.search(r'k_hop_count<W>,\s*dim3\(std::min\(blocks_of\(\(n\s*\+\s*63\)\s*/\s*64,\s*4\),\s*\(unsigned\)HOP_COUNT_BLOCKS\)\)', hops), 'the grid of k_hop_count'
    assert re.search(r'c\s*=\s*\(int64_t\)blockIdx\.x\s*\*\s*4\s*\+\s*wave;\s*c\s*<\s*chunks;\s*c\s*\+=\s*\(int64_t\)gridDim\.x\s*\*\s*4\)', hops), 'the chunk loop of k_hop_count'
    assert re.search(r'k_hop_level<W>,\s*dim3\(row_grid<HopRows>\(plan\)\)', hops) and re.search(r'using\s+HopRows\s*=\s*RowGeom<>\s*;', hops)
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
    nb_el = min(c['COL_UPDATE_BLOCKS'], blocks_of(n * c['COL_CP']))
    batches = blocks_of(P, c['COL_B'])
    groups = max(1, min(c['DIF_MAX_GROUPS'], batches, c['DIF_GROUP_NODES'] // max(n, 1)))
    return groups, nb_el, blocks_of(n * c['COL_CP'], nb_el * 256)


def row_grid(counts, c, short_rows=None):
    """row_grid<RowGeom<>> of csrc/dcr_analysis.h for (n_long, n_mid, n_short); short_rows: those of another geometry."""
    nl, nm, ns = counts
    return nl + blocks_of(nm, c['MID_ROWS']) + blocks_of(ns, short_rows or c['SHORT_ROWS'])


def resistance_elementwise(n, c):
    """(nb_el, grid-stride trips, elements of the last trip) of k_col_start / update / direction / scale over n * COL_CP elements."""
    total = n * c['COL_CP']
    nb_el = min(c['COL_UPDATE_BLOCKS'], blocks_of(total))
    trips = blocks_of(total, nb_el * 256)
    return nb_el, trips, total - (trips - 1) * nb_el * 256


def hop_count_grid(n, c):
    """(workgroups of k_hop_count, trips of its chunk loop): four waves a workgroup, 64 nodes a wave and trip."""
    chunks = blocks_of(n, 64)
    grid = min(blocks_of(chunks, 4), c['HOP_COUNT_BLOCKS'])
    return grid, blocks_of(chunks, 4 * grid)


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
RESISTANCE_SIZE = DIFFUSION_SIDE ** 2 + 5 + 4           # diffusion_large(): the element-wise kernels of the resistance on a second trip
HOPS_SMALL, HOPS_LARGE = WHOLE_SMALL, FOSR_LARGE        # many workgroups of k_hop_level; the chunk loop of k_hop_count on a second trip


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


# ---- what the resistance and hop tests ask at those sizes (tests/test_resistance_gpu.py, tests/test_hops_gpu.py) -------------------
SECOND_TRIP = 32_768   # the first node of diffusion_large() that the element-wise resistance kernels take on their second trip


def resistance_pairs():
    """(pairs int64 [19, 2], solved [17], names) on diffusion_large(): 17 pairs that take a column, so the second batch of 16 has
    15 padding columns, and two that the host decides (one with an isolated node, one u == v), which take none."""
    _, n, names = diffusion_large()
    side, hub0 = DIFFUSION_SIDE, names['hub0']
    pairs = np.array([
        (hub0, names['corner']),                 # 0: the long row and node 0
        (SECOND_TRIP + 32, 0),                   # 1: a lattice node of the second trip and node 0
        (33_000, 33_100),                        # 2: both in the second trip
        (5_000, 5_001),                          # 3: the two ends of a lattice edge, first trip
        (hub0, names['hub3']),                   # 4: the long row and a medium row
        (names['isolated'], 7),                  # 5: across components: inf, no column
        (12_345, 12_345),                        # 6: u == v: 0, no column
        (33_000, 33_001),                        # 7: a lattice edge inside the second trip
        (SECOND_TRIP - 1, SECOND_TRIP),          # 8: the lattice edge across the trip boundary
        (side * side - 1, 0),                    # 9: opposite corners
        (names['hub1'], SECOND_TRIP),            # 10: a medium row of 33 (the smallest) and the first node of the second trip
        (names['hub2'], names['hub4']),          # 11: two medium rows
        (side * side - 1, hub0),                 # 12: the last lattice node and the long row, neighbours in id
        (side - 1, side * (side - 1)),           # 13: the other two corners
        (91 * side + 91, hub0),                  # 14: the lattice's centre
        (names['hub4'], 20_000),                 # 15
        (SECOND_TRIP + 200, 16_000),             # 16
        (1, 2 * side),                           # 17: two hops apart near the corner
        (33_100, names['hub2']),                 # 18: the 17th solved pair: alone in the second batch
    ], dtype=np.int64)
    solved = np.array([i for i in range(len(pairs)) if i not in (5, 6)])
    return pairs, solved, names


# ---- the resistance sketch at its group counts and past the grid of k_sketch_pairs (tests/test_resistance_sketch_limits_gpu.py) -----
def sketch_groups(n, batches, c, env=None):
    """sketch_groups of csrc/dcr_resistance_sketch.hip; env: the value of DCR_SKETCH_GROUPS, honoured in 1 .. SKT_MAX_GROUPS."""
    cap = env if env is not None and 1 <= env <= c['SKT_MAX_GROUPS'] else c['SKT_MAX_GROUPS']
    return max(1, min(cap, batches, c['SKT_GROUP_NODES'] // max(n, 1)))


def sketch_launches(n, columns, c, env=None):
    """The group count of every launch of one dcr_resistance_sketch call, in order."""
    batches = blocks_of(columns, c['COL_B'])
    groups = sketch_groups(n, batches, c, env)
    return [min(groups, batches - first) for first in range(0, batches, groups)]


def sketch_pair_grid(P, c):
    """(workgroups of k_sketch_pairs, trips of its loop, pairs of the last trip)."""
    grid = min(blocks_of(P * c['COL_CP']), c['SKT_PAIR_BLOCKS'])
    per_trip = grid * 256 // c['COL_CP']
    trips = blocks_of(P, per_trip)
    return grid, trips, P - (trips - 1) * per_trip


def sketch_three_groups():
    """16,900 lattice nodes, a hub of 2,100, two medium rows, three isolated nodes: 65,536 // 16,906 = 3 groups."""
    if 'skt3' not in _GRAPHS:
        _GRAPHS['skt3'] = lattice_graph(130, [2100, 40, 300], 3)
    return _GRAPHS['skt3']


def sketch_two_groups():
    """22,500 lattice nodes and the same hubs and isolated nodes: 65,536 // 22,506 = 2 groups."""
    if 'skt2' not in _GRAPHS:
        _GRAPHS['skt2'] = lattice_graph(150, [2100, 40, 300], 3)
    return _GRAPHS['skt2']


# name -> (graph, columns, launches): the large graphs of the sketch's limit tests
SKETCH_LARGE = {'sketch_three_groups': (sketch_three_groups, 80, [3, 2]), 'sketch_two_groups': (sketch_two_groups, 48, [2, 1]),
                'diffusion_large': (diffusion_large, 20, [1, 1])}
SKETCH_SMALL_COLUMNS = {48: [3], 112: [4, 3]}     # on random300 and barbell_20_4: a launch of three groups alone, and four then three

PAIRS_EXTRA = 37       # pairs past SKT_PAIR_BLOCKS workgroups
FIXED_PAIR_AT = 5      # the fixed pair sits at 0, at FIXED_PAIR_AT and at the same offset into the second trip


def sketch_pairs_past_cap(n, names, c, side, seed=77):
    """(pairs int64 [P, 2], marks) with P = SKT_PAIR_BLOCKS * 256 / COL_CP + PAIRS_EXTRA on a lattice_graph of ``side`` with
    ``names``: seeded pairs of connected nodes, and at indices of the first trip of k_sketch_pairs and of the second (marks: name
    -> the two indices, first trip then second) a pair u == v ('same'), one with an isolated node ('isolated', 'isolated_last'),
    the hub with a lattice node ('hub'), and the pair marks['fixed'] at 0 as well ('fixed': 0, first trip, second trip)."""
    per_trip = c['SKT_PAIR_BLOCKS'] * 256 // c['COL_CP']
    P = per_trip + PAIRS_EXTRA
    rng = np.random.Generator(np.random.PCG64(seed))
    pairs = rng.integers(0, names['isolated'], size=(P, 2))      # lattice nodes and hubs: one component
    hub, iso, last = names['hub0'], names['isolated'], names['last']
    fixed = (hub, side * side // 2 + 7)
    marks = {'fixed': (0, FIXED_PAIR_AT, per_trip + FIXED_PAIR_AT), 'same': (100, per_trip + 1), 'isolated': (1_000, per_trip + 2),
             'isolated_last': (20_000, P - 1), 'hub': (per_trip - 1, per_trip), 'pair': fixed}
    for i in marks['fixed']:
        pairs[i] = fixed
    pairs[marks['same'][0]] = (4_321, 4_321)
    pairs[marks['same'][1]] = (hub, hub)
    pairs[marks['isolated'][0]] = (iso, 9)
    pairs[marks['isolated'][1]] = (11, iso + 1)
    pairs[marks['isolated_last'][0]] = (last, hub)
    pairs[marks['isolated_last'][1]] = (iso, last)               # two isolated nodes: two components
    pairs[marks['hub'][0]] = (hub, 0)
    pairs[marks['hub'][1]] = (side * side - 1, hub)
    return pairs.astype(np.int64), marks


def hop_sources_small():
    """21 sources of whole_small(): the long row, a medium row, node 0, an isolated node, the last node, the last connected one."""
    rng = np.random.Generator(np.random.PCG64(71))
    n = WHOLE_SMALL
    return np.concatenate([[40_000, 33_333, 0, n - 3, n - 1, n - 4], rng.integers(0, n, 15)]).astype(np.int32)


def hop_sources_large():
    """130 sources of fosr_large(): two full words and two bits of a third.  They are 26 nodes five times each, in shuffled order,
    so that the host reference searches 26 times (0.06 s a search: its levels are a thousand numpy steps) while the device gives
    every one of the 130 bits a search of its own.  Node 262,144 (the one connected node of the second trip of k_hop_count) has
    a bit in each of the three words, the isolated last node and node 0 sit at the word boundaries."""
    rng = np.random.Generator(np.random.PCG64(262))
    n = HOPS_LARGE
    nodes = np.concatenate([[262_144, n - 1, 0, n - 20, 5], rng.choice(np.arange(6, n - 37), size=21, replace=False)])
    fixed = {0: 262_144, 63: n - 1, 64: 262_144, 127: 0, 128: 262_144, 129: 0}
    pool = np.tile(nodes, 5).tolist()
    for node in fixed.values():
        pool.remove(node)
    pool = rng.permutation(pool)
    src = np.empty(130, dtype=np.int32)
    free = [i for i in range(130) if i not in fixed]
    src[free] = pool
    src[list(fixed)] = list(fixed.values())
    return src
