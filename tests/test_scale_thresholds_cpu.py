"""Where the sweep, diffusion, FoSR, resistance and hop kernels change their control flow, on the CPU: the constants are read out
of the sources (tests/scale_ref.py), the launch arithmetic of sweep_buffers, diffusion_batches, resistance_batches, the hop count
and row_grid is restated there, and every size that tests/test_sweep_gpu.py, tests/test_diffusion_gpu.py, tests/test_fosr_gpu.py,
tests/test_resistance_gpu.py and tests/test_hops_gpu.py run at is asserted to sit just past the boundary it is there for, with
the size below it on the other side.  A failure names the GPU size that a changed constant has left stale."""
import numpy as np
import pytest

import scale_ref as sc
import spectral_ref


@pytest.fixture(scope='module')
def c():
    return sc.constants()


def test_constants_are_those_the_sizes_were_chosen_for(c):
    """Not a demand on the kernels: a changed constant is allowed, and the tests below then say which size moved.  This one only
    prints what was read and pins what the restatement itself assumes."""
    print('  ' + ', '.join(f'{k} = {v}' for k, v in c.items()))
    assert sc.CLOSING_STRIDE == 256
    assert c['SP_SHORT_DEG'] == spectral_ref.SHORT_DEG and c['SP_LONG_DEG'] == spectral_ref.LONG_DEG
    assert c['COL_B'] % 2 == 0 and c['SW_SCAN_BLOCK'] == 8 * 256   # eight elements a thread


# ---- the sweep -----------------------------------------------------------------------------------------------------------------------
def test_sweep_value_closing_loop_and_grid_caps(c):
    stale = 'stale GPU size: scale_ref.WHOLE_SMALL (the closing loop of k_sweep_value past 256 partials)'
    grid, trips = sc.value_grid(sc.WHOLE_SMALL, c)
    assert sc.CLOSING_STRIDE < grid < c['SW_VALUE_BLOCKS'] and trips == 1, stale
    at = sc.CLOSING_STRIDE * 256 + 1                        # the largest n with 256 partials
    assert sc.value_grid(at, c)[0] == sc.CLOSING_STRIDE and sc.value_grid(at + 1, c)[0] == sc.CLOSING_STRIDE + 1, stale
    assert sc.sweep_buffers(sc.WHOLE_SMALL, c)[3] <= sc.CLOSING_STRIDE, stale   # and nothing else yet
    stale = 'stale GPU size: scale_ref.WHOLE_LARGE (second grid-stride trip of k_sweep_keys and k_sweep_value)'
    assert sc.value_grid(sc.WHOLE_LARGE, c) == (c['SW_VALUE_BLOCKS'], 2) and sc.keys_trips(sc.WHOLE_LARGE, c) == 3, stale
    assert sc.WHOLE_LARGE % (c['SW_KEYS_BLOCKS'] * 256) == 1, stale             # the third trip of k_sweep_keys holds the last key alone
    at = c['SW_KEYS_BLOCKS'] * 256
    assert sc.keys_trips(at, c) == 1 and sc.keys_trips(at + 1, c) == 2, stale
    assert sc.value_grid(at + 1, c)[1] == 1 and sc.value_grid(at + 2, c)[1] == 2, stale


def test_scan_closing_loop_on_the_difference_arrays(c):
    stale = 'stale GPU size: scale_ref.WHOLE_LARGE and SORT_SIZES[0] (carry of k_scan_reduce, difference arrays)'
    n = sc.WHOLE_LARGE
    assert n == sc.SORT_SIZES[0]
    assert sc.sweep_buffers(n, c)[3] == sc.CLOSING_STRIDE + 1 and sc.sweep_buffers(n - 1, c)[3] == sc.CLOSING_STRIDE, stale
    assert sc.sweep_buffers(n, c)[:3] == (c['SW_TILE'], 513, 65), stale        # the sort table is still within one trip


def test_scan_carry_is_read_by_a_prefix(c):
    """nb_diff = 257 is not enough: at 524,289 nodes the 257th block is element n - 1, the count of all nodes, and k_sweep_value
    stops at n - 2.  WHOLE_CARRY puts 1,499 valued prefixes into that block, isolated nodes and the chord-free tail among them."""
    stale = 'stale GPU size: scale_ref.WHOLE_CARRY (carry of k_scan_reduce read by k_sweep_value)'
    first = sc.CLOSING_STRIDE * c['SW_SCAN_BLOCK']          # the first element of the 257th block
    assert sc.WHOLE_LARGE - 2 < first, stale                # the issue's size: no prefix in it
    n = sc.WHOLE_CARRY
    assert sc.sweep_buffers(n, c)[3] == sc.CLOSING_STRIDE + 1 and (n - 2) - first + 1 == 1_499, stale
    assert sc.value_grid(n, c) == (c['SW_VALUE_BLOCKS'], 3), stale


def test_best_prefix_of_the_id_score_lies_in_the_last_workgroups(c):
    """With the node id as score the best prefix ends where the chord-free tail begins (one cut edge).  Its arg-min partial has an
    index above 256, so the closing loop of k_sweep_value must carry it on a later trip; at the larger sizes the prefix itself
    is taken on the second or third grid-stride trip."""
    import sweep_ref
    for build, n in ((sc.whole_small, sc.WHOLE_SMALL), (sc.whole_large, sc.WHOLE_LARGE), (sc.whole_carry, sc.WHOLE_CARRY)):
        ei, _ = build()
        isolated = int((sc.degrees(ei, n) == 0).sum())
        want = sweep_ref.sweep(ei, n, np.arange(n, dtype=np.float64), 'conductance')
        assert want.size == n - isolated - sc.TAIL and want.counts[1] + want.counts[2] == 1, (n, want.size)
        grid, trips = sc.value_grid(n, c)
        index = want.size - 1
        assert index // (256 * grid) == trips - 1, f'stale GPU size: {n} (the best prefix on the last grid-stride trip)'
        if n != sc.WHOLE_CARRY:   # (there the third trip starts over at workgroup 0, which takes it)
            assert (index // 256) % grid >= sc.CLOSING_STRIDE, f'stale GPU size: {n} (closing loop of k_sweep_value)'


def test_scan_closing_loop_on_the_sort_table(c):
    stale = 'stale GPU size: scale_ref.SORT_SIZES[1] (carry of k_scan_reduce, sort table)'
    n = sc.SORT_SIZES[1]
    tile, tiles, nb_table, nb_diff = sc.sweep_buffers(n, c)
    assert (tile, tiles, nb_table) == (c['SW_TILE'], 2050, sc.CLOSING_STRIDE + 1), stale
    at = sc.CLOSING_STRIDE * c['SW_SCAN_BLOCK'] // 256 * c['SW_TILE']           # 2,048 tiles: the last n with 256 blocks
    assert sc.sweep_buffers(at, c)[2] == sc.CLOSING_STRIDE and sc.sweep_buffers(at + 1, c)[2] == sc.CLOSING_STRIDE + 1, stale
    assert at < n <= at + 2 * c['SW_TILE'] and tiles % 4 != 0 and n % tile == 1, stale   # a last tile of one key, a last workgroup of two waves


def test_sort_tiles_beyond_the_tile_limit(c):
    stale = 'stale GPU size: scale_ref.SORT_SIZES[2] (tile above SW_TILE, tiles capped)'
    n = sc.SORT_SIZES[2]
    at = c['SW_MAX_TILES'] * c['SW_TILE']
    assert n == at + 1, stale
    assert sc.sweep_buffers(at, c)[:2] == (c['SW_TILE'], c['SW_MAX_TILES']), stale
    tile, tiles, nb_table, nb_diff = sc.sweep_buffers(n, c)
    assert tile == c['SW_TILE'] + 64 and tile % 64 == 0 and tiles < c['SW_MAX_TILES'] and tiles * tile >= n > (tiles - 1) * tile, stale
    assert nb_diff > 8 * sc.CLOSING_STRIDE and nb_table > sc.CLOSING_STRIDE, stale


# ---- diffusion -----------------------------------------------------------------------------------------------------------------------
def test_diffusion_elementwise_second_trip(c):
    stale = 'stale GPU size: scale_ref.DIFFUSION_SIDE (second grid-stride trip of k_col_start / update / direction / scale in diffusion_batches)'
    ei, n, names = sc.diffusion_large()
    at = c['COL_UPDATE_BLOCKS'] * 256 // c['COL_CP']   # 32,768: the largest n of one trip
    assert sc.diffusion_batches(at, sc.DIFFUSION_P, c)[1:] == (c['COL_UPDATE_BLOCKS'], 1), stale
    assert sc.diffusion_batches(at + 1, sc.DIFFUSION_P, c)[1:] == (c['COL_UPDATE_BLOCKS'], 2), stale
    groups, nb_el, trips = sc.diffusion_batches(n, sc.DIFFUSION_P, c)
    assert at < n < at + at // 16 and (groups, nb_el, trips) == (1, c['COL_UPDATE_BLOCKS'], 2), stale
    assert -(-sc.DIFFUSION_P // (groups * c['COL_B'])) == 2, stale              # two launches
    # every class of the mat-vec, and the sources the test names
    deg = sc.degrees(ei, n)
    nl, nm, ns = sc.class_counts(deg, c)
    assert nl == 1 and nm == 4 and deg[names['hub0']] == 2100 > c['SP_LONG_DEG'] and deg[names['hub1']] == c['SP_SHORT_DEG'] + 1, stale
    assert deg[names['isolated']] == 0 and deg[names['last']] == 0 and 2 <= deg[names['corner']] <= c['SP_SHORT_DEG'] and (deg == 0).sum() == 4
    mv_grid = nl + sc.blocks_of(nm, c['MID_ROWS']) + sc.blocks_of(ns, c['COL_SHORT_ROWS'])
    assert mv_grid > 2 * (256 // c['COL_CP']), stale                      # the column close_partials: more than one trip of 32 partials


def test_diffusion_groups_limited_by_n(c):
    stale = 'stale GPU size: scale_ref.GROUPS_SIDE / GROUPS_P (group count limited by n)'
    ei, n, names = sc.diffusion_groups()
    groups = sc.diffusion_batches(n, sc.GROUPS_P, c)[0]
    assert groups == c['DIF_GROUP_NODES'] // n == 6 < min(c['DIF_MAX_GROUPS'], sc.blocks_of(sc.GROUPS_P, c['COL_B'])), stale
    assert sc.GROUPS_P == groups * c['COL_B'] + 5, stale                         # a full launch of six groups, then five columns
    assert c['DIF_GROUP_NODES'] // c['DIF_MAX_GROUPS'] < n, stale
    deg = sc.degrees(ei, n)
    assert sc.class_counts(deg, c)[:2] == (1, 2) and deg[names['last']] == 0


def test_diffusion_all_eight_groups_at_small_n(c):
    stale = 'stale GPU size: scale_ref.SMALL_GROUPS_P (groups 2 .. 7 of one launch)'
    n = next(m for name, e, m in spectral_ref.plan_family() if name == 'long3_mid9_short63')
    assert sc.diffusion_batches(n, sc.SMALL_GROUPS_P, c)[0] == c['DIF_MAX_GROUPS'] == 8, stale
    assert sc.SMALL_GROUPS_P == c['DIF_MAX_GROUPS'] * c['COL_B'] and n <= c['DIF_GROUP_NODES'] // c['DIF_MAX_GROUPS'], stale
    assert sc.diffusion_batches(n, 17, c)[0] == 2      # what the batch-independence test of the plan family reaches


# ---- FoSR ----------------------------------------------------------------------------------------------------------------------------
def test_fosr_closing_loops_and_dot_cap(c):
    stale = 'stale GPU size: scale_ref.FOSR_SMALL (closing loop of k_fosr_pick, close_partials of k_fosr_matvec past 256 workgroups)'
    ei, n = sc.whole_small()
    deg = sc.degrees(ei, n)
    counts = sc.class_counts(deg, c)
    grid = sc.row_grid(counts, c)
    print(f'  n = {n}: classes {counts}, row grid {grid}')
    assert counts[0] == 1 and counts[1] >= 4 and grid > 8 * sc.CLOSING_STRIDE, stale
    assert sc.row_grid((0, 0, sc.CLOSING_STRIDE * c['SHORT_ROWS']), c) == sc.CLOSING_STRIDE, stale   # 8,192 short rows: one trip
    assert sc.row_grid((0, 0, sc.CLOSING_STRIDE * c['SHORT_ROWS'] + 1), c) == sc.CLOSING_STRIDE + 1, stale
    assert sc.dot_trips(n, c) == 1 and sc.blocks_of(n) > sc.CLOSING_STRIDE, stale
    assert (deg[-3:] == 0).all() and deg[-4] > 0 and counts[2] % c['SHORT_ROWS'] >= 2, stale     # the last two rows share the last workgroup
    stale = 'stale GPU size: scale_ref.FOSR_LARGE (second grid-stride trip of k_fosr_dot)'
    ei, n = sc.fosr_large()
    at = c['FSR_DOT_BLOCKS'] * 256
    assert sc.dot_trips(at, c) == 1 and sc.dot_trips(at + 1, c) == 2, stale
    assert at < n <= at + 64 and sc.dot_trips(n, c) == 2, stale
    deg = sc.degrees(ei, n)
    counts = sc.class_counts(deg, c)
    assert counts[:2] == (0, 0) and (deg[-37:] == 0).all() and deg[-38] > 0 and counts[2] % c['SHORT_ROWS'] >= 2, stale


def test_whole_call_graphs_are_what_the_gpu_tests_rely_on(c):
    ei, n = sc.whole_small()
    deg = sc.degrees(ei, n)
    assert n == sc.WHOLE_SMALL and ei.shape[1] % 2 == 0 and (ei[0] != ei[1]).all()
    assert deg[40_000] > c['SP_LONG_DEG'] and (deg > c['SP_LONG_DEG']).sum() == 1
    assert ((deg > c['SP_SHORT_DEG']) & (deg <= c['SP_LONG_DEG'])).sum() >= 4
    ei, n = sc.whole_large()
    deg = sc.degrees(ei, n)
    assert n == sc.WHOLE_LARGE and (deg[-37:] == 0).all() and (deg[:-37] > 0).all() and 9.5 < deg.mean() < 10.0
    assert np.array_equal(ei[0] * n + ei[1], np.unique(ei[0] * n + ei[1]))      # sorted, no repeats: ascending rows
    assert ei.shape[1] < 2 ** 31


# ---- effective resistance ------------------------------------------------------------------------------------------------------------
def test_resistance_elementwise_second_trip(c):
    stale = ('stale GPU size: scale_ref.RESISTANCE_SIZE (COL_UPDATE_BLOCKS / DCR_COL_B: second grid-stride trip of k_col_start / update / '
             'direction / scale in resistance_batches, tests/test_resistance_gpu.py::test_past_the_cap_*)')
    ei, n, names = sc.diffusion_large()
    assert n == sc.RESISTANCE_SIZE
    at = 256 * c['COL_UPDATE_BLOCKS'] // c['COL_CP']                              # 32,768: the largest n of one trip
    assert at == sc.SECOND_TRIP, stale
    assert sc.resistance_elementwise(at, c)[:2] == (c['COL_UPDATE_BLOCKS'], 1), stale
    assert sc.resistance_elementwise(at + 1, c)[:2] == (c['COL_UPDATE_BLOCKS'], 2), stale
    nb_el, trips, last = sc.resistance_elementwise(n, c)
    assert n * c['COL_CP'] > 256 * c['COL_UPDATE_BLOCKS'] and (nb_el, trips) == (c['COL_UPDATE_BLOCKS'], 2), stale
    assert 0 < last < nb_el * 256 and last == (n - at) * c['COL_CP'], stale       # ragged: fewer elements than one full grid
    assert last % 256 != 0, stale                                                 # and its last workgroup is partly filled
    assert nb_el == 32 * (256 // c['COL_CP']), stale                              # the column close_partials: 32 partials a thread group
    # what lies in the second trip: the lattice's tail, every hub and every isolated node; every pair the GPU test names
    deg = sc.degrees(ei, n)
    assert names['hub0'] >= at and deg[names['hub0']] > c['SP_LONG_DEG'], stale
    assert all(names[f'hub{i}'] >= at and c['SP_SHORT_DEG'] < deg[names[f'hub{i}']] <= c['SP_LONG_DEG'] for i in range(1, 5)), stale
    assert (deg[-4:] == 0).all() and (deg[:-4] > 0).all() and names['isolated'] == n - 4 >= at, stale
    assert sc.DIFFUSION_SIDE ** 2 - at >= 256, stale                               # a few hundred lattice nodes past the boundary
    pairs, solved, _ = sc.resistance_pairs()
    assert len(solved) == c['COL_B'] + 1 and len(pairs) == len(solved) + 2, stale   # the second batch: one column, 15 padded
    assert (pairs[solved][:, 0] != pairs[solved][:, 1]).all() and (deg[pairs[solved]] > 0).all()
    assert (pairs[2] >= at).all() and (pairs[7] >= at).all() and pairs[1, 0] >= at > pairs[1, 1] and (pairs[18] >= at).all(), stale
    assert pairs[8, 0] == at - 1 and pairs[8, 1] == at, stale
    edge = set(map(tuple, ei.T.tolist()))
    assert all(tuple(pairs[i]) in edge for i in (3, 7, 8))                          # lattice edges
    assert deg[pairs[5, 0]] == 0 and pairs[6, 0] == pairs[6, 1]
    # the mat-vec's grid: more than one step a thread group of the column close_partials, here and on the 70,001-node graph
    grid = sc.row_grid(sc.class_counts(deg, c), c, c['COL_SHORT_ROWS'])
    assert grid > 2 * (256 // c['COL_CP']), stale


def test_resistance_and_hop_matvec_grids_past_256_workgroups(c):
    ei, n = sc.whole_small()
    counts = sc.class_counts(sc.degrees(ei, n), c)
    assert c['COL_SHORT_ROWS'] == 256 // c['COL_SHORT_LANES'] * 8                   # RowGeom<COL_SHORT_LANES, COL_SHORT_ROWS / 8, ..>
    res_grid, hop_grid = sc.row_grid(counts, c, c['COL_SHORT_ROWS']), sc.row_grid(counts, c)
    print(f'  n = {n}: row_grid<ColRows> {res_grid}, row_grid<HopRows> {hop_grid}')
    assert res_grid > sc.CLOSING_STRIDE, 'stale GPU size: scale_ref.WHOLE_SMALL (COL_SHORT_ROWS: row_grid<ColRows> past 256 workgroups)'
    assert hop_grid > sc.CLOSING_STRIDE, ('stale GPU size: scale_ref.HOPS_SMALL (RowGeom<>: row_grid<HopRows> past 256 workgroups, '
                                          'tests/test_hops_gpu.py::test_rows_and_summary_at_70001_nodes)')


# ---- the resistance sketch -----------------------------------------------------------------------------------------------------------
def test_sketch_group_counts_and_launches(c):
    stale = 'stale GPU size: scale_ref.SKETCH_LARGE / SKETCH_SMALL_COLUMNS (SKT_MAX_GROUPS, SKT_GROUP_NODES: the groups of a launch)'
    import resistance_sketch_ref as skref
    assert c['SKT_MAX_GROUPS'] == 4 and skref.BATCH == c['COL_B'], stale
    at3, at2 = c['SKT_GROUP_NODES'] // 4, c['SKT_GROUP_NODES'] // 3                     # 16,384 and 21,845: the last n of 4 and of 3 groups
    assert [sc.sketch_groups(n, 9, c) for n in (at3, at3 + 1, at2, at2 + 1, c['SKT_GROUP_NODES'] // 2, c['SKT_GROUP_NODES'] // 2 + 1)] == [4, 3, 3, 2, 2, 1], stale
    want_n = {'sketch_three_groups': 16_906, 'sketch_two_groups': 22_506, 'diffusion_large': 33_133}
    for groups, (name, (build, k, launches)) in zip((3, 2, 1), sc.SKETCH_LARGE.items()):
        ei, n, names = build()
        assert n == want_n[name] and sc.sketch_groups(n, sc.blocks_of(k, c['COL_B']), c) == groups, stale
        assert sc.sketch_launches(n, k, c) == launches and sum(launches) == sc.blocks_of(k, c['COL_B']), stale
        deg = sc.degrees(ei, n)
        assert (deg > c['SP_LONG_DEG']).sum() == 1 and deg[names['hub0']] == 2100, stale   # exactly one long row
        assert deg[names['isolated']] == 0 and deg[names['last']] == 0
    assert sc.SKETCH_LARGE['diffusion_large'][1] % c['COL_B'] == 4                          # twelve padding columns in the second launch
    for name in ('random300', 'barbell_20_4'):
        n = skref.GENERAL[name]()[1]
        assert n <= 300
        for k, launches in sc.SKETCH_SMALL_COLUMNS.items():
            assert sc.sketch_launches(n, k, c) == launches, stale
        assert [sc.sketch_launches(n, 112, c, env) for env in (1, 2, 3, 4, 5)] == [[1] * 7, [2, 2, 2, 1], [3, 3, 1], [4, 3], [4, 3]], stale
    n = skref.large_case('windmill').n
    assert sc.sketch_launches(n, skref.WINDMILL_COLUMNS, c) == [4, 3], stale
    assert sc.sketch_launches(want_n['sketch_three_groups'], 16, c) == [1]              # the one-group call the k = 80 call is compared with
    assert sc.WHOLE_SMALL > 2 ** 16 and sc.sketch_groups(sc.WHOLE_SMALL, 1, c) == 1      # node ids past 16 bits in the Philox key


def test_sketch_pairs_past_the_cap(c):
    stale = 'stale GPU size: scale_ref.sketch_pairs_past_cap (SKT_PAIR_BLOCKS: second trip of k_sketch_pairs)'
    ei, n, names = sc.sketch_three_groups()
    pairs, marks = sc.sketch_pairs_past_cap(n, names, c, 130)
    per_trip = c['SKT_PAIR_BLOCKS'] * 256 // c['COL_CP']
    assert per_trip == 32_768 and len(pairs) == per_trip + sc.PAIRS_EXTRA == 32_805, stale
    assert sc.sketch_pair_grid(per_trip, c) == (c['SKT_PAIR_BLOCKS'], 1, per_trip), stale
    assert sc.sketch_pair_grid(per_trip + 1, c) == (c['SKT_PAIR_BLOCKS'], 2, 1), stale
    grid, trips, last = sc.sketch_pair_grid(len(pairs), c)
    assert (grid, trips) == (c['SKT_PAIR_BLOCKS'], 2) and 0 < last == sc.PAIRS_EXTRA < per_trip, stale   # ragged and not empty
    assert last * c['COL_CP'] % 256 != 0 and last * c['COL_CP'] > 256, stale            # more than one workgroup, the last partly filled
    assert sc.sketch_pair_grid(15, c) == (1, 1, 15)                                     # what the other tests pass: one workgroup
    assert pairs.min() >= 0 and pairs.max() < n
    deg = sc.degrees(ei, n)
    for key in ('same', 'isolated', 'isolated_last', 'hub'):
        first, second = marks[key]
        assert first < per_trip <= second < len(pairs), (key, stale)
    f0, f1, f2 = marks['fixed']
    assert f0 == 0 < f1 < per_trip <= f2 and all(tuple(pairs[i]) == marks['pair'] for i in marks['fixed'])
    assert deg[marks['pair'][0]] == 2100 and 0 < deg[marks['pair'][1]] <= 5
    assert all(pairs[i, 0] == pairs[i, 1] for i in marks['same'])
    assert all((deg[pairs[i]] == 0).sum() >= 1 for i in marks['isolated'] + marks['isolated_last'])
    assert (deg[pairs[marks['isolated_last'][1]]] == 0).all() and pairs[marks['isolated_last'][1], 0] != pairs[marks['isolated_last'][1], 1]
    assert all(names['hub0'] in pairs[i] and (pairs[i] < 130 * 130).any() for i in marks['hub'])
    across = (deg[pairs] == 0).any(axis=1) & (pairs[:, 0] != pairs[:, 1])
    assert across.sum() == 4 and (pairs[:, 0] == pairs[:, 1]).sum() >= 2
    again, _ = sc.sketch_pairs_past_cap(n, names, c, 130)
    assert np.array_equal(pairs, again)


def test_no_two_slots_of_the_long_row_can_be_exchanged_unseen(c):
    """On each large graph the reference values of the long row's edges differ pairwise by more than 100 times the largest
    acceptance bound among them, the bound taken with the residuals of the float64 CG replica at tol 1e-12 (the device's are the
    same iteration's): a value written to another slot of the row misses its bound by a factor of 99 at least.  On the windmill
    the row holds 100 bridges, all 1, and blades of few kinds; there at least 1,000 values lie more than 100 bounds apart."""
    import resistance_sketch_ref as skref
    for name in sc.SKETCH_LARGE:
        case = skref.large_case(name)
        assert len(case.hub_edges) == 2100 > c['SP_LONG_DEG']
        want = (case.a[:, case.hub_edges] ** 2).mean(axis=0)
        bound = case.bound(case.replica()[1])[case.hub_edges].max() + skref.SCALE_ROUNDING_ALLOW * max(1.0, want.max())
        gap = np.diff(np.sort(want)).min()
        print(f'  {name}, seed {case.seed}: smallest difference of two values of the long row {gap:.3e}, largest bound {bound:.3e}, ratio {gap / bound:.1f}')
        assert gap > 100.0 * bound, f'stale seed: resistance_sketch_ref.LARGE_SEEDS[{name!r}]'
    case = skref.large_case('windmill')
    want = (case.a[:, case.hub_edges] ** 2).mean(axis=0)
    bound = case.bound(case.replica()[1])[case.hub_edges].max()
    distinct = skref.distinct_values(want, 100.0 * bound)
    kept = skref.distinct_values((case.a[:, case.hub_kept] ** 2).mean(axis=0), 100.0 * bound)
    print(f'  windmill: {len(case.hub_edges)} slots in the long row, {distinct} values more than 100 bounds apart, largest bound {bound:.3e}; '
          f'{len(case.hub_kept)} of the slots lead to a larger id and are summed in the row itself, {kept} such values among them')
    assert len(case.hub_edges) > c['SP_LONG_DEG'] and distinct >= 1000
    # On the lattice graphs the hub's id is above all its neighbours': k_sketch_accumulate keeps an edge at its smaller endpoint, so
    # the long row there is walked and writes nothing, and its edges' values come from short rows.  The windmill's first centre has
    # a low id: its row writes most of its own slots, and at least 1,000 different values among those too.
    assert all(len(skref.large_case(name).hub_kept) == 0 for name in sc.SKETCH_LARGE)
    assert len(case.hub_kept) > c['SP_LONG_DEG'] and len(case.hub_edges) - len(case.hub_kept) >= 64 and kept >= 1000
    mid = skref.windmill_centres(case.parts)[1]
    assert c['SP_SHORT_DEG'] < sc.degrees(case.ei, case.n)[mid] <= c['SP_LONG_DEG'] and len(skref.WINDMILL_MID) * 3 >= 33


# ---- hop distances -------------------------------------------------------------------------------------------------------------------
def test_hop_count_second_trip(c):
    stale = ('stale GPU size: scale_ref.HOPS_LARGE (HOP_COUNT_BLOCKS: second trip of the chunk loop of k_hop_count, '
             'tests/test_hops_gpu.py::test_*_at_262182_nodes)')
    ei, n = sc.fosr_large()
    assert n == sc.HOPS_LARGE
    at = 64 * 4 * c['HOP_COUNT_BLOCKS']                                           # 262,144: the largest n of one trip
    assert sc.hop_count_grid(at, c) == (c['HOP_COUNT_BLOCKS'], 1) and sc.hop_count_grid(at + 1, c) == (c['HOP_COUNT_BLOCKS'], 2), stale
    assert sc.blocks_of(n, 64) > 4 * c['HOP_COUNT_BLOCKS'] and sc.hop_count_grid(n, c) == (c['HOP_COUNT_BLOCKS'], 2), stale
    deg = sc.degrees(ei, n)
    second = deg[at:]                                                             # the nodes of the second trip: one wave's chunk
    assert 0 < second.size <= 64 and (second > 0).sum() >= 1 and (second == 0).sum() >= 1, stale
    assert deg[at] > 0 and (deg[at + 1:] == 0).all() and second.size == 38, stale
    src = sc.hop_sources_large()
    assert src.size == 130 and np.unique(src).size == 26, stale
    for word in (src[:64], src[64:128], src[128:]):
        assert at in word, stale                                                  # the connected node of the second trip in every word
    assert n - 1 in src and 0 in src and deg[n - 1] == 0
    # the smaller size: one trip of the count, many workgroups of the level kernel, all three row classes
    stale = 'stale GPU size: scale_ref.HOPS_SMALL (tests/test_hops_gpu.py::test_rows_and_summary_at_70001_nodes)'
    ei, n = sc.whole_small()
    deg = sc.degrees(ei, n)
    grid, trips = sc.hop_count_grid(n, c)
    assert trips == 1 and 1 < grid < c['HOP_COUNT_BLOCKS'] and n % 64 != 0, stale
    src = sc.hop_sources_small()
    assert deg[src[0]] > c['SP_LONG_DEG'] and c['SP_SHORT_DEG'] < deg[src[1]] <= c['SP_LONG_DEG'] and src[2] == 0, stale
    assert deg[src[3]] == 0 and src[4] == n - 1 and deg[src[4]] == 0 and deg[src[5]] > 0 and src[5] == n - 4, stale
