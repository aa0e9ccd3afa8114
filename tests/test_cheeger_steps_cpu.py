"""tests/cheeger_steps_ref.py pinned without a GPU: its constants against the values the kernels were designed with, its palette
reference and its replica of ``k_cheeger_sliced`` against tests/cheeger_ref.py, its launch geometry against hand-computed
figures, and the replica with four planted faults against the palette reference on the clamp graph: each fault must show.

It also records the finding the GPU file tests/test_cheeger_limits_gpu.py rests on: every call of tests/test_cheeger_gpu.py
launches the sliced kernel with ``rounds == 4``, so no counter there holds more than 28."""
import numpy as np
import pytest

import cheeger_ref
import cheeger_steps_ref as steps
from conftest import load_golden


@pytest.fixture(scope='module')
def small():
    from dcr import synthetic
    ei, n = synthetic.powerlaw_graph(400, 4, seed=3)
    return ei, n, steps.slot_layout(ei, n)


@pytest.fixture(scope='module')
def clamp():
    ei, n = steps.clamp_graph()
    pal, pw = steps.clamp_palette(steps.CLAMP_W)
    return ei, n, steps.slot_layout(ei, n), pal, pw


def test_constants_are_the_ones_the_limits_were_worked_out_for():
    c = steps.CONSTANTS
    assert (c['CH_LOW'], c['CH_HIGH'], c['CH_RUN'], c['CH_MAX_ROUNDS']) == (3, 10, 7, 146)
    assert c['CH_RUN'] == (1 << c['CH_LOW']) - 1                       # a low counter is full after a run
    assert c['CH_MAX_ROUNDS'] * c['CH_RUN'] == 1022 <= (1 << c['CH_HIGH']) - 1 < (c['CH_MAX_ROUNDS'] + 1) * c['CH_RUN']
    assert c['CHEEGER_MAX_WORDS'] == 65535
    assert c['WL_LADDER'] == (('>=', 16, 16), ('>', 4, 8), ('>', 2, 4), ('==', 2, 2), (None, 0, 1))
    assert (c['WG_PER_CU'], c['CU_DEFAULT'], c['MIN_ROUNDS']) == (4, 256, 4)
    assert (c['LANE_DIV'], c['LANE_ROUND'], c['LANE_MIN']) == (8, 16, 512)
    assert [steps.word_lanes(W) for W in (1, 2, 3, 4, 5, 8, 15, 16, 17, 65535)] == [1, 2, 4, 4, 8, 8, 8, 16, 16, 16]
    assert steps.slack_for(np.array([0, 31, 32, 36, 16640])).tolist() == [8, 8, 8, 9, 4160]


def test_slot_layout_of_hand_graphs():
    """Rows in insertion order: the kept pairs are (src, dst) with dst < src, in the order given."""
    ei = np.array([[0, 0, 1, 1, 2, 2, 3, 3], [1, 2, 0, 3, 0, 3, 1, 2]])          # coalesced: 0-1, 0-2, 1-3, 2-3
    lay = steps.slot_layout(ei, 5)
    assert lay.cap_total == 5 * 8 + 8 and lay.rowinfo.tolist() == [[0, 2], [10, 2], [20, 2], [30, 2], [40, 0]]
    assert [lay.col[s:s + 3].tolist() for s in (0, 10, 20, 30, 40)] == [[1, 2, -1], [0, 3, -1], [0, 3, -1], [1, 2, -1], [-1] * 3]
    assert lay.slot_row.tolist() == sum(([u] * (10 if u < 4 else 8) for u in range(5)), [])
    un = np.array([[3, 1, 3, 2, 1, 3], [2, 0, 1, 0, 0, 2]])                      # unsorted, with duplicates: 3-2, 1-0, 3-1, 2-0
    lay = steps.slot_layout(un, 4)
    assert [lay.col[s:s + 2].tolist() for s in lay.rowinfo[:, 0]] == [[1, 2], [0, 3], [3, 0], [2, 1]]


def test_palette_counts_equal_the_plain_reference(small):
    ei, n, _ = small
    rng = np.random.Generator(np.random.PCG64(7))
    pw = rng.integers(0, 2 ** 64, size=(5, 3), dtype=np.uint64)
    pw[0], pw[1] = np.uint64(0xFFFFFFFFFFFFFFFF), 0
    pal = rng.integers(0, 5, size=n)
    words = steps.palette_members(pal, pw)
    want = cheeger_ref.counts(ei, cheeger_ref.unpack(words, 192))
    assert np.array_equal(steps.palette_counts(ei, n, pal, pw), want)
    assert np.array_equal(steps.palette_counts(ei, n, pal, pw, block_words=2), want)
    assert want[:, :3].max() > 100


@pytest.mark.parametrize('W', [1, 2, 3, 5, 8, 17])
def test_replica_over_all_workgroups_equals_the_plain_reference(small, W):
    ei, n, lay = small
    B = 64 * W - 5
    rng = np.random.Generator(np.random.PCG64(W))
    members = rng.random((B, n)) < rng.random((B, 1))
    members[0], members[1] = True, False
    bits = np.zeros((n, 64 * W), dtype=np.uint8)
    bits[:, :B] = members.T
    words = np.packbits(bits, axis=1, bitorder='little').view('<u8').reshape(n, W)
    assert np.array_equal(cheeger_ref.unpack(words, B), members)
    geom = steps.geometry(lay.cap_total, W, 0)
    got = steps.sliced_replica(lay, words, W, geom)
    assert got.shape == (64 * W, 3) and not got[B:].any()
    assert np.array_equal(got[:B], cheeger_ref.counts(ei, members)[:, :3])
    # a smaller chunk (more workgroups along the slots) changes nothing
    WL, groups, rounds, chunk, grid_x = geom.sliced
    more = (WL, groups, 1, chunk // rounds, -(-lay.cap_total // (chunk // rounds)))
    assert more[4] > grid_x and np.array_equal(steps.sliced_replica(lay, words, W, more), got)


def _cap_total(ei, n):
    return steps.slot_layout(ei, n).cap_total


def test_every_call_of_the_first_gpu_file_runs_four_rounds():
    """The graph / W pairs of tests/test_cheeger_gpu.py, test by test, at the 256 CUs of the MI355X (also the launcher's
    figure before a handle has asked the device).  Edited graphs: their rows are laid out again with twice the slack at most,
    so three times the created graph's slots bound them from above."""
    from dcr import synthetic
    fx = load_golden('cheeger_reference.json')
    caps = {}
    for case in fx['estimate']:
        ei = (synthetic.powerlaw_graph(*case['generator']['powerlaw_graph'])[0] if case['generator'] is not None
              else np.asarray(case['edge_index'], dtype=np.int64).reshape(2, -1))
        caps[case['name']] = _cap_total(ei, case['num_nodes'])
    pairs = []
    # test_hand_graphs_and_explicit_subsets_of_the_fixture
    pairs += [(rec['name'], caps[rec['name']], (len(rec['subsets']) + 63) // 64) for rec in fx['cheeger_S']]
    # test_estimate_cheeger_equals_the_reference: batches of 7, 64, all iterations, 5000
    pairs += [(c['name'], caps[c['name']], W) for c in fx['estimate'] for W in (1, (c['iterations'] + 63) // 64)]
    g400, g20k, g2485 = caps['powerlaw400m4'], _cap_total(*synthetic.powerlaw_graph(20000, 2, seed=4)), caps['powerlaw2485m2']
    # test_counts_on_powerlaw_graphs, test_packed_words_are_accepted_as_they_are, test_conductance_is_networkx_conductance,
    # test_estimate_cheeger_takes_a_live_graph_and_zero_iterations
    pairs += [('powerlaw400m4', g400, W) for W in (1, 2, 3)] + [('powerlaw20000m2', g20k, W) for W in (16, 3)] + [('powerlaw2485m2', g2485, 8)]
    # test_philox_subsets_are_the_documented_family, test_philox_estimate_does_not_depend_on_the_batch (batches of 64, 4096, 100)
    pairs += [('powerlaw2485m2', g2485, W) for W in (1, 4, 16, 64, 2, 15, 5)]
    # test_counts_follow_edits_and_sdrf_iterations (edited: three times the slots), test_cheeger_calls_leave_the_curvature_buffer_alone
    pairs += [('powerlaw400m4 edited', 3 * g400, 2), ('powerlaw20000m2', g20k, 1), ('powerlaw20000m2', g20k, 2)]
    # test_planted_hub_and_isolated_nodes
    ei, n0 = synthetic.powerlaw_graph(8000, 3, seed=9)
    others = np.setdiff1d(np.arange(n0), [4321])[:6000]
    ei = synthetic.coalesced_edge_index(np.concatenate([ei[0], np.full(6000, 4321)]), np.concatenate([ei[1], others]), n0 + 300)
    pairs += [('planted hub', _cap_total(ei, n0 + 300), 4)]
    # test_sdrf_replay_with_cheeger_calls_in_between: estimates of 70 and 10 draws on graphs that are being edited
    for case in load_golden('sdrf_traces_small.json')['cases']:
        if not case['error']:
            pairs += [(case['graph'] + ' edited', 3 * _cap_total(np.asarray(case['edge_index']), case['num_nodes']), W) for W in (1, 2)]
    # test_counts_at_s100k: powerlaw_graph(100000, 10): E = 10 * (100000 - 10); the slots are at most 2 E + n * 8 + 2 E / 4 + n
    s100k_bound = 2 * 999900 + 100000 * 8 + 2 * 999900 // 4 + 100000
    pairs += [('S100k (upper bound of its slots)', s100k_bound, 2)]
    assert len(pairs) > 60
    seen = {}
    for name, cap, W in pairs:
        WL, groups, rounds, chunk, grid_x = steps.geometry(cap, W, 256).sliced
        assert rounds == 4, (name, cap, W, rounds)
        seen[name, W] = cap
    print(sorted(seen.items()))
    # the largest of them is one round below the next step: 3 + 1
    assert (s100k_bound * 1) // (128 * 7 * 4 * 256) + 1 == 4
    # and a counter of four runs holds 28 at most: planes 5..9 of the high counter stay empty
    assert 4 * steps.CH_RUN < 1 << 5


def test_geometry_of_the_clamp_graph(clamp):
    ei, n, lay, pal, pw = clamp
    assert ei.shape == (2, 2 * 532480) and n == 16672 and lay.cap_total == 1331200
    assert lay.rowinfo[:32].tolist() == [[20800 * h, 16640] for h in range(32)]
    assert np.array_equal(lay.col[:16640], np.arange(32, 16672)) and (lay.col[16640:20800] == -1).all()
    assert lay.rowinfo[32].tolist() == [32 * 20800, 32] and lay.col[32 * 20800:32 * 20800 + 40].tolist() == list(range(32)) + [-1] * 8
    geom = steps.geometry(lay.cap_total, 200, 256)
    assert geom.sliced == (16, 13, 146, 16352, 82) and geom == steps.geometry(lay.cap_total, 200, 0)
    assert geom.lane == (130016, 11)                                   # 1,331,200 * 200 / 2,048 + 1 = 130,001, up to a multiple of 16
    assert 13 * 16 - 200 == 8                                          # the last word group has 8 active words of 16
    assert steps.geometry(lay.cap_total, 200, 256, max_rounds=147).sliced == (16, 13, 147, 16464, 81)
    assert 16464 <= 16640                                              # still inside hub 0's live row: 1,029 adds in every lane
    # chunk boundaries inside live hub rows
    bounds = np.arange(1, 82) * 16352
    assert (lay.col[bounds[bounds < 32 * 20800]] >= 32).sum() >= 20
    # the other instantiations on this graph: W = 15, 4, 2, 1
    assert [steps.geometry(lay.cap_total, W, 256).sliced[:3] for W in (15, 4, 2, 1)] == [(8, 2, 12), (4, 1, 4), (2, 1, 4), (1, 1, 4)]
    # WL < 16 meets the clamp only where cap_total * groups >= 145 * per_round * 1024: W = 15 (two groups of 8 lanes, 224 slots a
    # round) from 16.6 M slots, W = 4 from 66 M, W = 1 from 266 M
    for W, slots in ((15, 16629760), (8, 33259520), (4, 66519040), (2, 133038080), (1, 266076160)):
        assert steps.geometry(slots, W, 256).sliced[2] == 146 and steps.geometry(slots - 1, W, 256).sliced[2] == 145


def test_workgroup_zero_of_the_clamp_graph_saturates_every_category(clamp):
    """Stream st of workgroup 0 takes slots st, st + 16, ...: 1,022 of hub 0's leaves.  From the palette alone: ``in`` and ``hi``
    reach 1,022 in stream 0, ``lo`` in stream 1, and the random rows spread the other lanes over the range below."""
    ei, n, lay, pal, pw = clamp
    assert pal[0] == 2
    for stream, want in ((0, (1022, 0, 1022)), (1, (0, 1022, 0)), (2, (0, 1022, 1022)), (3, (1022, 0, 0))):
        leaves = 32 + np.arange(stream, 16352, 16)
        assert leaves.shape == (1022,)
        sub = np.stack([np.zeros(1022, dtype=np.int64), leaves])
        cnt = steps.palette_counts(sub, n, pal, pw[:, :2])
        assert tuple(cnt[:, :3].max(axis=0)) == want, stream
    sub = np.stack([np.zeros(1022, dtype=np.int64), 32 + np.arange(7, 16352, 16)])
    cnt = steps.palette_counts(sub, n, pal, pw[:, :2])
    assert len(np.unique(cnt[:, 0])) > 8 and 32 < cnt[:, 0].max() < 1022


FAULTS = [dict(planes_high=9), dict(max_rounds=147), dict(drop_carry=True), dict(planes_read=5)]


def test_replica_of_workgroup_zero_equals_the_palette_reference_and_every_planted_fault_shows(clamp):
    ei, n, lay, pal, pw = clamp
    W = steps.CLAMP_W
    words = steps.palette_members(pal, pw)
    assert words.shape == (n, W)
    geom = steps.geometry(lay.cap_total, W, 256)

    def reference(chunk):            # workgroup (0, 0): the first ``chunk`` slots, all of them live slots of hub 0, words 0..15
        assert chunk <= 16640
        sub = np.stack([np.zeros(chunk, dtype=np.int64), 32 + np.arange(chunk, dtype=np.int64)])
        return steps.palette_counts(sub, n, pal, pw[:, :16])[:, :3]

    good = steps.sliced_replica(lay, words, W, geom, workgroups=[(0, 0)])
    want = reference(geom.sliced[3])
    assert not good[1024:].any() and np.array_equal(good[:1024], want)
    assert want.max() > 8 * 1022                                       # a subset's total is the sum of its 16 streams' lanes
    for fault in FAULTS:
        bad = steps.sliced_replica(lay, words, W, geom, workgroups=[(0, 0)], **fault)
        want = reference(steps.geometry(lay.cap_total, W, 256, max_rounds=fault.get('max_rounds')).sliced[3])
        wrong = np.flatnonzero((bad[:1024] != want).any(axis=1))
        print(fault, len(wrong), 'subsets differ; first', wrong[:1], bad[wrong[:1]], want[wrong[:1]])
        assert len(wrong) > 0, fault


def test_replica_of_the_last_word_group_and_a_chunk_across_rows(clamp):
    """Word group 12 has 8 active words of 16; workgroup 40 starts inside hub 31's row and runs across its slack into the
    leaves' rows (a lane there meets live slots, free slots and slots with col < row)."""
    ei, n, lay, pal, pw = clamp
    W = steps.CLAMP_W
    words = steps.palette_members(pal, pw)
    geom = steps.geometry(lay.cap_total, W, 256)
    chunk = geom.sliced[3]
    bx = (32 * 20800 - 5000) // chunk
    assert bx * chunk < 31 * 20800 + 16640 and (bx + 1) * chunk > 32 * 20800
    got = steps.sliced_replica(lay, words, W, geom, workgroups=[(bx, 12)])
    s = np.arange(bx * chunk, (bx + 1) * chunk)
    live = (s - lay.rowinfo[lay.slot_row[s], 0] < lay.rowinfo[lay.slot_row[s], 1]) & (lay.col[s] > lay.slot_row[s])
    sub = np.stack([lay.slot_row[s][live].astype(np.int64), lay.col[s][live].astype(np.int64)])
    assert 0 < live.sum() < chunk and (sub[0] == 31).all()
    want = steps.palette_counts(sub, n, pal, pw[:, 192:200])[:, :3]
    assert not got[:64 * 192].any() and np.array_equal(got[64 * 192:], want)
