"""CPU: tests/vpq_ref.py against the reference's own results in tests/golden/vpq_*.npz at zero tolerance (tp, fn, fp as integers, iou bit
for bit), and the premises that tests/test_gpu_vpq.py rests on: the edge events that vpq_edges holds, the integer form of the
scripts' float predicates, and the sizes of the seeded inputs."""
import numpy as np
import pytest

import vpq_ref


def _run(name, batched=False):
    args, ids, maps, z = vpq_ref.load_case(name)
    ref = vpq_ref.VPQRef(**args)
    S, F = maps[0].shape[:2]
    for s, sid in enumerate(ids):
        if batched:
            ref.update_state(*(m[s] for m in maps), sequence_id=sid)
        else:
            for f in range(F):
                ref.update_state(*(m[s, f] for m in maps), sequence_id=sid)
    return args, ids, maps, z, ref


@pytest.mark.parametrize('name', vpq_ref.CASES)
def test_restatement_equals_the_reference(name):
    args, ids, maps, z, ref = _run(name)
    F, nc = maps[0].shape[1], args['num_classes'] + 1
    for i, k in enumerate(args['ks']):
        for s, sid in enumerate(ids):
            rows = ref.rows(sid, i)
            assert rows[0].shape == (max(F - k + 1, 0), nc)
            for m, got in zip(vpq_ref.ROW_KEYS, rows):
                want = z[f'k{i}_s{s}_{m}']
                assert want.dtype == np.float64 and vpq_ref.same_bits(got, want), f'{name}: {m} rows of k = {k}, sequence {s}'
            # the integer tables are those rows summed, and the log holds one record per true positive
            t = ref.tables(sid)
            for r in range(3):
                assert np.array_equal(t['acc'][i, r], z[f'k{i}_s{s}_{vpq_ref.ROW_KEYS[r + 1]}'].sum(axis=0).astype(np.int64))
            assert (t['log'][:, 0] >> 48 == i).sum() == t['acc'][i, 0].sum()
            assert t['status'] == 0 and t['frames'] == F
    vpq_ref.assert_counts(ref.counts(), z, name)
    vpq_ref.assert_result(ref.result(), z, name)
    _, _, _, _, batched = _run(name, batched=True)
    for sid in ids:
        vpq_ref.assert_same_tables(batched.tables(sid), ref.tables(sid), f'{name} batched')
    assert sum(len(ref.tables(sid)['log']) for sid in ids) > 0


def test_vipseg_ground_truth_is_the_raw_map_through_vip2hb():
    """the fixture's gt came from raw_pan through the reference's own vip2hb: stuff id + 1 -> class, thing (id + 1) * 100 + n -> instance n + 1,
    0 and 200 -> 255 (eval_dvpq_vipseg.py:275-293)"""
    _, _, maps, z = vpq_ref.load_case('vipseg')
    raw, gs, gi = z['raw_pan'], maps[0], maps[1]
    assert raw.shape == gs.shape and set(np.unique(raw)) >= {0, 200, 1, 300}
    assert ((gs == 255) == ((raw == 0) | (raw == 200))).all() and (gi[gs == 255] == 0).all()
    assert (gs[raw == 1] == 0).all() and (gi[raw == 1] == 0).all()
    assert (gs[raw == 301] == 66).all() and (gi[raw == 301] == 2).all() and (gs[raw > 128][raw[raw > 128] != 200] >= 66).all()


def test_every_edge_event_occurs_in_vpq_edges():
    args, ids, maps, z, ref = _run('edges')
    trace = ref.seqs[0]['trace']
    pairs = [e for w in trace for e in w['events'] if e[0] == 'pair']            # ('pair', class, int, union, void, hit)
    preds = [e for w in trace for e in w['events'] if e[0] == 'pred']            # ('pred', class, ignored, area, skipped)
    assert any(2 * ia == un and not hit for _, _, ia, un, _, hit in pairs)                           # IoU exactly 1/2: no TP
    assert any(2 * ia == un + 1 and hit for _, _, ia, un, _, hit in pairs)                           # one pixel above
    assert any(hit and void > 0 and 2 * ia <= un + void for _, _, ia, un, void, hit in pairs)         # a TP only through the void overlap
    assert any(2 * ig == area and not skip for _, _, ig, area, skip in preds)                        # half ignored: counted as fp
    assert any(2 * (ig - 1) == area and skip for _, _, ig, area, skip in preds)                      # one pixel more than half: skipped
    assert any(g & 0xFFFF for w in trace for g in w['ign_ids'])                                       # an ignored gt id with an instance part
    # ... which the void overlap does not see and the ignored overlap does: without it the skipped prediction would count
    assert (maps[0] == 255).any() and (maps[1][maps[0] == 255] > 0).any()
    assert z['k0_fp'][19] > 0 and (maps[2] == 19).any()                                               # the class-19 bin
    F = maps[0].shape[1]
    assert F < max(args['ks']) and z[f'k{len(args["ks"]) - 1}_s0_tp'].shape == (0, 20) and not ref.tables(0)['acc'][-1].any()
    assert F >= args['ks'][1] and len(ref.seqs[0]['rows'][1]) == F - args['ks'][1] + 1


def test_the_integer_predicates_are_the_float_predicates():
    """`int / union > 0.5` (eval_dvpq_step.py:74-75) and `ignored / area > 0.5` (:92) in float64 against 2 * a > b in integers, where it is
    closest: unions up to 2^40 and numerators within a few units of half"""
    rng = np.random.default_rng(7)
    union = np.concatenate([rng.integers(1, 1 << 40, 100000), rng.integers(1, 64, 50000), (1 << rng.integers(1, 41, 50000)) - rng.integers(0, 2, 50000)])
    inter = np.clip(union // 2 + rng.integers(-2, 3, union.size), 0, union)
    with np.errstate(all='raise'):
        flt = inter / union > 0.5
    assert flt.dtype == bool and np.array_equal(flt, 2 * inter > union)
    assert (2 * inter == union).sum() > 1000 and (2 * inter == union + 1).sum() > 1000 and (2 * inter == union - 1).sum() > 1000


@pytest.mark.parametrize('p', (vpq_ref.LONG, vpq_ref.SMALL), ids=('long', 'small'))
def test_seeded_videos_fit_the_default_capacities_and_exercise_the_matching(p):
    maps = vpq_ref.video_maps(p['seed'], p['F'], p['H'], p['W'], cell=p['cell'])
    ref = vpq_ref.VPQRef(**vpq_ref.KITTI)
    ref.update_state(*maps)
    t = ref.tables(0)
    assert t['status'] == 0 and t['frames'] == p['F']
    for name in ('gt', 'pred', 'pair'):
        assert 16 < ref.largest[name] <= vpq_ref.DEFAULT_CAPACITY[name] // 2, (name, ref.largest)
    assert len(t['log']) <= vpq_ref.DEFAULT_CAPACITY['log']
    for i in range(3):
        assert t['acc'][i, 0].sum() > 0 and t['acc'][i, 1].sum() > 0 and t['acc'][i, 2].sum() > 0
    assert (maps[0] == 255).any() and (maps[1][maps[0] == 255] > 0).any() and (maps[2] == 19).any()


def test_noisy_maps_overflow_sixteen_slots_of_every_table():
    p = vpq_ref.NOISY
    maps = vpq_ref.noisy_maps(p['seed'], p['F'], p['H'], p['W'])
    ref = vpq_ref.VPQRef(**vpq_ref.KITTI)
    ref.update_state(*maps)
    assert all(16 < ref.largest[n] <= vpq_ref.DEFAULT_CAPACITY[n] for n in ('gt', 'pred', 'pair')) and len(ref.tables(0)['log']) > 16


def test_lds_overflow_input_has_more_keys_in_a_span_than_the_workgroup_table_has_slots():
    p = vpq_ref.LDS_OVERFLOW
    gs, gi, ps, pi = (m.astype(np.int64).ravel()[:2048] for m in vpq_ref.noisy_maps(p['seed'], p['F'], p['H'], p['W'], n_ids=p['n_ids']))
    yt, yp = (gs << 16) + gi, (ps << 16) + pi
    assert len(np.unique(yt)) + len(np.unique(yp)) + len(np.unique(yt * 2 ** 30 + yp)) > 2048                  # VKN_VPQ_SPAN_PX, VKN_VPQ_LDS_SLOTS
    ref = vpq_ref.VPQRef(**vpq_ref.KITTI)
    ref.update_state(*vpq_ref.noisy_maps(p['seed'], p['F'], p['H'], p['W'], n_ids=p['n_ids']))
    assert all(ref.largest[n] <= p['capacity'][n] for n in ('gt', 'pred', 'pair')) and ref.tables(0)['acc'][:, 0].sum() > 0


def test_range_flags_of_the_restatement():
    base = [m[0] for m in vpq_ref.video_maps(5, 1, 8, 8, cell=2)]               # gt_sem, gt_ins, pred_sem, pred_ins
    for edits, bit in ((((3, 1 << 16),), vpq_ref.ID_RANGE), (((1, -1),), vpq_ref.ID_RANGE), (((2, 20),), vpq_ref.CLASS_RANGE),
                       (((0, 20),), vpq_ref.CLASS_RANGE), (((2, 255),), vpq_ref.CLASS_RANGE), (((0, 255), (1, 0)), 0)):
        maps = [m.copy() for m in base]
        for which, value in edits:
            maps[which][3, 3] = value
        ref = vpq_ref.VPQRef(**vpq_ref.KITTI)
        ref.update_state(*maps)
        assert ref.tables(0)['status'] == bit, edits
