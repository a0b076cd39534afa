"""CPU: the NumPy restatement tests/stq_ref.py against every fixture tests/golden/stq_*.npz (written by tools/gen_golden_stq.py from the
reference's own `STQuality`, fed as its evaluation scripts feed it) — integers at zero tolerance, floats within the re-ordering bound
of their sums — and the premises of the inputs that tests/test_gpu_stq.py builds with it."""
import numpy as np
import pytest

import stq_ref


def _run(name, mode, batched=False):
    args, ids, maps, z = stq_ref.load_case(name)
    ref = stq_ref.STQRef(**args, drop_ignored_gt=bool(mode))
    for s, sid in enumerate(ids):
        if batched:
            ref.update_state(*(m[s] for m in maps), sequence_id=sid)
        else:
            for f in range(maps[0].shape[1]):
                ref.update_state(*(m[s, f] for m in maps), sequence_id=sid)
    return ref, ids, z


@pytest.mark.parametrize('mode', (1, 0))
@pytest.mark.parametrize('name', stq_ref.CASES)
def test_restatement_equals_the_reference_fixture(name, mode):
    for batched in (False, True):
        ref, ids, z = _run(name, mode, batched)
        for s, sid in enumerate(ids):
            t = ref.tables(sid)
            stq_ref.assert_tables(t, z, mode, s, f'{name} mode {mode}')
            assert t['status'] == 0 and t['frames'] == z[f'm{mode}_Length_per_seq'][s]
        with np.errstate(all='ignore'):
            stq_ref.assert_result(ref.result(), z, mode, [ref.pairs(sid) for sid in ids], f'{name} mode {mode}')


def test_fixtures_pin_what_they_are_for():
    args, ids, maps, z = stq_ref.load_case('kitti')
    assert maps[0].shape == (2, 3, 24, 39) and len(ids) == 2
    gs, gi, ps, pi = maps
    things = args['things_list']
    assert (gs == 255).any() and (ps == 255).any() and (np.isin(gs, things) & (gi == 0)).any()              # ignore in gt AND pred; crowd
    assert (np.isin(ps, things) & ~np.isin(gs, things) & (gs != 255)).any()                                 # pred things over gt stuff
    assert any(not np.array_equal(z[f'm0_s0_{k}'], z[f'm1_s0_{k}']) for k in ('confusion', 'pred_counts'))  # the two modes differ
    assert all(z[f'm{m}_s{s}_pair_keys'].size <= 16 for m in (0, 1) for s in (0, 1))        # a cap_pair = 16 meter holds a kitti sequence
    assert z['m1_s0_confusion'].shape == (20, 20) and z['m1_s0_confusion'][:, 19].sum() > 0                 # pred ignore -> column 19
    args, _, maps, z = stq_ref.load_case('city')
    assert 0 in args['things_list'] and (maps[0] == 0).any() and (z['m1_s0_gt_keys'] >> 16 == 0).any()
    args, _, maps, z = stq_ref.load_case('vipseg')
    assert z['m1_s0_confusion'].shape == (125, 125) and z['m0_s0_confusion'][124].sum() > 0                 # 200 -> row 124, unmasked
    args, _, maps, z = stq_ref.load_case('ign_in')
    assert z['m0_s0_confusion'].shape == (5, 5) and z['m0_s0_confusion'][2].sum() > 0 and z['m1_s0_confusion'][2].sum() == 0
    args, _, maps, z = stq_ref.load_case('ign_eq')
    assert z['m0_s0_confusion'].shape == (7, 7) and z['m0_s0_confusion'][6].sum() > 0 and z['m1_s0_confusion'][:, 6].sum() > 0


def test_offset_below_the_reference_bound_is_refused():
    with pytest.raises(ValueError):
        stq_ref.STQRef(19, [11], 255, 16, (19 << 16) - 1)


def test_premises_of_the_gpu_inputs(vkn):
    span, slots = vkn._lib.STQ['VKN_STQ_SPAN_PX'], vkn._lib.STQ['VKN_STQ_LDS_SLOTS']
    K = stq_ref.KITTI
    # LDS overflow: more distinct keys (of all four kinds) inside at least one span than the workgroup's table holds
    p = stq_ref.LDS_OVERFLOW
    gs, gi, ps, pi = (m.ravel().astype(np.int64) for m in stq_ref.noisy_maps(p['seed'], p['H'], p['W']))
    assert gs.size > span
    yt, yp = (gs << 16) + gi, (ps << 16) + pi
    most = max(sum(np.unique(k[a:a + span]).size for k in (gs * 20 + ps, yt, yp, yt * K['offset'] + yp)) for a in range(0, gs.size, span))
    assert most > slots, (most, slots)
    # capacity: more distinct pair keys than cap_pair = 16
    p = stq_ref.CAPACITY
    ref = stq_ref.STQRef(**K)
    ref.update_state(*stq_ref.noisy_maps(p['seed'], p['H'], p['W']))
    assert ref.pairs() > 16 and len(ref.seqs[0]['gt']) <= 2048 and len(ref.seqs[0]['pred']) <= 8192
    # contention: one pair covers more than half of the pixels, across many workgroups
    p = stq_ref.CONTENTION
    ref = stq_ref.STQRef(**K)
    ref.update_state(*stq_ref.dominant_maps(p['seed'], p['H'], p['W']))
    assert max(ref.seqs[0]['pair'].values()) * 2 > p['H'] * p['W'] and p['H'] * p['W'] > 16 * span and (p['H'] * p['W']) % 4 == 2      # 465 750 pixels: no multiple of the 4-pixel load
