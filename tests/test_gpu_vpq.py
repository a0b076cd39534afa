"""GPU: the device VPQ meter (include/vkn_vpq.h, csrc/vkn_vpq.hip, `VPQMeter`).  Everything is compared at zero tolerance: the integer
tables and the set of TP records with tests/vpq_ref.py (pinned to the reference's own results by tests/test_vpq_refs.py, which also
proves the premises of the seeded inputs used here), `counts()` and `result()` bit for bit with the fixtures tests/golden/vpq_*.npz."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import vpq_ref
from abi_arena import Arena, frozen

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_WORKSPACE, E_ALIGN = -3, -5
K = vpq_ref.KITTI


def _dev(*maps):
    return [torch.from_numpy(np.ascontiguousarray(m)).to(DEV) for m in maps]


def _feed(meter, dm, splits, sequence_id=0):
    at = 0
    for n in splits:
        meter.update_state(*(m[at] if n == 1 else m[at:at + n] for m in dm), sequence_id=sequence_id)      # n == 1: the [H,W] form
        at += n
    assert at == dm[0].shape[0]


@functools.lru_cache(maxsize=None)
def _video(name):
    """(maps, the restatement's tables) of a seeded video, computed once"""
    p = getattr(vpq_ref, name)
    maps = vpq_ref.video_maps(p['seed'], p['F'], p['H'], p['W'], cell=p['cell'])
    ref = vpq_ref.VPQRef(**K)
    ref.update_state(*maps)
    return maps, ref.tables(0)


@pytest.mark.parametrize('name', vpq_ref.CASES)
def test_fixtures_frame_by_frame_and_batched(vkn, name):
    args, ids, maps, z = vpq_ref.load_case(name)
    S, F = maps[0].shape[:2]
    ref = vpq_ref.VPQRef(**args)
    for s, sid in enumerate(ids):
        ref.update_state(*(m[s] for m in maps), sequence_id=sid)
    dm = _dev(*maps)
    for batched in (False, True):
        meter = vkn.VPQMeter(**args, device=DEV)
        for s, sid in enumerate(ids):
            _feed(meter, [m[s] for m in dm], [F] if batched else [1] * F, sid)
        for sid in ids:
            vpq_ref.assert_same_tables(meter.tables(sid), ref.tables(sid), f'{name} batched {batched}')
            assert meter.tables(sid)['frames'] == F and meter.tables(sid)['status'] == 0
        meter.check_status()
        vpq_ref.assert_counts(meter.counts(), z, f'{name} batched {batched}')
        vpq_ref.assert_result(meter.result(), z, f'{name} batched {batched}')


def test_ten_frames_fed_in_every_grouping(vkn):
    """1 + 1 + ..., 3 + 7 and 10 at once, and the splits around the launch group of VKN_VPQ_GROUP frames: a call of 8 frames is one group,
    9 are two; windows of 4 frames reach back over the border of calls and of groups"""
    G = vkn._lib.VPQ['VKN_VPQ_GROUP']
    maps, want = _video('LONG')
    F = maps[0].shape[0]
    assert F == 10 and G == 8 and (maps[0].shape[1] * maps[0].shape[2]) // vkn._lib.VPQ['VKN_VPQ_SPAN_PX'] == 14
    dm = _dev(*maps)
    for splits in ([1] * F, [3, 7], [F], [G, F - G], [G - 1, F - G + 1], [G + 1, F - G - 1]):
        meter = vkn.VPQMeter(**K, device=DEV)
        _feed(meter, dm, splits)
        vpq_ref.assert_same_tables(meter.tables(0), want, f'splits {splits}')
    assert want['status'] == 0 and len(want['log']) > 100


def test_the_ring_wraps_over_many_frames(vkn):
    """25 frames: more than the ring's max(ks) - 1 + VKN_VPQ_GROUP = 11 slots, fed singly, in calls of several groups and in uneven calls"""
    p = dict(vpq_ref.SMALL, F=25)
    maps = vpq_ref.video_maps(p['seed'], p['F'], p['H'], p['W'], cell=p['cell'])
    ref = vpq_ref.VPQRef(**K)
    ref.update_state(*maps)
    dm = _dev(*maps)
    for splits in ([1] * 25, [25], [13, 12], [2, 9, 8, 6]):
        meter = vkn.VPQMeter(**K, device=DEV)
        _feed(meter, dm, splits)
        vpq_ref.assert_same_tables(meter.tables(0), ref.tables(0), f'splits {splits}')


def test_odd_frame_size_and_maps_off_the_16_byte_grid(vkn):
    """H W = 897: frames of one call start at every residue of the 4-pixel load; then each map on its own residue"""
    maps, want = _video('SMALL')
    F, H, W = maps[0].shape
    assert (H * W) % 4 == 1
    meter = vkn.VPQMeter(**K, device=DEV)
    _feed(meter, _dev(*maps), [F])
    vpq_ref.assert_same_tables(meter.tables(0), want, 'odd H W')
    for skews in ((1, 1, 1, 1), (0, 1, 2, 3), (3, 0, 0, 2)):
        views = []
        for m, k in zip(maps, skews):
            buf = torch.zeros((m.size + 4,), dtype=torch.int32, device=DEV)
            v = buf[k:k + m.size].view(F, H, W)
            v.copy_(torch.from_numpy(m))
            assert v.data_ptr() % 16 == 4 * k
            views.append(v)
        meter = vkn.VPQMeter(**K, device=DEV)
        _feed(meter, views, [F])
        vpq_ref.assert_same_tables(meter.tables(0), want, f'skews {skews}')


def test_one_map_alone_off_gt_sems_residue(vkn):
    """gt_ins, pred_sem, pred_ins in turn on a residue of its own: that map is loaded by words, the other three by 16 bytes.  Two frames
    of 897 pixels: the second one starts behind a peel"""
    maps = [np.ascontiguousarray(m[:2]) for m in _video('SMALL')[0]]
    ref = vpq_ref.VPQRef(**K)
    ref.update_state(*maps)
    for skews in ((0, 1, 0, 0), (0, 0, 2, 0), (0, 0, 0, 3)):
        views = []
        for m, k in zip(maps, skews):
            v = torch.zeros((m.size + 4,), dtype=torch.int32, device=DEV)[k:k + m.size].view(m.shape)
            v.copy_(torch.from_numpy(m))
            assert v.data_ptr() % 16 == 4 * k
            views.append(v)
        meter = vkn.VPQMeter(**K, device=DEV)
        _feed(meter, views, [2])
        vpq_ref.assert_same_tables(meter.tables(0), ref.tables(0), f'skews {skews}')


def test_tail_and_peel_arms(vkn):
    span = vkn._lib.VPQ['VKN_VPQ_SPAN_PX']
    for HW in (1, 3, 5, span - 1, span, span + 1):
        maps = [m.reshape(3, 1, HW) for m in vpq_ref.video_maps(100 + HW % 97, 3, 1, HW, cell=3)]
        ref = vpq_ref.VPQRef(**K)
        ref.update_state(*maps)
        meter = vkn.VPQMeter(**K, device=DEV)
        _feed(meter, _dev(*maps), [3])
        vpq_ref.assert_same_tables(meter.tables(0), ref.tables(0), f'HW = {HW}')


def test_more_spans_than_workgroups_of_a_frame(vkn):
    """8 frames of one launch share VKN_VPQ_MAX_GRID workgroups: beyond 64 spans a workgroup walks two, with one table in LDS"""
    C = vkn._lib.VPQ
    H, W = 264, 512
    spans = -(-H * W // C['VKN_VPQ_SPAN_PX'])
    assert C['VKN_VPQ_MAX_GRID'] // C['VKN_VPQ_GROUP'] < spans < 2 * (C['VKN_VPQ_MAX_GRID'] // C['VKN_VPQ_GROUP'])
    cfg = dict(K, ks=(1, 2))
    maps = vpq_ref.video_maps(61, 8, H, W, cell=32)
    ref = vpq_ref.VPQRef(**cfg)
    ref.update_state(*maps)
    meter = vkn.VPQMeter(**cfg, device=DEV)
    _feed(meter, _dev(*maps), [8])
    vpq_ref.assert_same_tables(meter.tables(0), ref.tables(0), 'two spans per workgroup')


@pytest.mark.parametrize('capacity,in_lds', ((dict(gt=1024, pred=512, pair=8192), True), (dict(gt=512, pred=1024, pair=8192), False),
                                             (dict(gt=1024, pred=1024, pair=16384), False)))
def test_window_tables_in_lds_up_to_its_size_and_in_the_scratch_beyond(vkn, capacity, in_lds):
    """a window's tables take 16 bytes per slot and 8 more per pred slot: exactly 156 KiB (the CU's 160 less the kernel's own 4) still live
    in LDS, 160 KiB and more do not"""
    assert (16 * sum(capacity.values()) + 8 * capacity['pred'] <= 156 * 1024) == in_lds
    assert not in_lds or 16 * sum(capacity.values()) + 8 * capacity['pred'] == 156 * 1024
    maps, want = _video('LONG')
    for splits in ([10], [4, 1, 5]):
        meter = vkn.VPQMeter(**K, capacity=capacity, device=DEV)
        _feed(meter, _dev(*maps), splits)
        vpq_ref.assert_same_tables(meter.tables(0), want, f'capacity {capacity} splits {splits}')


def test_lds_overflow_takes_the_global_path(vkn):
    p = vpq_ref.LDS_OVERFLOW
    maps = vpq_ref.noisy_maps(p['seed'], p['F'], p['H'], p['W'], n_ids=p['n_ids'])
    ref = vpq_ref.VPQRef(**K)
    ref.update_state(*maps)
    meter = vkn.VPQMeter(**K, capacity=p['capacity'], device=DEV)
    _feed(meter, _dev(*maps), [1])
    vpq_ref.assert_same_tables(meter.tables(0), ref.tables(0), 'LDS overflow')


def test_two_sequences_interleaved_equal_one_after_the_other(vkn):
    args, ids, maps, z = vpq_ref.load_case('kitti')
    S, F = maps[0].shape[:2]
    assert S == 2
    dm = _dev(*maps)
    inter, serial = vkn.VPQMeter(**args, device=DEV), vkn.VPQMeter(**args, device=DEV)
    for f in range(F):
        for s, sid in enumerate(ids):
            inter.update_state(*(m[s, f] for m in dm), sequence_id=sid)
    for s, sid in enumerate(ids):
        _feed(serial, [m[s] for m in dm], [1] * F, sid)
    for sid in ids:
        vpq_ref.assert_same_tables(inter.tables(sid), serial.tables(sid), f'sequence {sid}')
    for a, b in zip(inter.counts(), serial.counts()):
        assert all(vpq_ref.same_bits(a[m], b[m]) for m in vpq_ref.ROW_KEYS)
    vpq_ref.assert_counts(inter.counts(), z, 'interleaved')
    vpq_ref.assert_result(inter.result(), z, 'interleaved')


@pytest.mark.parametrize('table', ('gt', 'pred', 'pair', 'log'))
def test_full_table_is_flagged_and_result_raises(vkn, table):
    p = vpq_ref.NOISY
    maps = vpq_ref.noisy_maps(p['seed'], p['F'], p['H'], p['W'])
    ref = vpq_ref.VPQRef(**K)
    ref.update_state(*maps)
    meter = vkn.VPQMeter(**K, capacity={table: 16}, device=DEV)
    _feed(meter, _dev(*maps), [p['F']])
    got, want = meter.tables(0), ref.tables(0)
    assert got['status'] == vkn._lib.VPQ['VKN_VPQ_STATUS_FULL_' + table.upper()] and got['frames'] == p['F']
    with pytest.raises(vkn.VknError) as e:
        meter.result()
    assert 'FULL' in str(e.value) and f'capacity["{table}"]' in str(e.value) and str(e.value).count('FULL') == 1
    with pytest.raises(vkn.VknError):
        meter.check_status()
    if table == 'log':
        # nothing else is disturbed: every count is exact, and the 16 slots hold 16 of the true records
        assert np.array_equal(got['acc'], want['acc']) and got['log'].shape == (16, 4)
        assert {tuple(r) for r in got['log'].tolist()} <= {tuple(r) for r in want['log'].tolist()}
    meter.reset_states()
    small, small_want = _video('SMALL')
    roomy = vkn.VPQMeter(**K, device=DEV)
    _feed(roomy, _dev(*small), [small[0].shape[0]])
    vpq_ref.assert_same_tables(roomy.tables(0), small_want, 'default capacities')


@pytest.mark.parametrize('what,bit', (('id_2_16', 'ID_RANGE'), ('id_negative', 'ID_RANGE'), ('pred_class_20', 'CLASS_RANGE'),
                                      ('pred_class_255', 'CLASS_RANGE'), ('gt_class_20', 'CLASS_RANGE')))
def test_range_flags_skip_the_pixel_and_count_the_rest(vkn, what, bit):
    maps = [m[0].copy() for m in vpq_ref.video_maps(31, 1, 24, 39, cell=4)]
    gs, gi, ps, pi = maps
    y, x = np.argwhere((gs == ps) & (gi == pi) & np.isin(gs, K['things_list']))[5]          # a pixel inside a matched pair
    if what == 'id_2_16':
        pi[y, x] = 2 ** 16
    elif what == 'id_negative':
        gi[y, x] = -3
    elif what == 'gt_class_20':
        gs[y, x] = 20
    else:
        ps[y, x] = 20 if what == 'pred_class_20' else 255
    meter = vkn.VPQMeter(**K, device=DEV)
    meter.update_state(*_dev(*maps))
    keep = np.ones(gs.shape, bool)
    keep[y, x] = False
    ref = vpq_ref.VPQRef(**K)
    ref.update_state(*(m[keep][None] for m in maps))                         # the same maps without that pixel
    got, want = meter.tables(0), ref.tables(0)
    assert got['status'] == vkn._lib.VPQ['VKN_VPQ_STATUS_' + bit] and want['status'] == 0
    assert np.array_equal(got['acc'], want['acc']) and np.array_equal(got['log'], want['log']) and got['frames'] == 1
    with pytest.raises(vkn.VknError) as e:
        meter.result()
    assert bit in str(e.value)


def test_buffer_contract(vkn):
    lib = vkn._lib
    L = lib.lib()
    cfg = vkn.ops.vpq_cfg(20, (1, 2, 4), cap_gt=64, cap_pred=64, cap_pair=256, cap_log=1024)
    nbytes, off = vkn.ops.vpq_layout(cfg)
    assert nbytes == L.vkn_vpq_state_bytes(ctypes.byref(cfg)) and nbytes % 16 == 0
    small, want = _video('SMALL')
    B, HW = small[0].shape[0], small[0].shape[1] * small[0].shape[2]
    maps = _dev(*(m.reshape(B, HW) for m in small))
    A = Arena(DEV)
    state = A.out((nbytes,), torch.uint8, name='state', align=16)
    ptrs = [ctypes.c_void_p(m.data_ptr()) for m in maps]
    with torch.cuda.device(DEV):
        assert L.vkn_vpq_reset(ctypes.byref(cfg), state.ptr, nbytes, None) == 0
        A.check('reset')                                                     # all of the state written, nothing else
        assert not state.t.cpu().numpy().any()
        with frozen(*maps):
            assert L.vkn_vpq_update_i32(ctypes.byref(cfg), state.ptr, nbytes, *ptrs, B, HW, None) == 0
        A.check('update')
        before = state.t.clone()
        for d in (-16, 16, 1):
            assert L.vkn_vpq_update_i32(ctypes.byref(cfg), state.ptr, nbytes + d, *ptrs, B, HW, None) == E_WORKSPACE
            assert L.vkn_vpq_reset(ctypes.byref(cfg), state.ptr, nbytes + d, None) == E_WORKSPACE
        assert L.vkn_vpq_update_i32(ctypes.byref(cfg), ctypes.c_void_p(state.addr + 4), nbytes, *ptrs, B, HW, None) == E_ALIGN
        assert L.vkn_vpq_update_i32(ctypes.byref(cfg), state.ptr, nbytes, ctypes.c_void_p(maps[0].data_ptr() + 2), *ptrs[1:], B, HW, None) == E_ALIGN
        assert L.vkn_vpq_reset(ctypes.byref(cfg), ctypes.c_void_p(state.addr + 4), nbytes, None) == E_ALIGN
    A.check('refusals')
    assert torch.equal(state.t, before)
    raw = state.t.cpu().numpy()
    status, frames, used = raw[:12].view(np.uint32).tolist()
    assert (status, frames, used) == (0, B, len(want['log'])) and not raw[12:off[1]].any()
    assert np.array_equal(raw[off[1]:off[1] + 3 * 3 * 20 * 8].view(np.int64).reshape(3, 3, 20), want['acc'])
    log = raw[off[2]:off[2] + 32 * used].view(np.int64).reshape(-1, 4)
    assert np.array_equal(log[np.lexsort((log[:, 1], log[:, 0]))], want['log']) and not raw[off[2] + 32 * used:off[3]].any()
