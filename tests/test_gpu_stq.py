"""GPU: the device STQ meter (include/vkn_stq.h, csrc/vkn_stq.hip, `STQMeter`).  Every table is compared at zero tolerance: with the
reference's own tables in the fixtures tests/golden/stq_*.npz, and with tests/stq_ref.py (pinned to those fixtures by
tests/test_stq_refs.py, which also proves the premises of the seeded inputs used here)."""
import ctypes

import numpy as np
import pytest
import torch

import stq_ref
from abi_arena import Arena, frozen

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_WORKSPACE, E_ALIGN = -3, -5
K = stq_ref.KITTI


def _dev(*maps):
    return [torch.from_numpy(np.ascontiguousarray(m)).to(DEV) for m in maps]


def _same_tables(got, want, what):
    for k in stq_ref.TABLE_KEYS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f'{what}: {k} differs'


def _against_ref(vkn, maps, what, cfg=K, drop=True, capacity=None):
    meter = vkn.STQMeter(**cfg, drop_ignored_gt=drop, capacity=capacity, device=DEV)
    meter.update_state(*_dev(*maps))
    ref = stq_ref.STQRef(**cfg, drop_ignored_gt=drop)
    ref.update_state(*maps)
    got, want = meter.tables(0), ref.tables(0)
    _same_tables(got, want, what)
    assert got['frames'] == want['frames'] and got['status'] == want['status'] == 0, what
    return meter, ref


@pytest.mark.parametrize('mode', (1, 0))
@pytest.mark.parametrize('name', stq_ref.CASES)
def test_fixtures_frame_by_frame_and_batched(vkn, name, mode):
    args, ids, maps, z = stq_ref.load_case(name)
    S, F = maps[0].shape[:2]
    assert F >= 2
    for batched in (False, True):                       # B >= 2 with an odd H W: frame bases that no 16-byte load can start at
        meter = vkn.STQMeter(**args, drop_ignored_gt=bool(mode), device=DEV)
        dm = _dev(*maps)
        for s, sid in enumerate(ids):
            if batched:
                meter.update_state(*(m[s] for m in dm), sequence_id=sid)
            else:
                for f in range(F):
                    meter.update_state(*(m[s, f] for m in dm), sequence_id=sid)
        terms = []
        for s, sid in enumerate(ids):
            t = meter.tables(sid)
            stq_ref.assert_tables(t, z, mode, s, f'{name} mode {mode} batched {batched}')
            assert t['frames'] == F and t['status'] == 0
            terms.append(t['pair_keys'].size)
        meter.check_status()
        stq_ref.assert_result(meter.result(), z, mode, terms, f'{name} mode {mode} batched {batched}')


def test_tail_and_peel_arms(vkn):
    span = vkn._lib.STQ['VKN_STQ_SPAN_PX']
    for HW in (1, 3, 4, 5, span - 1, span, span + 1):
        maps = [m.reshape(1, HW) for m in stq_ref.seeded_maps(100 + HW % 97, 1, HW, cell=3)]
        _against_ref(vkn, maps, f'HW = {HW}')
        # the same pixels as three frames of one call: frame bases at every residue of the 4-pixel load
        if HW >= 5:
            three = [np.stack([m, m[:, ::-1], m]).copy() for m in maps]
            _against_ref(vkn, three, f'3 x HW = {HW}')


def test_more_spans_than_workgroups(vkn):
    """beyond VKN_STQ_MAX_GRID spans a workgroup walks several, across frame borders, with one table in LDS"""
    span, grid = vkn._lib.STQ['VKN_STQ_SPAN_PX'], vkn._lib.STQ['VKN_STQ_MAX_GRID']
    HW = 2 * span + 1                                   # three spans per frame, the last of one pixel
    B = (3 * grid // 2) // 3 + 1                        # a little over 1.5 x MAX_GRID spans: two per workgroup, an odd number of them
    assert 2 * grid > 3 * B > grid and (3 * B) % 2 == 1
    maps = [m.reshape(B, 1, HW) for m in stq_ref.seeded_maps(77, B, HW, cell=16)]
    _against_ref(vkn, maps, 'several spans per workgroup')


def test_maps_that_start_off_the_16_byte_grid(vkn):
    """each of the four maps on its own residue: the peel follows gt_sem, the other maps are loaded by words where they must"""
    HW = 1000
    maps = stq_ref.seeded_maps(7, 8, 125, cell=4)
    for skews in ((1, 1, 1, 1), (0, 1, 2, 3), (3, 0, 0, 2)):
        bufs = [torch.zeros((HW + 4,), dtype=torch.int32, device=DEV) for _ in range(4)]
        views = []
        for buf, m, k in zip(bufs, maps, skews):
            v = buf[k:k + HW].view(8, 125)
            v.copy_(torch.from_numpy(m))
            assert v.data_ptr() % 16 == 4 * k
            views.append(v)
        meter = vkn.STQMeter(**K, device=DEV)
        meter.update_state(*views)
        ref = stq_ref.STQRef(**K)
        ref.update_state(*maps)
        _same_tables(meter.tables(0), ref.tables(0), f'skews {skews}')


def test_one_map_alone_off_gt_sems_residue(vkn):
    """gt_ins, pred_sem, pred_ins in turn on a residue of its own: that map is loaded by words, the other three by 16 bytes.  Two frames
    of 375 pixels: the second one starts behind a peel"""
    maps = [m.reshape(2, 3, 125) for m in stq_ref.seeded_maps(9, 6, 125, cell=4)]
    ref = stq_ref.STQRef(**K)
    ref.update_state(*maps)
    for skews in ((0, 1, 0, 0), (0, 0, 2, 0), (0, 0, 0, 3)):
        views = []
        for m, k in zip(maps, skews):
            v = torch.zeros((m.size + 4,), dtype=torch.int32, device=DEV)[k:k + m.size].view(m.shape)
            v.copy_(torch.from_numpy(m))
            assert v.data_ptr() % 16 == 4 * k
            views.append(v)
        meter = vkn.STQMeter(**K, device=DEV)
        meter.update_state(*views)
        _same_tables(meter.tables(0), ref.tables(0), f'skews {skews}')
        assert meter.tables(0)['status'] == 0 and meter.tables(0)['frames'] == 2


def test_lds_overflow_takes_the_global_path(vkn):
    p = stq_ref.LDS_OVERFLOW
    _against_ref(vkn, stq_ref.noisy_maps(p['seed'], p['H'], p['W']), 'LDS overflow')


def test_contention_on_one_dominant_tube(vkn):
    p = stq_ref.CONTENTION
    meter, ref = _against_ref(vkn, stq_ref.dominant_maps(p['seed'], p['H'], p['W']), 'contention')
    assert meter.tables(0)['pair_counts'].max() * 2 > p['H'] * p['W']


def test_full_table_is_flagged_and_nothing_else_is_disturbed(vkn):
    p = stq_ref.CAPACITY
    maps = stq_ref.noisy_maps(p['seed'], p['H'], p['W'])
    meter = vkn.STQMeter(**K, capacity=dict(pair=16), device=DEV)
    meter.update_state(*_dev(*maps))
    ref = stq_ref.STQRef(**K)
    ref.update_state(*maps)
    with pytest.raises(vkn.VknError) as e:
        meter.result()
    assert 'FULL' in str(e.value) and 'pair' in str(e.value) and 'gt table' not in str(e.value) and 'pred table' not in str(e.value)
    with pytest.raises(vkn.VknError):
        meter.check_status()
    got, want = meter.tables(0), ref.tables(0)
    assert got['status'] == vkn._lib.STQ['VKN_STQ_STATUS_FULL_PAIR']
    for k in ('confusion', 'gt_keys', 'gt_counts', 'pred_keys', 'pred_counts'):
        assert np.array_equal(got[k], want[k]), k
    # the 16 slots hold 16 of the true pairs with their true counts
    assert got['pair_keys'].size == 16 and all(ref.seqs[0]['pair'][int(k)] == int(c) for k, c in zip(got['pair_keys'], got['pair_counts']))
    meter.reset_states()
    args, ids, fm, z = stq_ref.load_case('kitti')
    assert args == K
    dm = _dev(*fm)
    for s, sid in enumerate(ids):
        meter.update_state(*(m[s] for m in dm), sequence_id=sid)
    for s, sid in enumerate(ids):
        stq_ref.assert_tables(meter.tables(sid), z, 1, s, 'kitti after reset_states')
    stq_ref.assert_result(meter.result(), z, 1, [meter.tables(sid)['pair_keys'].size for sid in ids], 'kitti after reset_states')


@pytest.mark.parametrize('what,bit', (('id_2_16', 'VKN_STQ_STATUS_ID_RANGE'), ('id_negative', 'VKN_STQ_STATUS_ID_RANGE'),
                                      ('class_200', 'VKN_STQ_STATUS_CLASS_RANGE')))
def test_range_flags_skip_the_pixel_and_count_the_rest(vkn, what, bit):
    maps = [m.copy() for m in stq_ref.seeded_maps(31, 24, 39, cell=4)]
    gs, gi, ps, pi = maps
    y, x = np.argwhere(np.isin(gs, K['things_list']) & (gi > 0))[5]          # a pixel that counts in every table it can
    if what == 'id_2_16':
        pi[y, x] = 2 ** 16
    elif what == 'id_negative':
        gi[y, x] = -3
    else:
        ps[y, x] = 200
    meter = vkn.STQMeter(**K, device=DEV)
    meter.update_state(*_dev(*maps))
    keep = np.ones(gs.shape, bool)
    keep[y, x] = False
    ref = stq_ref.STQRef(**K)
    ref.update_state(*(m[keep][None] for m in maps))                         # the same maps without that pixel
    got = meter.tables(0)
    assert got['status'] == vkn._lib.STQ[bit] and ref.tables(0)['status'] == 0
    _same_tables(got, ref.tables(0), what)
    with pytest.raises(vkn.VknError) as e:
        meter.result()
    assert bit[len('VKN_STQ_STATUS_'):] in str(e.value)


def test_buffer_contract(vkn):
    lib = vkn._lib
    L = lib.lib()
    cfg = vkn.ops.stq_cfg(K['num_classes'], K['ignore_label'], K['label_bit_shift'], K['offset'], True, 64, 64, 256)
    nbytes, off = vkn.ops.stq_layout(cfg)
    assert nbytes == L.vkn_stq_state_bytes(ctypes.byref(cfg)) and nbytes % 16 == 0
    B, HW = 2, 24 * 39
    maps = _dev(*(np.stack([m, m[::-1]]).reshape(B, HW) for m in stq_ref.seeded_maps(41, 24, 39, cell=4)))
    thing = torch.zeros((20,), dtype=torch.uint8, device=DEV)
    thing[K['things_list']] = 1
    A = Arena(DEV)
    state = A.out((nbytes,), torch.uint8, name='state', align=16)
    ptrs = [ctypes.c_void_p(m.data_ptr()) for m in maps]
    with torch.cuda.device(DEV):
        assert L.vkn_stq_reset(ctypes.byref(cfg), state.ptr, nbytes, None) == 0
        A.check('reset')                                                     # all of the state written, nothing else
        raw = state.t.cpu().numpy()
        assert not raw[:off[2]].any() and (raw[off[2]:off[3]].view(np.int64) == -1).all() and not raw[off[3]:off[4]].any()
        with frozen(thing, *maps):
            assert L.vkn_stq_update_i32(ctypes.byref(cfg), state.ptr, nbytes, ctypes.c_void_p(thing.data_ptr()), *ptrs, B, HW, None) == 0
        A.check('update')
        before = state.t.clone()
        for d in (-16, 16):
            assert L.vkn_stq_update_i32(ctypes.byref(cfg), state.ptr, nbytes + d, ctypes.c_void_p(thing.data_ptr()), *ptrs, B, HW, None) == E_WORKSPACE
            assert L.vkn_stq_reset(ctypes.byref(cfg), state.ptr, nbytes + d, None) == E_WORKSPACE
        assert L.vkn_stq_update_i32(ctypes.byref(cfg), ctypes.c_void_p(state.addr + 4), nbytes, ctypes.c_void_p(thing.data_ptr()), *ptrs, B, HW, None) == E_ALIGN
        assert L.vkn_stq_reset(ctypes.byref(cfg), ctypes.c_void_p(state.addr + 4), nbytes, None) == E_ALIGN
    A.check('refusals')
    assert torch.equal(state.t, before)
    ref = stq_ref.STQRef(**K)
    ref.update_state(*(m.cpu().numpy() for m in maps))
    raw = state.t.cpu().numpy()
    n = 20
    assert raw[:8].view(np.uint32).tolist() == [0, B] and np.array_equal(raw[off[1]:off[1] + n * n * 8].view(np.int64).reshape(n, n), ref.tables(0)['confusion'])


def test_chain_from_the_tracking_tail(vkn):
    """`ops.track_maps` on the pan_video golden's panoptic result, fed straight in as pred_* against synthetic ground truth"""
    from importlib import import_module
    from helpers import PAN_CFG, load_pan_golden, make_pan_case
    tt = import_module('video_k_net_amd.track_tail')
    g, case = load_pan_golden('pan_video')
    cls, logits, meta = make_pan_case(case)
    T, n_stuff = case['T'], case['ncls'] - case['T']
    seg, info, nseg, _ = vkn.ops.panoptic_joint(cls.to(DEV), logits.to(DEV), case['Np'], T, case['Np'], PAN_CFG['instance_score_thr'],
                                                PAN_CFG['overlap_thr'], meta['img_shape'][:2], meta['batch_input_shape'], meta['ori_shape'][:2],
                                                upsample_stride=case['up'], want_bbox=True)
    _, _, _, segid, count = vkn.ops.track_boxes(seg, info, nseg, T)
    Bf, Kk = int(info.shape[0]), int(info.shape[1])
    ids = (torch.arange(Kk, dtype=torch.int64, device=DEV)[None] * 3 + 1).repeat(Bf, 1).contiguous()
    table = torch.tensor(tt.sem_of_label(T, n_stuff, False), dtype=torch.int32, device=DEV)
    track_map, semantic_map = vkn.ops.track_maps(seg, segid, count, ids, count, info, table)
    assert track_map.dtype == semantic_map.dtype == torch.int32 and track_map.is_cuda and track_map.dim() == 3
    sem_h, trk_h = semantic_map.cpu().numpy(), track_map.cpu().numpy()
    assert (trk_h > 0).any() and int(sem_h.max()) < 255
    nc = int(sem_h.max()) + 1
    things = sorted({int(c) for c in np.unique(sem_h[trk_h > 0])})
    cfg = dict(num_classes=nc, things_list=things, ignore_label=255, label_bit_shift=16, offset=2 ** 16 * 256)
    H, W = sem_h.shape[1:]
    rng = np.random.default_rng(5)
    gt_sem = np.roll(sem_h, 3, axis=2).astype(np.int32)                       # the prediction, shifted: tubes intersect
    gt_ins = np.roll(trk_h, 3, axis=2).astype(np.int32)
    gt_sem[:, :, :2] = 255
    gt_ins[rng.random(gt_ins.shape) < 0.02] = 0                               # crowd pixels
    meter = vkn.STQMeter(**cfg, device=DEV)
    meter.update_state(*_dev(gt_sem, gt_ins), semantic_map, track_map, sequence_id='video')
    ref = stq_ref.STQRef(**cfg)
    ref.update_state(gt_sem, gt_ins, sem_h, trk_h, sequence_id='video')
    got, want = meter.tables('video'), ref.tables('video')
    _same_tables(got, want, 'chain')
    assert got['status'] == 0 and got['frames'] == Bf and want['pair_keys'].size > 0
    res, rres = meter.result(), ref.result()
    assert res['ID_per_seq'] == ['video'] and res['Length_per_seq'] == [Bf]
    for k in ('STQ', 'AQ', 'IoU'):
        assert abs(float(res[k]) - float(rres[k])) <= max(want['pair_keys'].size, 1) * 2.0 ** -52 * abs(float(rres[k])), k
