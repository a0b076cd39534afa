"""The CPU references of the tracking tail (tests/track_tail_refs.py) checked on their own, without a GPU: against
`tensor_mask2box`, against a literal transcription of the reference's loops on hand-made frames, and the two premises the GPU
tests build on (exactness of the dyadic inputs, near-tie share of the non-dyadic ones).  Plus what the new part of the C ABI
promises before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import track_tail_refs as R

T, S = 2, 3       # thing / stuff classes of the hand-made frames


def _f32(bits_or_float):
    return float(np.float32(bits_or_float))


# the frames: (joint label, rectangle, score) in segment order
FRAMES = {
    'no_things': [(2, (0, 4, 0, 9), 0.5), (4, (4, 7, 0, 9), 0.5)],
    'one_thing': [(3, (0, 7, 0, 9), 0.5), (1, (2, 5, 3, 8), 0.75)],
    'mixed': [(0, (0, 3, 0, 4), 0.9), (2, (3, 7, 0, 9), 0.5), (1, (1, 6, 5, 9), 0.7), (0, (5, 7, 0, 2), 0.6), (4, (0, 1, 4, 9), 0.3)],
}


def _literal_segments(layout):
    """segments_info as the reference's merge writes it, from the layout itself (not through `info`)."""
    out = []
    for i, (label, _, score) in enumerate(layout):
        if label < T:
            out.append(dict(id=i + 1, isthing=True, category_id=label, score=_f32(score), instance_id=0))
        else:
            out.append(dict(id=i + 1, isthing=False, category_id=label - T + 1))
    return out


def _literal_track_map(ids, masks, panoptic_seg):
    """`generate_track_id_maps`, knet/video/knet_quansi_dense_embed_fc_joint_train.py:724-736, as written."""
    final_id_maps = np.zeros(panoptic_seg.shape)
    if len(ids) == 0:
        return final_id_maps
    masks = masks.bool()
    for i, id in enumerate(ids):
        mask = masks[i].cpu().numpy()
        final_id_maps[mask] = id
    return final_id_maps


def _literal_semantic(panoptic_seg, segments_info, kitti_step, num_stuff_classes):
    """`get_semantic_seg`, :698-722, as written."""
    kitti_step2cityscpaes = [11, 13]
    semantic_seg = np.zeros(panoptic_seg.shape)
    for segment in segments_info:
        if segment['isthing'] == True:  # noqa: E712
            if kitti_step:
                cat_cur = kitti_step2cityscpaes[segment["category_id"]]
                semantic_seg[panoptic_seg == segment["id"]] = cat_cur
            else:
                semantic_seg[panoptic_seg == segment["id"]] = segment["category_id"] + num_stuff_classes
        else:
            if kitti_step:
                cat_cur = segment["category_id"]
                cat_cur -= 1
                offset = 0
                for thing_id in kitti_step2cityscpaes:
                    if cat_cur + offset >= thing_id:
                        offset += 1
                cat_cur += offset
                semantic_seg[panoptic_seg == segment["id"]] = cat_cur
            else:
                semantic_seg[panoptic_seg == segment["id"]] = segment["category_id"] - 1
    return semantic_seg


@pytest.mark.parametrize('name', list(FRAMES))
def test_boxes_without_filter_are_tensor_mask2box(name):
    layout = FRAMES[name]
    seg, info = R.hand_frame(7, 9, layout, T)
    got = R.track_boxes(seg, info, T)
    things = [i + 1 for i, (label, _, _) in enumerate(layout) if label < T]
    assert got['segid'].tolist() == things
    assert got['labels'].tolist() == [layout[i - 1][0] for i in things]
    assert got['rows'].tolist() == [10 + i - 1 for i in things]
    assert got['det'][:, 4].tolist() == [_f32(layout[i - 1][2]) for i in things]
    if things:
        want = R.tensor_mask2box(torch.from_numpy(np.stack([seg == i for i in things])))
        assert np.array_equal(got['det'][:, :4], want.astype(np.float32))
    else:
        assert got['det'].shape == (0, 5)


IDS = {'no_things': [[]], 'one_thing': [[], [4], [-1]], 'mixed': [[], [7, -1, 0], [3], [-1, 5], [0, 1, 2]]}


@pytest.mark.parametrize('name', list(FRAMES))
@pytest.mark.parametrize('kitti', [False, True])
def test_maps_are_the_reference_loops(name, kitti):
    layout = FRAMES[name]
    seg, info = R.hand_frame(7, 9, layout, T)
    segs = _literal_segments(layout)
    assert np.array_equal(R.semantic_map(seg, info, T, S, kitti), _literal_semantic(seg, segs, kitti, S))
    masks = [seg == s['id'] for s in segs if s['isthing']]
    for ids in IDS[name]:
        if len(ids):                                      # :591-592 on what the tracker returned
            t = torch.tensor(ids) + 1
            t[t == -1] = 0
            want = _literal_track_map(t, torch.from_numpy(np.stack(masks)), seg)
        else:                                             # :597-598
            want = _literal_track_map([], None, seg)
        assert np.array_equal(R.track_map(seg, info, T, ids), want), ids


def test_label_tables_of_the_package(vkn):
    """`track_tail.sem_of_label` (what TrackTail uploads) gives the reference's semantic class for every joint label, both mappings."""
    from importlib import import_module
    tt = import_module('video_k_net_amd.track_tail')
    for kitti, (t, s) in ((False, (8, 11)), (True, (2, 17)), (False, (58, 66))):
        table = tt.sem_of_label(t, s, kitti)
        assert len(table) == t + s
        for label in range(t + s):
            seg = np.ones((1, 1), dtype=np.int32)
            info = np.asarray([[0, label, 1, 1, 1, 0]], dtype=np.int32)
            assert table[label] == int(R.semantic_map(seg, info, t, s, kitti)[0, 0]), (kitti, label)
    assert sorted(tt.sem_of_label(2, 17, True)) == list(range(19))       # KITTI-STEP: a permutation of the 19 Cityscapes train ids
    with pytest.raises(ValueError):
        tt.sem_of_label(3, 17, True)


@pytest.mark.parametrize('case', R.DYADIC_CASES)
def test_dyadic_inputs_are_exact(case):
    """The exactness premise: float32 and float64 `semantic_thing` agree on every pixel of the dyadic inputs, whose top-two margin is
    an exact multiple of 2^-8 — and exactly zero on a sizeable share of the map (the deliberate ties)."""
    (hs, ws), size, seed = case
    x = R.dyadic_logits(R.CS, hs, ws, seed, R.T_SEM)
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 8
    a, m32 = R.semantic_thing(x, size, R.T_SEM, torch.float32)
    b, m64 = R.semantic_thing(x, size, R.T_SEM, torch.float64)
    assert np.array_equal(a, b)
    assert np.array_equal(m32.astype(np.float64), m64) and np.array_equal(m64 * 256, np.round(m64 * 256))
    assert (m64 == 0).mean() > 0.2
    assert 0.2 < a.mean() < 0.8


@pytest.mark.parametrize('case', R.NONDYADIC_CASES)
def test_nondyadic_inputs_keep_the_near_tie_cap(case):
    (hs, ws), size, seed = case
    x = R.float_logits(R.CS, hs, ws, seed)
    thing, margin = R.semantic_thing(x, size, R.T_SEM, torch.float64)
    assert (margin < R.MARGIN).mean() <= R.NEAR_TIE_CAP
    assert 0.2 < thing.mean() < 0.8


# ---------------------------------------------------------------------------------------------------- the ABI, before any launch
def test_tracker_device_count_entry_refuses_before_any_launch(vkn):
    """vkn_qd_tracker_match_dev_f32: every pointer is required, n_max lies in [1, max_dets]; checked on the host (fake pointers)."""
    L = vkn._lib.lib()
    trk = vkn.QuasiDenseEmbedTracker(max_dets=32, max_tracklets=64)
    cfg = trk._make_cfg(16)
    nb, nw = L.vkn_qd_tracker_state_bytes(ctypes.byref(cfg)), L.vkn_qd_tracker_workspace_bytes(ctypes.byref(cfg))
    p = 0x10000

    def call(cfg_=cfg, state=p, bboxes=p, labels=p, embeds=p, n_dev=p, n_max=8, ob=p, ol=p, oi=p, oc=p, ws=p, nws=nw):
        return L.vkn_qd_tracker_match_dev_f32(ctypes.byref(cfg_) if cfg_ is not None else None, state, nb, bboxes, labels, embeds, n_dev,
                                              n_max, 0, ob, ol, oi, oc, ws, nws, None)

    for name in ('cfg_', 'state', 'bboxes', 'labels', 'embeds', 'n_dev', 'ob', 'ol', 'oi', 'oc'):
        assert call(**{name: None}) == -1, name
    assert call(n_max=0) == -1 and call(n_max=-3) == -1
    assert call(n_max=33) == -2                              # more rows than max_dets
    assert call(ws=None) == -3 and call(nws=nw - 1) == -3
    assert call(state=p + 16) == -5 and call(ws=p + 16) == -5


def test_track_entries_refuse_before_any_launch(vkn):
    """NULL pointers, K over the LDS capacity, a map of 2^31 bytes and misaligned pointers are refused by the host-side checks, in this
    order, before a pointer is looked at (the fake pointers below are never dereferenced)."""
    L = vkn._lib.lib()
    cap = vkn._lib.TRACK_MAX_K
    assert cap >= 100 + 66                                   # max_per_img + stuff of the largest shipped config (VIP-Seg)
    assert L.vkn_track_boxes_workspace_bytes(1, cap) > 0 and L.vkn_track_boxes_workspace_bytes(1, cap + 1) == 0
    assert L.vkn_track_maps_workspace_bytes(2, cap) > 0 and L.vkn_track_maps_workspace_bytes(2, cap + 1) == 0
    p = 0x10000

    def boxes(seg=p, info=p, nseg=p, sem=None, K=8, Ho=16, Wo=16, det=p, labels=p, rows=p, segid=p, count=p, tm=None, ws=p):
        return L.vkn_track_boxes_f32(seg, info, nseg, sem, 5, 4, 4, 2, 1, K, Ho, Wo, det, labels, rows, segid, count, tm, ws, 1 << 20, None)

    def maps(seg=p, segid=p, count=p, ids=p, n_ids=p, info=p, table=p, K=8, Ho=16, Wo=16, tmap=p, smap=p, ws=p):
        return L.vkn_track_maps_i32(seg, segid, count, ids, n_ids, 256, info, table, 5, 1, K, Ho, Wo, tmap, smap, ws, 1 << 20, None)

    E_ARG, E_SHAPE, E_WS, E_ALIGN = -1, -2, -3, -5
    for name in ('seg', 'info', 'nseg', 'det', 'labels', 'rows', 'segid', 'count'):
        assert boxes(**{name: None}) == E_ARG, name
    for name in ('seg', 'segid', 'count', 'ids', 'n_ids', 'info', 'table', 'tmap', 'smap'):
        assert maps(**{name: None}) == E_ARG, name
    assert boxes(K=cap + 1) == E_SHAPE and maps(K=cap + 1) == E_SHAPE
    assert boxes(Ho=1 << 15, Wo=1 << 14) == E_SHAPE and maps(Ho=1 << 15, Wo=1 << 14) == E_SHAPE      # Ho * Wo * 4 == 2^31
    for name in ('seg', 'info', 'nseg', 'det', 'labels', 'rows', 'segid', 'count', 'sem', 'tm'):
        assert boxes(**{name: p + 4}) == E_ALIGN, name
    for name in ('seg', 'segid', 'count', 'ids', 'info', 'tmap', 'smap'):
        assert maps(**{name: p + 4}) == E_ALIGN, name
    assert maps(n_ids=p + 2) == E_ALIGN and maps(table=p + 2) == E_ALIGN
    assert boxes(ws=None) == E_WS and maps(ws=None) == E_WS
