"""GPU: the thing-first panoptic merge (`vkn_panoptic_thing_first_u8`, csrc/vkn_merge.hip: k_mg_count / k_mg_paint) on its own and
bit for bit.  The kernel is integer work on one-byte masks plus one fp64 division and two fp64 comparisons, so it has one right answer:
`oracle.knet_oracle.thing_first_merge`, the reference's loop restated on the CPU and pinned to the unmodified reference by the
`merge_tf_*` fixtures (tests/test_oracle_merge_thing_first.py).  Every comparison here is `array_equal`: the map, nseg and all five
`info` columns of every step, rejected and stopped steps included."""
import numpy as np
import pytest
import torch

from helpers import MERGE_TF, load_merge_tf, merge_tf_oracle, pan_info_rows
from oracle import synth
from oracle.knet_oracle import thing_first_feat_rows, thing_first_merge

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_WORKSPACE = -3
THR = dict(instance_score_thr=0.25, iou_thr=0.5, stuff_max_area=12)
GRID_PIXELS = 2048 * 256          # the launcher's grid cap: one trip of the grid-stride loops


def _dev(a, dtype):
    """numpy -> device tensor, None (a null pointer at the ABI) for an empty array"""
    return None if a is None or a.size == 0 else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _abi(vkn, a, thr, ws=None, ws_bytes=None):
    """`vkn_panoptic_thing_first_u8` through ctypes.  a: the arguments of `thing_first_merge` (masks of any dtype, taken as raw
    bytes [K, HW]); outputs prefilled with -7, the workspace (unless given) with 0xA5.  -> (return code, map, info, nseg)."""
    L, P = vkn._lib.lib(), vkn.ops._ptr
    Kt, Ks = len(a['thing_order']), len(a['stuff_order'])
    HW = int(np.prod(a['thing_masks'].shape[1:]))
    u8 = lambda m: np.asarray(m).astype(np.uint8, copy=False).reshape(m.shape[0], HW)  # noqa: E731
    d = [_dev(u8(a['thing_masks']), torch.uint8), _dev(a['thing_scores'], torch.float32), _dev(a['thing_labels'], torch.int32),
         _dev(a['thing_order'], torch.int32), _dev(u8(a['stuff_masks']), torch.uint8), _dev(a['stuff_labels'], torch.int32),
         _dev(a['stuff_order'], torch.int32)]
    need = L.vkn_merge_workspace_bytes(Kt, Ks)
    if ws is None:
        ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    seg = torch.full((HW,), -7, dtype=torch.int32, device=DEV)
    info = torch.full((max(Kt + Ks, 1), 5), -7, dtype=torch.int32, device=DEV)
    nseg = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    rc = L.vkn_panoptic_thing_first_u8(P(d[0]), P(d[1]), P(d[2]), P(d[3]), Kt, P(d[4]), P(d[5]), P(d[6]), Ks, HW,
                                       float(thr['instance_score_thr']), float(thr['iou_thr']), int(thr['stuff_max_area']), P(seg),
                                       P(info if Kt + Ks else None), P(nseg), P(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                       vkn.ops._stream())
    torch.cuda.synchronize()
    return rc, seg.cpu().numpy(), info.cpu().numpy()[:Kt + Ks], int(nseg)


def _ops(vkn, a, thr):
    """the same call through `ops.panoptic_thing_first` (boolean masks [K, H, W])"""
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(DEV)  # noqa: E731
    seg, info, nseg = vkn.ops.panoptic_thing_first(
        t(a['thing_masks'], torch.bool), t(a['thing_scores'], torch.float32), t(a['thing_labels'], torch.int64),
        t(a['thing_order'], torch.int64), t(a['stuff_masks'], torch.bool), t(a['stuff_labels'], torch.int64),
        t(a['stuff_order'], torch.int64), thr['instance_score_thr'], thr['iou_thr'], thr['stuff_max_area'])
    torch.cuda.synchronize()
    return 0, seg.cpu().numpy(), info.cpu().numpy(), int(nseg)


def _same(got, r):
    rc, seg, info, nseg = got
    assert rc == 0
    assert seg.dtype == np.int32 and np.array_equal(seg.reshape(r['panoptic_seg'].shape), r['panoptic_seg'])
    assert info.shape == r['info'].shape and np.array_equal(info, r['info'])
    assert nseg == r['nseg']


def _args(tm, ts, tl, to, sm, sl, so):
    return dict(thing_masks=np.asarray(tm), thing_scores=np.asarray(ts, dtype=np.float32), thing_labels=np.asarray(tl, dtype=np.int64),
                thing_order=np.asarray(to, dtype=np.int64), stuff_masks=np.asarray(sm), stuff_labels=np.asarray(sl, dtype=np.int64),
                stuff_order=np.asarray(so, dtype=np.int64))


# ------------------------------------------------------------------------------------------------------- the reference's fixtures
@pytest.mark.parametrize('name', MERGE_TF)
def test_edge_fixtures_through_the_abi(vkn, name):
    """every threshold edge of the merge_tf_* fixtures (what each holds: tests/test_oracle_merge_thing_first.py) through the C ABI"""
    g, a, thr = load_merge_tf(name)
    args, r = merge_tf_oracle(a, thr)
    assert np.array_equal(r['panoptic_seg'], g['panoptic_seg'])
    _same(_abi(vkn, args, thr), r)


@pytest.fixture(scope='module')
def heads(vkn):
    """the det and the video head with merge_joint=False, built as test_gpu_parity.test_thing_first_merge_vs_reference_golden does"""
    out = []
    for video in (False, True):
        cfg = vkn.configs.roi_head_cfg(video, C=32, heads=8, ffn=64, ncls=5, n_thing=2, n_stuff=3, S=1, up=1, nprop=4, merge_joint=False)
        cfg['test_cfg'] = dict(max_per_img=4, mask_thr=0.5, merge_stuff_thing=dict(overlap_thr=0.6, **THR))
        out.append(vkn.build_head(cfg).to(DEV).eval())
    return out


@pytest.mark.parametrize('name', MERGE_TF)
def test_edge_fixtures_through_the_heads(vkn, heads, name):
    """`KernelIterHead.merge_stuff_thing` and `VideoKernelIterHead.merge_stuff_thing_thing_first` on the device against what the
    reference's methods returned: the map, every segments_info field, and the embeddings the video form hands back — with unsorted
    scores (merge_tf_video) `thing_obj_feat[argsort(-scores)][instance_ids]` is not the identity.  merge_tf_dupstuff takes the
    OR-of-one-label branch, the empty cases hand over [0, H, W] tensors."""
    g, a, thr = load_merge_tf(name)
    det, video = heads
    t = {k: torch.from_numpy(v).to(DEV) for k, v in a.items()}
    cfg = dict(overlap_thr=0.6, **thr)
    args = (t['thing_masks'], t['thing_labels'], t['thing_scores'], t['stuff_masks'], t['stuff_labels'], t['stuff_scores'], cfg)
    seg, info = det.merge_stuff_thing(*args)
    assert seg.dtype == np.int32 and np.array_equal(seg, g['panoptic_seg'])
    assert np.array_equal(pan_info_rows(info), g['info'], equal_nan=True)
    Kt = a['thing_masks'].shape[0]
    feat = torch.from_numpy((100.0 * np.arange(Kt)[:, None] + np.arange(8)[None, :]).astype(np.float32)).to(DEV)
    if 'thing_obj_feat' in a:
        assert torch.equal(feat.cpu(), torch.from_numpy(a['thing_obj_feat']))
    (seg2, info2), got = video.merge_stuff_thing_thing_first(*args, thing_obj_feat=feat)
    assert np.array_equal(seg2, g['panoptic_seg']) and np.array_equal(pan_info_rows(info2), g['info'], equal_nan=True)
    rows = thing_first_feat_rows(np.argsort(-a['thing_scores'], kind='stable'), info2)
    if 'feat_rows' in g:
        assert np.array_equal(rows, g['feat_rows'])
    assert got.shape == (len(rows), 8) and torch.equal(got, feat[torch.from_numpy(rows).to(DEV)])


# ---------------------------------------------------------------------------------------------------------------- pixel counts
@pytest.mark.parametrize('HW', [1, 63, 255, 256, 257, 4160, GRID_PIXELS, GRID_PIXELS + 1, 1572941])
def test_pixel_count_edges(vkn, HW):
    """One pixel, less than a wave, around one workgroup, several workgroups, exactly one trip of the capped grid (2048 x 256), one
    pixel more (second trip, one live thread) and a ragged fourth trip.  Thing 0 is the LAST pixel alone, thing 1 the first pixel
    of the second trip alone (the middle pixel where there is no second trip): a loop that ends early loses them."""
    second = GRID_PIXELS if HW > GRID_PIXELS + 1 else HW // 2          # (at 2048 x 256 + 1 the last pixel is that pixel already)
    tm = synth.rect_masks(5, 1, HW, [(0, 0, HW - 1, 1, HW), (1, 0, second, 1, second + 1)], 3, HW % 977)
    sm = synth.rect_masks(3, 1, HW, [], 3, HW % 977 + 1)
    a = _args(tm, [0.95, 0.9, 0.6, 0.8, 0.7], [0, 1, 1, 0, 1], [0, 1, 3, 4, 2], sm, [3, 1, 2], [2, 0, 1])
    thr = dict(THR, stuff_max_area=max(1, HW // 64))
    r = thing_first_merge(**a, **thr)
    assert r['info'][0, 0] == 1 and r['panoptic_seg'][0, HW - 1] == 1
    if HW > 1:
        assert r['info'][1, 0] == 2 and r['panoptic_seg'][0, second] == 2
        assert (r['info'][5:, 3] > 0).any() and r['nseg'] > 2
    _same(_ops(vkn, a, thr), r)
    if HW in (1, 257, GRID_PIXELS + 1):
        _same(_abi(vkn, a, thr), r)


def _frame_case():
    """1024 x 2048, 12 things, 6 stuff classes, stuff_max_area 4096: rectangles laid out so that every kind of decision occurs
    (asserted on the oracle's rows in the test).  Array order is the reverse of the score order."""
    things = [[(100, 100, 400, 600)],                                   # a clear block
              [(150, 150, 350, 500)],                                   # inside it: rejected
              [(300, 500, 500, 900)],                                   # 1/8 of it painted: clipped
              [(600, 0, 800, 300)],                                     # clear
              [(600, 100, 800, 350)],                                   # 4/5 painted: rejected
              [(700, 200, 900, 400)],                                   # 1/4 painted: clipped
              [(0, 1000, 200, 1400)],
              [(100, 1300, 300, 1700), (250, 1600, 420, 1800)],         # a union, 1/8 of its first part painted
              [(500, 1500, 900, 2000)],
              [],                                                       # empty
              [(900, 1900, 1024, 2048)],                                # the last pixel of the frame
              [(0, 0, 50, 50)]]                                         # below the score threshold
    scores = [0.95, 0.90, 0.85, 0.80, 0.75, 0.70, 0.65, 0.60, 0.55, 0.50, 0.45, 0.20]
    stuff = [[(800, 0, 1024, 2048)],                                    # passes
             [(0, 0, 100, 2048)],                                       # passes, less what a thing holds
             [(450, 1000, 500, 1080)],                                  # 4000 px: under the limit
             [(420, 1100, 484, 1164)],                                  # 4096 px: on the limit
             [(200, 200, 300, 300)],                                    # under a thing
             [(0, 0, 1024, 2048)]]                                      # the rest
    n = len(things)
    tm = synth.rect_masks(n, 1024, 2048, [(n - 1 - k, *r) for k, rs in enumerate(things) for r in rs])
    sm = synth.rect_masks(6, 1024, 2048, [(k, *r) for k, rs in enumerate(stuff) for r in rs])
    ts = np.array(scores[::-1], dtype=np.float32)
    return _args(tm, ts, np.arange(n) % 2, np.argsort(-ts, kind='stable'), sm, [4, 2, 6, 1, 5, 3], np.arange(6))


def test_a_real_frame(vkn):
    a = _frame_case()
    thr = dict(THR, stuff_max_area=4096)
    r = thing_first_merge(**a, **thr)
    info, seg = r['info'], r['panoptic_seg']
    assert info[:12, 3].tolist() == list(range(11, -1, -1))
    full = a['thing_masks'][info[:12, 3]].reshape(12, -1).sum(1)
    painted = np.array([(seg == i).sum() if i else 0 for i in info[:12, 0]])
    kept = info[:12, 0] > 0
    assert not kept[1] and not kept[4] and full[1] > 0 and full[4] > 0                      # rejected for overlap
    assert kept[2] and kept[5] and kept[7] and 0 < painted[2] < full[2] and 0 < painted[5] < full[5] and 0 < painted[7] < full[7]   # clipped
    assert kept[0] and painted[0] == full[0] and not kept[9] and full[9] == 0 and not kept[11]
    assert info[12:, 0].tolist() == [9, 10, 0, 11, 0, 12] and info[14, 3] == 4000 and info[15, 3] == 4096 and info[16, 3] == 0
    assert 0 < info[13, 3] < 100 * 2048 and seg[-1, -1] == 8 and not (seg == 0).any()
    _same(_ops(vkn, a, thr), r)


# ------------------------------------------------------------------------------------------------------------------- decisions
def _blocks(n, side=4):
    """n disjoint side x side blocks on an (n * side) x side map"""
    return synth.rect_masks(n, n * side, side, [(k, k * side, 0, (k + 1) * side, side) for k in range(n)])


@pytest.mark.parametrize('scores,thing_ids', [([0.9, 0.1, 0.8, 0.7], [1, 0, 0, 0]), ([0.9, 0.8, 0.7, 0.1], [1, 2, 3, 0])],
                         ids=['low_second', 'low_last'])
def test_stop_latch(vkn, scores, thing_ids):
    """An explicit paste order that is NOT sorted by score: after the first score below the threshold nothing more is painted and no
    id is consumed, although later things score above it again (the reference `break`s).  The stuff loop has no break: it runs and
    its ids go on from the things' last one."""
    m = _blocks(6)
    a = _args(m[:4], scores, [0, 1, 0, 1], [0, 1, 2, 3], m[4:], [2, 1], [1, 0])
    r = thing_first_merge(**a, **THR)
    assert r['info'][:4, 0].tolist() == thing_ids and r['info'][4:, 0].tolist() == [max(thing_ids) + 1, max(thing_ids) + 2]
    assert r['info'][4:, 3].tolist() == [16, 16] and all((r['panoptic_seg'][4 * k:4 * k + 4] == i).all() for k, i in enumerate(thing_ids))
    _same(_ops(vkn, a, THR), r)
    _same(_abi(vkn, a, THR), r)


@pytest.mark.parametrize('kind,thr,last_score,ids', [
    ('ratio', dict(instance_score_thr=0.25, iou_thr=0.6 - 1e-9, stuff_max_area=1), 0.25, [1, 0, 2, 3]),
    ('score', dict(instance_score_thr=0.25 + 1e-9, iou_thr=0.6, stuff_max_area=1), 0.25, [1, 2, 0, 3]),
    ('score', dict(instance_score_thr=0.7, iou_thr=0.6, stuff_max_area=1), 0.7, [1, 2, 0, 3]),           # float32(0.7) < 0.7
], ids=['ratio', 'score', 'score_rounds_down'])
def test_comparisons_are_made_in_fp64(vkn, kind, thr, last_score, ids):
    """Scores and intersect / area against the thresholds as Python evaluates them: in double precision.  Each case sits where the
    fp64 comparison decides and the same comparison with both sides rounded to fp32 is a tie, which decides the other way."""
    tm = synth.rect_masks(3, 8, 12, [(0, 0, 0, 8, 8), (1, 3, 5, 4, 10), (2, 0, 10, 8, 12)])        # block; 3 of 5 px in it; clear
    sm = synth.rect_masks(1, 8, 12, [(0, 0, 0, 8, 12)])
    a = _args(tm, [0.95, 0.9, last_score], [0, 1, 1], [0, 1, 2], sm, [1], [0])
    ratio, score = 3 * 1.0 / 5, a['thing_scores'][2]
    if kind == 'ratio':
        assert ratio > thr['iou_thr'] and np.float32(ratio) == np.float32(thr['iou_thr']) and not float(score) < thr['instance_score_thr']
    else:
        assert float(score) < thr['instance_score_thr'] and score == np.float32(thr['instance_score_thr']) and not ratio > thr['iou_thr']
    r = thing_first_merge(**a, **thr)
    assert r['info'][:, 0].tolist() == ids
    _same(_ops(vkn, a, thr), r)


def test_every_nonzero_byte_is_on(vkn):
    """raw u8 masks holding 0, 1, 2, 128 and 255 give what the 0 / 1 masks give"""
    H, W = 37, 53
    tm = synth.rect_masks(5, H, W, [], 5, 11)
    sm = synth.rect_masks(3, H, W, [], 3, 12)
    a = _args(tm, [0.5, 0.9, 0.3, 0.7, 0.2], [0, 1, 1, 0, 1], [1, 3, 0, 2, 4], sm, [1, 2, 3], [2, 0, 1])
    r = thing_first_merge(**a, **THR)
    assert r['nseg'] >= 3
    vals = np.array([1, 2, 128, 255], dtype=np.uint8)
    raw = dict(a)
    for k in ('thing_masks', 'stuff_masks'):
        m = a[k]
        raw[k] = np.where(m, vals[np.arange(m.size).reshape(m.shape) % 4], 0).astype(np.uint8)
        assert set(np.unique(raw[k]).tolist()) == {0, 1, 2, 128, 255}
    _same(_abi(vkn, a, THR), r)
    _same(_abi(vkn, raw, THR), r)


# ------------------------------------------------------------------------------------------------------------ degenerate counts
def test_degenerate_counts(vkn):
    L = vkn._lib.lib()
    H, W = 9, 14
    tm = synth.rect_masks(3, H, W, [], 3, 21)
    sm = synth.rect_masks(2, H, W, [], 2, 22)
    none_t, none_s = np.zeros((0, H, W), dtype=bool), np.zeros((0, H, W), dtype=bool)
    full = _args(tm, [0.9, 0.5, 0.7], [0, 1, 1], [0, 2, 1], sm, [2, 1], [1, 0])
    cases = {'no things': dict(full, thing_masks=none_t, thing_scores=np.zeros(0, np.float32), thing_labels=np.zeros(0, np.int64),
                               thing_order=np.zeros(0, np.int64)),
             'no stuff': dict(full, stuff_masks=none_s, stuff_labels=np.zeros(0, np.int64), stuff_order=np.zeros(0, np.int64))}
    cases['neither'] = dict(cases['no things'], stuff_masks=none_s, stuff_labels=np.zeros(0, np.int64), stuff_order=np.zeros(0, np.int64))
    thr = dict(THR, stuff_max_area=1)
    for tag, a in cases.items():
        Kt, Ks = len(a['thing_order']), len(a['stuff_order'])
        # two counters per step, one {id, stop} slot per step and one behind the last: at least that much, whatever the padding
        assert L.vkn_merge_workspace_bytes(Kt, Ks) >= 8 * (Kt + Ks) + 8 * (Kt + Ks + 1), tag
        r = thing_first_merge(**a, **thr)
        if tag == 'neither':
            assert r['nseg'] == 0 and r['info'].shape == (0, 5) and r['panoptic_seg'].shape == (H, W) and not r['panoptic_seg'].any()
        else:
            assert r['nseg'] > 0
        _same(_abi(vkn, a, thr), r)                                        # null pointers for the absent side
        _same(_ops(vkn, a, thr), r)                                        # [0, H, W] tensors
    assert L.vkn_merge_workspace_bytes(-1, 2) == 0 and L.vkn_merge_workspace_bytes(2, -1) == 0 and L.vkn_merge_workspace_bytes(-1, -1) == 0
    # a workspace one byte short: refused, nothing written
    need = L.vkn_merge_workspace_bytes(3, 2)
    rc, seg, info, nseg = _abi(vkn, full, thr, ws_bytes=need - 1)
    assert rc == E_WORKSPACE and (seg == -7).all() and (info == -7).all() and nseg == -7
    _same(_abi(vkn, full, thr, ws_bytes=need), thing_first_merge(**full, **thr))


def test_same_workspace_twice_with_a_larger_problem_in_between(vkn):
    """The counters are accumulated atomically into workspace that the launcher clears: a second run into the same, now dirty,
    workspace gives the same bits as the first."""
    small = _args(synth.rect_masks(4, 20, 30, [], 4, 31), [0.9, 0.5, 0.7, 0.6], [0, 1, 1, 0], [0, 2, 3, 1],
                  synth.rect_masks(3, 20, 30, [], 3, 32), [2, 1, 3], [1, 0, 2])
    large = _args(synth.rect_masks(9, 64, 96, [], 9, 33), np.linspace(0.9, 0.3, 9), np.arange(9) % 2, np.arange(9)[::-1],
                  synth.rect_masks(5, 64, 96, [], 5, 34), [5, 4, 3, 2, 1], np.arange(5))
    ws = torch.full((vkn._lib.lib().vkn_merge_workspace_bytes(9, 5),), 0xFF, dtype=torch.uint8, device=DEV)
    first = _abi(vkn, small, THR, ws=ws)
    _same(_abi(vkn, large, THR, ws=ws), thing_first_merge(**large, **THR))
    second = _abi(vkn, small, THR, ws=ws)
    _same(first, thing_first_merge(**small, **THR))
    assert first[0] == second[0] == 0 and all(np.array_equal(x, y) for x, y in zip(first[1:3], second[1:3])) and first[3] == second[3]
