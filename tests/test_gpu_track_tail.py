"""The video detector's tracking tail on the MI355X (video-k-net_amd/csrc/vkn_tracktail.hip, include/vkn_track.h): semantic filter +
thing boxes (vkn_track_boxes_f32), the track-id and semantic maps (vkn_track_maps_i32), and `TrackTail` end to end.  Every comparison
of the two entry points goes through the C ABI on guarded buffers and is exact: integer outputs, min / max boxes, and a filter whose
inputs are chosen so that fp32 is exact (dyadic cases) or whose near-ties are excluded by a float64 margin (non-dyadic cases).
The CPU references are tests/track_tail_refs.py (checked on their own by tests/test_track_tail_refs.py)."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import track_tail_refs as R
from helpers import PAN_CFG
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T, NSTUFF, NP = 2, 4, 8                       # thing classes, stuff kernels, thing kernels of the panoptic inputs
K = NP + NSTUFF
GUARD = 256                                   # guard bytes before and after every output buffer
SHAPES = ((16, 64), (37, 53), (1, 70), (65, 129))
MAP_CASES = [(size, B) for size in SHAPES for B in (1, 3)] + [(SHAPES[0], 'special')]
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -5


# ---------------------------------------------------------------------------------------------------- guarded buffers + ABI calls
class Guarded:
    """A device buffer with GUARD sentinel bytes on both sides; `.t` is the payload viewed as `dtype` `shape`."""

    def __init__(self, shape, dtype, fill=0x5A):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.pad = (n + 15) // 16 * 16
        self.raw = torch.full((2 * GUARD + self.pad,), fill, dtype=torch.uint8, device=DEV)
        self.n, self.fill = n, fill
        self.t = self.raw[GUARD:GUARD + n].view(dtype).reshape(shape)

    def guards_intact(self):
        r = self.raw.cpu().numpy()
        return bool((r[:GUARD] == self.fill).all() and (r[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.raw.cpu().numpy() == self.fill).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=DEV)


def call_boxes(vkn, seg, info, nseg, sem, n_thing, want_mask=True):
    """vkn_track_boxes_f32 on device tensors -> dict of numpy outputs (guards checked)."""
    L = vkn._lib.lib()
    B, Ho, Wo = seg.shape
    Kk = info.shape[1]
    out = dict(det=Guarded((B, Kk, 5), torch.float32), labels=Guarded((B, Kk), torch.int64), rows=Guarded((B, Kk), torch.int32),
               segid=Guarded((B, Kk), torch.int32), count=Guarded((B,), torch.int32))
    if want_mask:
        out['thing_mask'] = Guarded((B, Ho, Wo), torch.uint8)
    ws = _ws(L.vkn_track_boxes_workspace_bytes(B, Kk))
    Cs, hs, wsw = (sem.shape[1:] if sem is not None else (0, 0, 0))
    rc = L.vkn_track_boxes_f32(_p(seg), _p(info), _p(nseg), _p(sem), Cs, hs, wsw, n_thing, B, Kk, Ho, Wo, _p(out['det'].t),
                               _p(out['labels'].t), _p(out['rows'].t), _p(out['segid'].t), _p(out['count'].t),
                               _p(out['thing_mask'].t) if want_mask else None, _p(ws), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for name, g in out.items():
        assert g.guards_intact(), name
    return {k: g.t.cpu().numpy() for k, g in out.items()}, {k: g.t for k, g in out.items()}


def call_maps(vkn, seg, segid, count, ids, n_ids, info, table):
    L = vkn._lib.lib()
    B, Ho, Wo = seg.shape
    Kk = info.shape[1]
    tm, sm = Guarded((B, Ho, Wo), torch.int32), Guarded((B, Ho, Wo), torch.int32)
    ws = _ws(L.vkn_track_maps_workspace_bytes(B, Kk))
    rc = L.vkn_track_maps_i32(_p(seg), _p(segid), _p(count), _p(ids), _p(n_ids), ids.shape[1], _p(info), _p(table), table.numel(), B, Kk,
                              Ho, Wo, _p(tm.t), _p(sm.t), _p(ws), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert tm.guards_intact() and sm.guards_intact()
    return tm.t.cpu().numpy(), sm.t.cpu().numpy()


def check_against_helper(got, seg, info, n_thing, thing=None):
    """Every frame of a vkn_track_boxes_f32 result == tests/track_tail_refs.track_boxes, bit for bit; rows beyond count are zero."""
    for b in range(seg.shape[0]):
        want = R.track_boxes(seg[b], info[b], n_thing, None if thing is None else thing[b])
        n = len(want['segid'])
        assert int(got['count'][b]) == n
        assert np.array_equal(got['det'][b, :n].view(np.int32), want['det'].view(np.int32))
        for name in ('labels', 'rows', 'segid'):
            assert np.array_equal(got[name][b, :n], want[name]), name
            assert not got[name][b, n:].any(), name
        assert not got['det'][b, n:].view(np.int32).any()


# ---------------------------------------------------------------------------------------------------- the maps of test (1)
def _panoptic(vkn, cls, logits, size):
    seg, info, nseg, bbox = vkn.ops.panoptic_joint(cls.to(DEV), logits.to(DEV), NP, T, NP, PAN_CFG['instance_score_thr'],
                                                   PAN_CFG['overlap_thr'], size, size, size, upsample_stride=1, want_bbox=True)
    torch.cuda.synchronize()
    assert (nseg >= 0).all()
    return seg, info, nseg, bbox


_PAN = {}


def pan_maps(vkn, size, B):
    """(seg, info, nseg, bbox) device tensors of vkn_panoptic_joint_f32 on small structured logits; computed once per (size, B).
    B == 'special': three frames at this size — no segment at all, thing segments only, stuff segments only."""
    key = (size, B)
    if key not in _PAN:
        Ho, Wo = size
        nb = 3 if B == 'special' else B
        cls, logits = synth.panoptic_inputs(nb, K, NP, T + NSTUFF, Ho, Wo, 5 + Ho + nb)
        cls, logits = torch.from_numpy(cls), torch.from_numpy(logits)
        if B == 'special':
            logits[0] = -20.0                  # nothing reaches probability 0.5: every entry is rejected
            logits[1, NP:] = -20.0             # no stuff
            logits[2, :NP] = -20.0             # no things
        _PAN[key] = _panoptic(vkn, cls, logits, size)
    return _PAN[key]


def _compact(info_b):
    acc = np.nonzero((info_b[:, 2] > 0) & (info_b[:, 1] < T))[0]
    return acc[np.argsort(info_b[acc, 2], kind='stable')]


# ---------------------------------------------------------------------------------------------------- 1. filter off
@pytest.mark.parametrize('size,B', MAP_CASES)
def test_filter_off_equals_the_panoptic_bbox(vkn, size, B):
    seg, info, nseg, bbox = pan_maps(vkn, size, B)
    got, _ = call_boxes(vkn, seg, info, nseg, None, T)
    seg_h, info_h, bbox_h, nseg_h = seg.cpu().numpy(), info.cpu().numpy(), bbox.cpu().numpy(), nseg.cpu().numpy()
    assert (got['thing_mask'] == 1).all()
    counts = []
    for b in range(seg_h.shape[0]):
        acc = _compact(info_h[b])
        n = len(acc)
        counts.append(n)
        assert int(got['count'][b]) == n
        assert np.array_equal(got['det'][b, :n, :4], bbox_h[b][acc].astype(np.float32))
        assert np.array_equal(got['det'][b, :n, 4].view(np.int32), info_h[b][acc, 5])
        assert np.array_equal(got['labels'][b, :n], info_h[b][acc, 1]) and np.array_equal(got['rows'][b, :n], info_h[b][acc, 0])
        assert np.array_equal(got['segid'][b, :n], info_h[b][acc, 2])
        assert not got['det'][b, n:].view(np.int32).any() and not got['labels'][b, n:].any() and not got['rows'][b, n:].any() \
            and not got['segid'][b, n:].any()
    check_against_helper(got, seg_h, info_h, T)
    if B == 'special':
        assert nseg_h[0] == 0 and counts[0] == 0
        assert counts[1] > 0 and counts[1] == nseg_h[1]                   # thing segments only
        assert counts[2] == 0 and nseg_h[2] > 0                           # stuff segments only
    elif B == 3:
        assert len(set(nseg_h.tolist())) > 1 and sum(counts) > 0          # a different nseg per frame
    else:
        assert counts[0] > 0


# ---------------------------------------------------------------------------------------------------- 2 / 3. filter on
def _filter_layout(Ho, Wo):
    """Thing and stuff rectangles of a filter frame, in segment order: one segment on every border, one in the left (tie) third, one
    inside the bottom-right quarter minus one source cell (the region the dyadic logits hand to a stuff class)."""
    return [(0, (0, max(Ho // 5, 1), 0, Wo), 0.9),                                    # top border, full width
            (2, (Ho // 5, Ho, 0, Wo), 0.5),                                           # stuff background below it
            (1, (Ho // 4, Ho, 0, max(Wo // 8, 1)), 0.85),                             # left + bottom border, inside the tie third
            (0, (Ho // 3, Ho // 2, Wo - max(Wo // 6, 1), Wo), 0.8),                   # right border
            (1, (Ho - max(Ho // 8, 1), Ho, Wo // 4, Wo // 2), 0.7),                   # bottom border
            (0, (Ho * 11 // 16, Ho * 14 // 16, Wo * 10 // 16, Wo * 14 // 16), 0.95),  # inside the stuff quarter
            (3, (Ho // 4, Ho // 3, Wo // 4, Wo // 2), 0.4)]                           # a second stuff segment


def _filter_frames(size, logits_of, seeds):
    segs, infos, sems = [], [], []
    for k, seed in enumerate(seeds):
        layout = _filter_layout(*size)
        if k % 2:
            layout = layout[::-1]              # other segment ids, other overlaps
        seg, info = R.hand_frame(size[0], size[1], layout, R.T_SEM)
        segs.append(seg)
        infos.append(info)
        sems.append(logits_of(seed))
    seg, info, sem = np.stack(segs), np.stack(infos), np.stack(sems)
    nseg = np.full((len(seeds),), len(_filter_layout(*size)), dtype=np.int32)
    return seg, info, nseg, sem


@pytest.mark.parametrize('case', R.DYADIC_CASES)
def test_filter_on_exact(vkn, case):
    (hs, ws), size, seed = case
    seg, info, nseg, sem = _filter_frames(size, lambda s: R.dyadic_logits(R.CS, hs, ws, s, R.T_SEM), (seed, seed + 100))
    dev = [torch.from_numpy(a).to(DEV) for a in (seg, info, nseg, sem)]
    got, _ = call_boxes(vkn, *dev, R.T_SEM)
    thing = np.stack([R.semantic_thing(sem[b], size, R.T_SEM)[0] for b in range(len(sem))])
    assert np.array_equal(got['thing_mask'], thing.astype(np.uint8))
    check_against_helper(got, seg, info, R.T_SEM, thing)
    # ties between a thing and a stuff channel resolve to the lower channel, the thing
    for b in range(len(sem)):
        up = torch.nn.functional.interpolate(torch.from_numpy(sem[b]).double()[None], size, mode='bilinear', align_corners=False)[0].numpy()
        top = up.max(0)
        tie = ((up[0] == top) & (up[R.T_SEM] == top)) | ((up[R.T_SEM - 1] == top) & (up[R.CS - 1] == top))
        assert tie.mean() > 0.2 and (got['thing_mask'][b][tie] == 1).all()
    # the segment inside the stuff quarter is emptied by the filter: unitrack's empty box, and it still counts
    b = 0
    sid = 6
    assert not thing[b][seg[b] == sid].any() and (seg[b] == sid).any()
    slot = got['segid'][b].tolist().index(sid)
    assert got['det'][b, slot, :4].tolist() == [-1.0, -1.0, 10.0, 10.0] and slot < got['count'][b]
    assert int(got['count'][b]) == 5
    # borders: the segments reach row / column 0 and the last row / column
    d = R.track_boxes(seg[b], info[b], R.T_SEM)['det']                     # (a condition on the inputs: the unfiltered segments)
    assert d[:, 0].min() == 0 and d[:, 1].min() == 0 and d[:, 2].max() == size[1] - 1 and d[:, 3].max() == size[0] - 1
    # without the thing_mask output the filter is evaluated on thing-segment pixels only: the same entries
    got2, _ = call_boxes(vkn, *dev, R.T_SEM, want_mask=False)
    for name in ('det', 'labels', 'rows', 'segid', 'count'):
        assert np.array_equal(got2[name].view(np.int32) if name == 'det' else got2[name],
                              got[name].view(np.int32) if name == 'det' else got[name]), name


@pytest.mark.parametrize('case', R.NONDYADIC_CASES)
def test_filter_on_nondyadic(vkn, case):
    (hs, ws), size, seed = case
    seg, info, nseg, sem = _filter_frames(size, lambda s: R.float_logits(R.CS, hs, ws, s), (seed,))
    dev = [torch.from_numpy(a).to(DEV) for a in (seg, info, nseg, sem)]
    got, _ = call_boxes(vkn, *dev, R.T_SEM)
    thing, margin = R.semantic_thing(sem[0], size, R.T_SEM, torch.float64)
    decided = margin >= R.MARGIN
    assert (~decided).mean() <= R.NEAR_TIE_CAP                                   # a condition on the inputs
    assert np.array_equal(got['thing_mask'][0][decided], thing.astype(np.uint8)[decided])
    assert set(np.unique(got['thing_mask'])) <= {0, 1}
    check_against_helper(got, seg, info, R.T_SEM, got['thing_mask'].astype(bool))   # boxes of the device's OWN mask, bit for bit


# ---------------------------------------------------------------------------------------------------- 4. maps
def _ids_cases(counts, D):
    """Per-frame (ids row [D], n_ids) sets: some -1, n_ids < count, n_ids = 0; rows beyond n_ids hold a value that must not show."""
    rng = np.random.RandomState(3)
    for mode in ('all', 'short', 'none'):
        ids = np.full((len(counts), D), 777, dtype=np.int64)
        n_ids = np.zeros((len(counts),), dtype=np.int32)
        for b, c in enumerate(counts):
            n = {'all': c, 'short': c // 2, 'none': 0}[mode]
            row = rng.randint(0, 40, size=n)
            row[::3] = -1                                                        # unmatched detections
            if n > 1:
                row[1] = -2                                                      # ids + 1 == -1 -> 0 (:592)
            ids[b, :n] = row
            n_ids[b] = n
        yield ids, n_ids


@pytest.mark.parametrize('kitti', [False, True])
@pytest.mark.parametrize('size,B', MAP_CASES)
def test_maps(vkn, size, B, kitti):
    tt = import_module('video_k_net_amd.track_tail')
    seg, info, nseg, _ = pan_maps(vkn, size, B)
    n_stuff = 17 if kitti else NSTUFF                                            # KITTI-STEP's table has 19 rows; labels < T + NSTUFF use it
    table = torch.tensor(tt.sem_of_label(T, n_stuff, kitti), dtype=torch.int32, device=DEV)
    _, boxes = call_boxes(vkn, seg, info, nseg, None, T, want_mask=False)
    seg_h, info_h = seg.cpu().numpy(), info.cpu().numpy()
    counts = boxes['count'].cpu().numpy().tolist()
    want_sem = np.stack([R.semantic_map(seg_h[b], info_h[b], T, n_stuff, kitti) for b in range(len(counts))])
    D = 16
    for ids, n_ids in _ids_cases(counts, D):
        tm, sm = call_maps(vkn, seg, boxes['segid'], boxes['count'], torch.from_numpy(ids).to(DEV), torch.from_numpy(n_ids).to(DEV), info, table)
        assert np.array_equal(sm, want_sem)
        for b in range(len(counts)):
            assert np.array_equal(tm[b], R.track_map(seg_h[b], info_h[b], T, ids[b, :n_ids[b]])), (b, n_ids[b])
        assert not (tm == 778).any()
    if B == 'special':
        assert counts[0] == 0 and counts[2] == 0 and not sm[0].any() and sm[2].any()


# ---------------------------------------------------------------------------------------------------- 5. arguments
def test_arguments_are_refused_before_any_launch(vkn):
    L = vkn._lib.lib()
    seg, info, nseg, _ = pan_maps(vkn, SHAPES[0], 1)
    B, Ho, Wo = seg.shape
    outs = dict(det=Guarded((B, K, 5), torch.float32), labels=Guarded((B, K), torch.int64), rows=Guarded((B, K), torch.int32),
                segid=Guarded((B, K), torch.int32), count=Guarded((B,), torch.int32), tm=Guarded((B, Ho, Wo), torch.uint8),
                tmap=Guarded((B, Ho, Wo), torch.int32), smap=Guarded((B, Ho, Wo), torch.int32))
    ws = _ws(1 << 16)
    sem = torch.zeros((B, 5, 4, 8), device=DEV)
    ids = torch.zeros((B, 16), dtype=torch.int64, device=DEV)
    n_ids = torch.zeros((B,), dtype=torch.int32, device=DEV)
    table = torch.zeros((T + NSTUFF,), dtype=torch.int32, device=DEV)
    segid = torch.zeros((B, K), dtype=torch.int32, device=DEV)
    count = torch.zeros((B,), dtype=torch.int32, device=DEV)
    host = torch.zeros((B * Ho * Wo,), dtype=torch.int32)                       # a CPU tensor's memory

    def boxes(**kw):
        a = dict(seg=seg.data_ptr(), info=info.data_ptr(), nseg=nseg.data_ptr(), sem=sem.data_ptr(), K=K, det=outs['det'].t.data_ptr(),
                 labels=outs['labels'].t.data_ptr(), rows=outs['rows'].t.data_ptr(), segid=outs['segid'].t.data_ptr(),
                 count=outs['count'].t.data_ptr(), tm=outs['tm'].t.data_ptr())
        a.update(kw)
        return L.vkn_track_boxes_f32(a['seg'], a['info'], a['nseg'], a['sem'], 5, 4, 8, T, B, a['K'], Ho, Wo, a['det'], a['labels'], a['rows'],
                                     a['segid'], a['count'], a['tm'], _p(ws), ws.numel(), None)

    def maps(**kw):
        a = dict(seg=seg.data_ptr(), segid=segid.data_ptr(), count=count.data_ptr(), ids=ids.data_ptr(), n_ids=n_ids.data_ptr(),
                 info=info.data_ptr(), table=table.data_ptr(), K=K, tmap=outs['tmap'].t.data_ptr(), smap=outs['smap'].t.data_ptr())
        a.update(kw)
        return L.vkn_track_maps_i32(a['seg'], a['segid'], a['count'], a['ids'], a['n_ids'], 16, a['info'], a['table'], T + NSTUFF, B, a['K'],
                                    Ho, Wo, a['tmap'], a['smap'], _p(ws), ws.numel(), None)

    for name in ('seg', 'info', 'nseg', 'det', 'labels', 'rows', 'segid', 'count'):
        assert boxes(**{name: None}) == E_ARG, name
        assert boxes(**{name: host.data_ptr()}) == E_ARG, name                  # host memory
    assert boxes(sem=host.data_ptr()) == E_ARG and boxes(tm=host.data_ptr()) == E_ARG
    for name in ('seg', 'segid', 'count', 'ids', 'n_ids', 'info', 'table', 'tmap', 'smap'):
        assert maps(**{name: None}) == E_ARG, name
        assert maps(**{name: host.data_ptr()}) == E_ARG, name
    cap = vkn._lib.TRACK_MAX_K
    assert boxes(K=cap + 1) == E_SHAPE and maps(K=cap + 1) == E_SHAPE
    for name, t in (('seg', seg), ('info', info), ('sem', sem), ('det', outs['det'].t), ('labels', outs['labels'].t), ('rows', outs['rows'].t),
                    ('segid', outs['segid'].t), ('tm', outs['tm'].t)):
        assert boxes(**{name: t.data_ptr() + 4}) == E_ALIGN, name
    for name, t in (('seg', seg), ('segid', segid), ('ids', ids), ('info', info), ('tmap', outs['tmap'].t), ('smap', outs['smap'].t)):
        assert maps(**{name: t.data_ptr() + 4}) == E_ALIGN, name
    torch.cuda.synchronize()
    for name, g in outs.items():
        assert g.untouched(), name
    assert torch.cuda.is_available() and int(torch.zeros(1, device=DEV).item()) == 0     # the device is healthy: nothing was launched on bad pointers


def test_repeated_segment_id_keeps_the_first_entry(vkn):
    """vkn_panoptic_joint_f32 never repeats a segment id; if `info` does, the first entry is the entry and every row below count is written."""
    layout = [(0, (0, 3, 0, 4), 0.9), (2, (3, 7, 0, 9), 0.5), (1, (1, 6, 5, 9), 0.7)]
    seg, info = R.hand_frame(7, 9, layout, T)
    info = np.concatenate([info, info[:1]])                  # the first row once more, behind the rejected entry
    info[-1, 0], info[-1, 1] = 55, 0                         # (another mask row and label: it must not show)
    dev = [torch.from_numpy(a).to(DEV) for a in (seg[None], info[None], np.asarray([3], dtype=np.int32))]
    got, _ = call_boxes(vkn, *dev, None, T)
    check_against_helper(got, seg[None], info[None, :-1], T)
    assert int(got['count'][0]) == 2 and 55 not in got['rows'][0]


# ---------------------------------------------------------------------------------------------------- the tracker's device count
def _trk(vkn):
    return vkn.QuasiDenseEmbedTracker(init_score_thr=0.8, obj_score_thr=0.5, match_score_thr=0.5, max_dets=16, max_tracklets=32)


def _trk_inputs(rows, seed):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand((rows, 2), generator=g) * 80
    wh = 5 + torch.rand((rows, 2), generator=g) * 20
    score = 0.55 + 0.4 * torch.rand((rows, 1), generator=g)
    return (torch.cat([xy, xy + wh, score], 1).to(DEV), torch.randint(0, 2, (rows,), generator=g).to(DEV),
            (torch.randn((rows, 16), generator=g) * 3).to(DEV))


def _live_state(trk):
    """The live part of the device memo (the state buffer is allocated uninitialised: rows beyond the counts are dead data): header,
    tracklets and backdrops, floats as bit patterns."""
    bits = lambda t: t.contiguous().view(torch.int32).tolist()  # noqa: E731
    tr = [(i, t['label'], t['last_frame'], t['acc_frame'], bits(t['bbox']), bits(t['velocity']), bits(t['embed']))
          for i, t in trk.tracklets.items()]
    bd = [(bits(b['bboxes']), bits(b['embeds']), b['labels'].tolist()) for b in trk.backdrops]
    return trk._header()[:6], tr, bd


@pytest.mark.parametrize('count', [5, 8, 100])
def test_tracker_device_count_equals_host_count(vkn, count):
    """vkn_qd_tracker_match_dev_f32 with n = min(*n_dev, n_max) == vkn_qd_tracker_match_f32 with that n on the host: outputs and the
    live state, bit for bit, over two frames (rows beyond the count are never read; a count above n_max is clamped)."""
    a, b = _trk(vkn), _trk(vkn)
    n = min(count, 8)
    for fid in range(2):
        bb, lb, em = _trk_inputs(8, 40 + fid)
        ct = torch.tensor([count], dtype=torch.int32, device=DEV)
        ob, ol, oi, oc = a.match_padded(bb, lb, em, fid, count=ct)
        wb, wl, wi, wc = b.match_padded(bb[:n], lb[:n], em[:n], fid)
        torch.cuda.synchronize()
        k = int(wc[0])
        assert oc.tolist() == wc.tolist() and k > 0
        assert torch.equal(ob[:k], wb[:k]) and torch.equal(ol[:k], wl[:k]) and torch.equal(oi[:k], wi[:k])
        assert _live_state(a) == _live_state(b)
    assert a.num_tracklets > 0


def test_tracker_device_count_zero_is_no_call(vkn):
    a = _trk(vkn)
    bb, lb, em = _trk_inputs(8, 50)
    a.match_padded(bb, lb, em, 0)
    before = a._state.clone()
    _, _, _, oc = a.match_padded(bb, lb, em, 1, count=torch.zeros(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert oc.tolist() == [0, 0] and torch.equal(before, a._state)
    with pytest.raises(vkn.VknLibraryError):
        a.match_padded(bb, lb, em, 2, count=torch.zeros(1, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------- 6. TrackTail end to end
N_E2E, C_E2E, H_E2E, W_E2E, NP_E2E = 8, 64, 16, 32, 6


def _e2e_frame(shift, things=True):
    """cls_prob [1, 8, 4], mask logits [1, 8, 16, 32]: six thing kernels on a 2 x 3 grid of 4 x 6 rectangles (moved right by `shift`;
    `things=False`: none of them reaches probability 0.5), two
    stuff kernels as the upper / lower half."""
    cls = torch.full((1, N_E2E, T + 2), 0.05)
    logits = torch.full((1, N_E2E, H_E2E, W_E2E), -6.0)
    for i in range(NP_E2E):
        cls[0, i, i % T] = 0.95 - 0.01 * i
        y0, x0 = 1 + 8 * (i // 3), 1 + 10 * (i % 3) + shift
        logits[0, i, y0:y0 + 4, x0:x0 + 6] = 6.0
    for j in range(2):
        cls[0, NP_E2E + j, T + j] = 0.9
        logits[0, NP_E2E + j, 8 * j:8 * j + 8] = 2.0
    if not things:
        logits[0, :NP_E2E] = -20.0
    return cls, logits


def _e2e_panoptic(vkn, cls, logits):
    size = (H_E2E, W_E2E)
    return vkn.ops.panoptic_joint(cls.to(DEV), logits.to(DEV), NP_E2E, T, NP_E2E, PAN_CFG['instance_score_thr'], PAN_CFG['overlap_thr'],
                                  size, size, size, upsample_stride=1, want_bbox=True)


@pytest.mark.parametrize('kitti', [False, True])
def test_track_tail_end_to_end(vkn, kitti):
    tt = import_module('video_k_net_amd.track_tail')
    n_stuff = 17 if kitti else 2
    g = torch.Generator().manual_seed(7)
    head = vkn.QuasiDenseMaskEmbedHeadGTMask(num_convs=0, num_fcs=1, roi_feat_size=1, in_channels=C_E2E, fc_out_channels=64, embed_channels=32,
                                             loss_track_aux=None)
    with torch.no_grad():
        for p in head.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.2)
    head = head.to(DEV).eval()
    kw = dict(init_score_thr=0.8, obj_score_thr=0.5, match_score_thr=0.5, memo_tracklet_frames=10, memo_backdrop_frames=1,
              memo_momentum=0.8, nms_conf_thr=0.5, nms_backdrop_iou_thr=0.3, nms_class_iou_thr=0.7, with_cats=True,
              match_metric='bisoftmax', max_dets=32, max_tracklets=64)
    trk_dev, trk_host = vkn.QuasiDenseEmbedTracker(**kw), vkn.QuasiDenseEmbedTracker(**kw)
    tail = tt.TrackTail(T, n_stuff, semantic_filter=True, kitti_step=kitti, tracker=trk_dev, track_head=head)
    obj = (torch.randn((1, N_E2E, C_E2E), generator=g) * 4.0).to(DEV)
    # dyadic semantic logits (4 x 8 -> 16 x 32, scale 4): the filter is exact in fp32
    sem = torch.from_numpy(R.dyadic_logits(R.CS, 4, 8, 31, T))[None]
    thing = R.semantic_thing(sem[0].numpy(), (H_E2E, W_E2E), T)[0]
    KIH = import_module('video_k_net_amd.kernel_iter_head').KernelIterHead
    head_like = type('H', (), dict(num_thing_classes=T))()
    seen_ids = []
    for fid, shift in enumerate((0, 1)):
        seg, info, nseg, bbox = _e2e_panoptic(vkn, *_e2e_frame(shift))
        feats = obj + 0.01 * fid
        sm, tm, det, ids = tail(seg, info, nseg, sem.to(DEV), feats, fid)
        torch.cuda.synchronize()
        # the host path: things_for_tracking + the helper's filter + tracker.match + the helper's maps
        seg_h, info_h, bbox_h = seg[0].cpu().numpy(), info[0].cpu().numpy(), bbox[0].cpu().numpy()
        acc, labels, _, scores = KIH.things_for_tracking(head_like, info_h, bbox_h)
        want = R.track_boxes(seg_h, info_h, T, thing)
        assert len(acc) == NP_E2E and want['labels'].tolist() == labels
        assert np.array_equal(want['det'][:, 4], np.asarray(scores, dtype=np.float32))
        rows = torch.from_numpy(want['rows']).long().to(DEV)
        emb = head(feats[0].index_select(0, rows))
        _, _, ids_h = trk_host.match(torch.from_numpy(want['det']).to(DEV), torch.from_numpy(want['labels']).to(DEV), emb, fid)
        n = int(tail.last['n_ids'][0])
        assert n == len(ids_h) and int(tail.last['count'][0]) == NP_E2E
        assert ids[0, :n].cpu().tolist() == ids_h.tolist() and (ids[0, n:] == -2).all()
        assert np.array_equal(det[0, :NP_E2E].cpu().numpy().view(np.int32), want['det'].view(np.int32))
        assert np.array_equal(tm[0].cpu().numpy(), R.track_map(seg_h, info_h, T, ids_h.tolist()))
        assert np.array_equal(sm[0].cpu().numpy(), R.semantic_map(seg_h, info_h, T, n_stuff, kitti))
        assert tm.dtype == torch.int32 and sm.dtype == torch.int32 and tm.is_cuda and sm.is_cuda and det.is_cuda and ids.is_cuda
        seen_ids.append(ids_h.tolist())
    assert max(seen_ids[0]) >= 0 and set(i for i in seen_ids[1] if i >= 0) & set(seen_ids[0])      # tracks are born, then found again
    # a frame without things: not a tracker call — zero track map, tracker state bit-identical
    before = trk_dev._state.clone()
    seg, info, nseg, _ = _e2e_panoptic(vkn, *_e2e_frame(0, things=False))
    sm, tm, det, ids = tail(seg, info, nseg, sem.to(DEV), obj, 2)
    torch.cuda.synchronize()
    assert int(tail.last['count'][0]) == 0 and int(tail.last['n_ids'][0]) == 0 and int(nseg[0]) == 2
    assert not tm.any() and not det.any() and (ids == -2).all() and sm.any()
    assert torch.equal(before, trk_dev._state)
    with pytest.raises(vkn.VknLibraryError):
        tail(seg.cpu(), info, nseg, sem, obj, 3)
    with pytest.raises(vkn.VknLibraryError):
        vkn.ops.track_boxes(seg.cpu(), info.cpu(), nseg.cpu(), T)
    with pytest.raises(vkn.VknLibraryError):
        vkn.ops.track_maps(seg.cpu(), info, nseg, ids, nseg, info, nseg)
