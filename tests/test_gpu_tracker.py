"""GPU (-m gpu): the device-side quasi-dense association (`vkn_qd_tracker_match_f32`, one single-workgroup kernel per frame over a
device-resident memo) against the reference's own tracker (tests/golden/qd_tracker.npz, bit-exact ids / labels / boxes) and, on
videos far larger than the goldens, against the CPU oracle (oracle/tracker_oracle.py, itself pinned to the same goldens)."""
import os

import numpy as np
import pytest
import torch

import tracker_edge_cases as TC
from helpers import GOLDEN
from oracle import synth
from oracle.tracker_oracle import TrackerOracle, random_video

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CFG = dict(init_score_thr=0.35, obj_score_thr=0.3, match_score_thr=0.5, memo_tracklet_frames=5, memo_backdrop_frames=1,
           memo_momentum=0.8, nms_conf_thr=0.5, nms_backdrop_iou_thr=0.3, nms_class_iou_thr=0.7, with_cats=True)


def _step(trk, bb, lab, em, t):
    return trk.match(torch.from_numpy(bb).to(DEV), torch.from_numpy(lab).to(DEV), torch.from_numpy(em).to(DEV), t)


@pytest.mark.parametrize('name', ['trk_a', 'trk_b', 'trk_c', 'trk_d'])
def test_tracker_ids_bit_exact_vs_reference(vkn, name):
    g = dict(np.load(os.path.join(GOLDEN, 'qd_tracker.npz'), allow_pickle=False))
    T, n_obj, emb, n_cls, seed = (int(v) for v in g[name + '_case'])
    trk = vkn.build_tracker(dict(CFG, type='QuasiDenseEmbedTracker', match_metric=str(g[name + '_metric'])))
    for t, (bb, lab, em, _) in enumerate(synth.tracker_sequence(T, n_obj, emb, n_cls, seed)):
        b, l_, ids = _step(trk, bb, lab, em, t)
        assert not ids.is_cuda and ids.dtype == torch.int64
        assert np.array_equal(ids.numpy(), g[f'{name}_ids{t}']), (name, t)
        assert np.array_equal(l_.cpu().numpy(), g[f'{name}_labels{t}']) and np.array_equal(b.cpu().numpy(), g[f'{name}_bboxes{t}'])
    assert trk.num_tracklets == int(max(g[f'{name}_ids{t}'].max() for t in range(T))) + 1


@pytest.mark.parametrize('metric', ['bisoftmax', 'softmax', 'cosine'])
@pytest.mark.parametrize('bd_frames', [0, 1, 3])
def test_tracker_vs_oracle_on_dense_videos(vkn, metric, bd_frames):
    """120 objects, 256-d embeddings, 14 frames, tracks expiring after 3 unseen frames: every per-frame decision (survivors, ids),
    and at the end the whole memo (track table in creation order, momentum embeddings, velocities, backdrops)."""
    cfg = dict(CFG, match_metric=metric, memo_backdrop_frames=bd_frames, memo_tracklet_frames=3, init_score_thr=0.5, obj_score_thr=0.35)
    trk = vkn.build_tracker(dict(cfg, type='QuasiDenseEmbedTracker', max_tracklets=1024))
    ora = TrackerOracle(**cfg)
    for t, (bb, lab, em) in enumerate(random_video(14, 120, 256, 4, 7 + bd_frames)):
        b, l_, ids = _step(trk, bb, lab, em, t)
        rb, rl, rids = ora.step(torch.from_numpy(bb), torch.from_numpy(lab), torch.from_numpy(em), t)
        assert np.array_equal(b.cpu().numpy(), rb.numpy()) and np.array_equal(l_.cpu().numpy(), rl.numpy()), t
        assert np.array_equal(ids.numpy(), rids.numpy()), (t, np.nonzero(ids.numpy() != rids.numpy()))
    tr = trk.tracklets
    assert list(tr) == ora.t_id and trk.num_tracklets == ora.next_id
    for i, tid in enumerate(ora.t_id):
        e = tr[tid]
        assert e['last_frame'] == ora.t_last[i] and e['acc_frame'] == ora.t_acc[i] and e['label'] == int(ora.t_label[i])
        assert torch.equal(e['bbox'], ora.t_box[i])
        assert float((e['embed'] - ora.t_emb[i]).abs().max()) == 0.0, 'momentum embedding: same fp32 operation sequence'
        assert float((e['velocity'] - ora.t_vel[i]).abs().max()) < 1e-6
    bds = trk.backdrops
    assert len(bds) == len(ora.backdrops)
    for a, r in zip(bds, ora.backdrops):
        assert torch.equal(a['bboxes'], r['box']) and torch.equal(a['embeds'], r['emb']) and torch.equal(a['labels'].long(), r['label'])


def test_tracker_padded_api_and_edge_cases(vkn):
    trk = vkn.build_tracker(dict(CFG, type='QuasiDenseEmbedTracker', max_dets=64, max_tracklets=8))
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    b, l_, ids = trk.match(z(0, 5), z(0, dt=torch.long), z(0, 32), 0)                      # an empty frame
    assert b.shape == (0, 5) and ids.numel() == 0 and trk.empty
    bb, lab, em = random_video(1, 40, 32, 2, 3)[0]
    ob, ol, oi, cnt = trk.match_padded(torch.from_numpy(bb).to(DEV), torch.from_numpy(lab).to(DEV), torch.from_numpy(em).to(DEV), 1)
    assert ob.shape == (64, 5) and cnt.dtype == torch.int32 and oi.is_cuda
    k, status = cnt.cpu().tolist()
    assert 0 < k <= bb.shape[0]
    assert status == 1, 'more births than max_tracklets = 8: reported, not silently dropped'
    with pytest.raises(RuntimeError):
        trk.match(torch.from_numpy(bb).to(DEV), torch.from_numpy(lab).to(DEV), torch.from_numpy(em).to(DEV), 2)
    trk.reset()
    assert trk.empty and trk.num_tracklets == 0
    with pytest.raises(ValueError):
        trk.match(z(65, 5), z(65, dt=torch.long), z(65, 32), 0)


# ==================================================================================================== decision edges and capacities
class DeviceRunner:
    """`step` / `tracklets` / `backdrops` of tests/tracker_edge_cases.check_case over the device tracker.  `padded`: through
    `match_padded(..., count=...)` with the inputs padded to max_dets rows that would win every decision if they were read."""

    def __init__(self, vkn, cfg, caps, padded=False):
        self.trk = vkn.build_tracker(dict(cfg, type='QuasiDenseEmbedTracker', **caps))
        self.padded, self.status = padded, []

    def step(self, bb, lab, em, fid):
        if not self.padded:
            b, l_, ids = _step(self.trk, bb, lab, em, fid)
            return b.cpu().numpy(), l_.cpu().numpy(), ids.numpy()
        n, D = bb.shape[0], self.trk.max_dets
        pad_b = np.tile(np.asarray([[0, 0, 1000, 1000, 0.984375]], dtype=np.float32), (D - n, 1))
        bb, lab, em = np.concatenate([bb, pad_b]), np.concatenate([lab, np.zeros(D - n, np.int64)]), np.concatenate([em, np.ones((D - n, em.shape[1]), np.float32)])
        ob, ol, oi, cnt = self.trk.match_padded(torch.from_numpy(bb).to(DEV), torch.from_numpy(lab).to(DEV), torch.from_numpy(em).to(DEV), fid,
                                                count=torch.tensor([n], dtype=torch.int32, device=DEV))
        k, status = cnt.cpu().tolist()
        self.status.append(status)
        return ob[:k].cpu().numpy(), ol[:k].cpu().numpy(), oi[:k].cpu().numpy()

    def tracklets(self):
        return [dict(id=i, label=e['label'], last=e['last_frame'], acc=e['acc_frame'], box=e['bbox'].numpy(), vel=e['velocity'].numpy(),
                     emb=e['embed'].numpy()) for i, e in self.trk.tracklets.items()]

    def backdrops(self):
        return [dict(box=f['bboxes'].numpy(), emb=f['embeds'].numpy(), label=f['labels'].numpy()) for f in self.trk.backdrops]


@pytest.mark.parametrize('name', list(TC.CASES))
def test_tracker_decision_edges(vkn, name):
    """Every hand-made video of tests/tracker_edge_cases.py: the kernel's ids, labels, survivors, tracklet table and backdrop ring equal
    the hand-stated outcome (which the oracle and, where it can run the case, the reference's own class give as well)."""
    c = TC.CASES[name]
    TC.check_case(c, DeviceRunner(vkn, c['cfg'], c['caps']), twin=TC.OracleRunner(c['cfg']))


@pytest.mark.parametrize('name', TC.PADDED_CASES)
def test_tracker_decision_edges_through_the_device_count_entry(vkn, name):
    c = TC.CASES[name]
    run = DeviceRunner(vkn, c['cfg'], c['caps'], padded=True)
    TC.check_case(c, run)
    assert run.status == [0] * len(c['frames'])


def _against_oracle(trk, ora, video, frame_ids=None):
    """ids, labels, boxes per frame and the whole memo at the end, as test_tracker_vs_oracle_on_dense_videos"""
    for t, (bb, lab, em) in enumerate(video):
        fid = t if frame_ids is None else frame_ids[t]
        b, l_, ids = _step(trk, bb, lab, em, fid)
        rb, rl, rids = ora.step(torch.from_numpy(bb), torch.from_numpy(lab), torch.from_numpy(em), fid)
        assert np.array_equal(b.cpu().numpy(), rb.numpy()) and np.array_equal(l_.cpu().numpy(), rl.numpy()), t
        assert np.array_equal(ids.numpy(), rids.numpy()), (t, np.nonzero(ids.numpy() != rids.numpy()))
    tr = trk.tracklets
    assert list(tr) == ora.t_id and trk.num_tracklets == ora.next_id
    for i, tid in enumerate(ora.t_id):
        e = tr[tid]
        assert e['last_frame'] == ora.t_last[i] and e['acc_frame'] == ora.t_acc[i] and e['label'] == int(ora.t_label[i])
        assert torch.equal(e['bbox'], ora.t_box[i])
        assert float((e['embed'] - ora.t_emb[i]).abs().max()) == 0.0, 'momentum embedding: same fp32 operation sequence'
        assert float((e['velocity'] - ora.t_vel[i]).abs().max()) < 1e-6
    bds = trk.backdrops
    assert len(bds) == len(ora.backdrops)
    for a, r in zip(bds, ora.backdrops):
        assert torch.equal(a['bboxes'], r['box']) and torch.equal(a['embeds'], r['emb']) and torch.equal(a['labels'].long(), r['label'])


@pytest.mark.parametrize('name', list(TC.SWEEPS))
def test_tracker_capacity_and_configuration_sweeps(vkn, name):
    """max_dets detections in one frame, a memo of more than 1024 columns (the second step of the 1024-thread strides), embedding
    widths 1 / 3 / 1024, with_cats=False and other momenta: against the oracle (tests/test_tracker_edge_cases.py shows on the CPU
    that each sweep reaches the capacity it is about)."""
    s = TC.SWEEPS[name]
    trk = vkn.build_tracker(dict(s['cfg'], type='QuasiDenseEmbedTracker', **s['caps']))
    _against_oracle(trk, TrackerOracle(**s['cfg']), s['video']())
    assert trk.status == 0


def test_tracker_table_exactly_full(vkn):
    """max_tracklets == the births of the video: status 0 to the last row.  One birth more: that frame reports status 1, returns
    the oracle's ids (the id is consumed) and the table stays full; after reset() the tracker reproduces the first video."""
    frames, extra = TC.full_table_video()
    ref = TrackerOracle(**TC.FULL_CFG)
    want = [ref.step(torch.from_numpy(bb), torch.from_numpy(lab), torch.from_numpy(em), t)[2].tolist() for t, (bb, lab, em) in enumerate(frames)]
    T = ref.next_id
    assert len(ref.t_id) == T
    run = DeviceRunner(vkn, TC.FULL_CFG, dict(max_dets=32, max_tracklets=T), padded=True)
    for again in (False, True):
        for t, (bb, lab, em) in enumerate(frames):
            assert run.step(bb, lab, em, t)[2].tolist() == want[t], (again, t)
        assert run.status == [0] * len(frames) and run.trk.num_tracklets == T and [r['id'] for r in run.tracklets()] == ref.t_id[:T]
        if not again:
            ids = run.step(*extra, len(frames))[2].tolist()
            assert ids == ref.step(*(torch.from_numpy(x) for x in extra), len(frames))[2].tolist() == [T]
            assert run.status[-1] == 1 and run.trk.status == 1 and run.trk.num_tracklets == T + 1
            assert [r['id'] for r in run.tracklets()] == ref.t_id[:T], 'the dropped birth wrote nothing'
            run.trk.reset()
            run.status = []


def test_tracker_full_table_is_tested_before_expiry(vkn):
    """A birth and an expiry in one frame with the table full: the capacity test runs before the expiry compaction, so the birth is
    dropped (include/vkn_track.h); the freed row serves the next frame."""
    fe = TC.FULL_EXPIRY
    run = DeviceRunner(vkn, fe['cfg'], fe['caps'], padded=True)
    ins = TC.inputs(dict(frames=fe['frames'], frame_ids=range(len(fe['frames']))))
    for (fid, bb, lab, em), (ids, status, live, handed) in zip(ins, fe['expect']):
        assert run.step(bb, lab, em, fid)[2].tolist() == ids, fid
        assert run.status[-1] == status and [r['id'] for r in run.tracklets()] == live and run.trk.num_tracklets == handed, fid


def test_tracker_bit_exact_vs_reference_on_the_other_axes(vkn):
    """tests/golden/qd_tracker_edges.npz: with_cats=False, memo_momentum=0.3, three backdrop frames, cosine with frame gaps — ids,
    labels and boxes of the reference's own tracker class."""
    import json
    g = dict(np.load(os.path.join(GOLDEN, 'qd_tracker_edges.npz'), allow_pickle=False))
    for name in (str(n) for n in g['video_names']):
        T, n_obj, emb, n_cls, seed = (int(v) for v in g[name + '_case'])
        fids = g[name + '_frame_ids'].tolist()
        trk = vkn.build_tracker(dict(json.loads(str(g[name + '_cfg'])), type='QuasiDenseEmbedTracker'))
        for t, (bb, lab, em, _) in enumerate(synth.tracker_sequence(T, n_obj, emb, n_cls, seed)):
            b, l_, ids = _step(trk, bb, lab, em, fids[t])
            assert np.array_equal(ids.numpy(), g[f'{name}_ids{t}']), (name, t)
            assert np.array_equal(l_.cpu().numpy(), g[f'{name}_labels{t}']) and np.array_equal(b.cpu().numpy(), g[f'{name}_bboxes{t}'])
