"""The hand-made tracker videos of tests/tracker_edge_cases.py checked on their own, without a GPU: the oracle
(oracle/tracker_oracle.py) gives every hand-stated outcome, the reference's own class gave the same (tests/golden/qd_tracker_edges.npz,
oracle/gen_golden_tracker.py), the inputs are exact where the cases say so, and the sweeps reach the capacities they are about.  Plus
what the C ABI promises about the number of backdrop frames before any launch.

Which case notices which one-character change of csrc/vkn_tracker.hip (each mutant was applied to the oracle's twin of the line):
  phase B  `score < obj_score_thr` -> `<=`            obj_b_at
  phase B  `iou > thr` -> `>=`                        iou_b_at                 (`>` -> against kept boxes only: suppressed_suppressor)
  phase E  `best > match_score_thr` -> `>=`           match_at, match_at_no_birth, taken_no_choice
  phase E  `score > obj_score_thr` -> `>=`            obj_e_at_conf_above, obj_e_at_conf_equal
  phase E  `best > nms_conf_thr` -> `>=`              obj_e_at_conf_equal
  phase F  `score > init_score_thr` -> `>=`           init_at, init_order, match_at_no_birth
  phase G  `iou > nms_backdrop_iou_thr` -> `>=`       iou_g_at
  phase G  `frame - last >= frames` -> `>`            expiry_ge, expiry_zero, expiry_compaction, birth_and_expiry
  phase E  `oj < bj` -> `oj > bj` / scan `>` -> `>=`  tie_other_lane_tracks, tie_other_lane_backdrop / tie_same_lane_tracks, tie_same_lane_backdrop
  phase D  the with_cats multiply dropped             cats_on
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import tracker_edge_cases as TC
from helpers import GOLDEN
from oracle.tracker_oracle import TrackerOracle, iou_matrix


@pytest.mark.parametrize('name', list(TC.CASES))
def test_oracle_gives_the_hand_stated_outcome(name):
    c = TC.CASES[name]
    TC.check_case(c, TC.OracleRunner(c['cfg']))


def test_every_required_decision_has_its_three_forms():
    """at the limit / one step above / one step below, per decision of the issue's list"""
    for stem in ('match', 'obj_b', 'iou_b', 'iou_g', 'init'):
        assert {f'{stem}_at', f'{stem}_above'} <= set(TC.CASES) and any(n.startswith(f'{stem}_below') for n in TC.CASES), stem
    assert {'obj_e_at_conf_above', 'obj_e_at_conf_equal', 'obj_e_above', 'obj_e_below'} <= set(TC.CASES)
    assert {f'ring_{f}' for f in (0, 1, 2, 64)} <= set(TC.CASES) and len(TC.CASES['ring_64']['frames']) == 66
    assert {f'momentum_{m}' for m in (0.0, 0.25, 1.0, 0.3)} <= set(TC.CASES)
    assert all(n in TC.CASES for n in TC.PADDED_CASES)


@pytest.mark.parametrize('name', list(TC.CASES))
def test_inputs_are_exact(name):
    """The exactness premise: integer boxes, scores on the 2^-6 grid, four unit entries per embedding, and every cosine a detection
    meets in the oracle's memo a multiple of 0.25 — the same float from the fp32 product and from float64."""
    c = TC.CASES[name]
    ora = TrackerOracle(**c['cfg'])
    dyadic_memo = c['cfg']['memo_momentum'] in (0.0, 0.25, 0.5, 1.0)
    for fid, bb, lab, em in TC.inputs(c):
        assert np.array_equal(bb[:, :4], np.round(bb[:, :4])) and np.array_equal(bb[:, 4] * 64, np.round(bb[:, 4] * 64))
        assert np.array_equal(np.abs(em), np.abs(em) ** 2) and (np.abs(em).sum(1) == 4).all()
        memo = list(ora.t_emb) + [r for f in ora.backdrops for r in f['emb']]
        if memo and dyadic_memo:
            f32, f64 = TC.cosines(em, torch.stack(memo))
            assert torch.equal(f32.double(), f64) and torch.equal(f64 * 4, torch.round(f64 * 4)), (name, fid)
        ora.step(torch.from_numpy(bb), torch.from_numpy(lab), torch.from_numpy(em), fid)
    if not dyadic_memo:
        assert name == 'momentum_0.3' and len(c['frames']) == 2, 'the one non-dyadic momentum: nothing is matched against its embedding'


def test_ious_at_a_limit_are_the_stated_fractions():
    for key, (pair, inter, union) in TC.IOU_PAIRS.items():
        a, b = (torch.tensor([p], dtype=torch.float32) for p in pair)
        assert float((a[0, 2] - a[0, 0]) * (a[0, 3] - a[0, 1])) == 6.0 == float((b[0, 2] - b[0, 0]) * (b[0, 3] - b[0, 1]))
        got = iou_matrix(a, b)[0, 0]
        assert got.dtype == torch.float32 and float(got) == float(np.float32(inter) / np.float32(union)), key
    assert float(iou_matrix(torch.tensor([TC.IOU_PAIRS['half'][0][0]], dtype=torch.float32),
                            torch.tensor([TC.IOU_PAIRS['half'][0][1]], dtype=torch.float32))) == 0.5
    assert TC.BELOW_HALF < 0.5 and float(np.float32(TC.BELOW_HALF)) == TC.BELOW_HALF
    assert float(np.nextafter(np.float32(TC.BELOW_HALF), np.float32(1))) == 0.5
    # the between-the-limits box of the obj_b cases and the suppressed suppressor's three overlaps
    assert 0.25 < 3 / 9 < 0.5
    a, b, c_ = (torch.tensor([d[0]], dtype=torch.float32) for d in (TC.CASES['suppressed_suppressor']['frames'][0][i] for i in (1, 2, 0)))
    assert float(iou_matrix(b, a)) == float(np.float32(24) / np.float32(40)) and float(iou_matrix(c_, b)) == float(np.float32(16) / np.float32(40))
    assert float(iou_matrix(c_, a)) == 0.0


# ---------------------------------------------------------------------------------------------------- the sweeps are not vacuous
def _oracle_run(cfg, video):
    ora, outs = TrackerOracle(**cfg), []
    for t, (bb, lab, em) in enumerate(video):
        outs.append(ora.step(torch.from_numpy(bb), torch.from_numpy(lab), torch.from_numpy(em), t))
    return ora, outs


def test_sweep_n256_fills_max_dets():
    s = TC.SWEEPS['n256']
    video = s['video']()
    ora, outs = _oracle_run(s['cfg'], video)
    assert all(bb.shape[0] == 256 == s['caps']['max_dets'] for bb, _, _ in video)
    assert all(b.shape[0] == 256 for b, _, _ in outs), 'boxes on a grid: every detection survives'
    assert any((ids >= 0).sum() > 50 and (ids == -1).sum() > 50 for _, _, ids in outs[1:])


def test_sweep_memo_exceeds_1024_entries_at_match_time():
    s = TC.SWEEPS['memo_over_1024']
    video = s['video']()
    ora = TrackerOracle(**s['cfg'])
    for t, (bb, lab, em) in enumerate(video):
        if t == len(video) - 1:
            m = len(ora.t_id) + sum(f['emb'].shape[0] for f in ora.backdrops)
            assert m > 1024 and len(ora.backdrops) == 2 and all(f['emb'].shape[0] > 0 for f in ora.backdrops), m
        _, _, ids = ora.step(torch.from_numpy(bb), torch.from_numpy(lab), torch.from_numpy(em), t)
        first = ora.next_id if t == 0 else first
    assert len(ora.t_id) <= s['caps']['max_tracklets'], 'the table is never overfilled'
    old = [i for i in ids.tolist() if 0 <= i < first]
    assert len(old) >= 8, 'the persistent objects still find their first-frame tracks among the > 1024 columns'


def test_sweeps_stay_inside_the_capacities():
    for name, s in TC.SWEEPS.items():
        video = s['video']()
        ora = TrackerOracle(**s['cfg'])
        peak = 0
        for t, (bb, lab, em) in enumerate(video):
            assert bb.shape[0] <= s['caps']['max_dets'], name
            ora.step(torch.from_numpy(bb), torch.from_numpy(lab), torch.from_numpy(em), t)
            peak = max(peak, len(ora.t_id))
        assert 0 < peak <= s['caps']['max_tracklets'], (name, peak)
    assert {TC.SWEEPS[f'embed_{e}_bisoftmax']['video']()[0][2].shape[1] for e in (1, 3, 1024)} == {1, 3, 1024}


def test_full_table_video_fills_the_table_exactly():
    frames, extra = TC.full_table_video()
    ora, outs = _oracle_run(TC.FULL_CFG, frames)
    assert len(ora.t_id) == ora.next_id >= 12, 'no expiry: live tracks == births'
    before = ora.next_id
    _, _, ids = ora.step(*(torch.from_numpy(x) for x in extra), len(frames))
    assert ids.tolist() == [before] and ora.next_id == before + 1, 'the extra frame is exactly one birth more'


# ---------------------------------------------------------------------------------------------------- the reference's own class
def test_reference_fixture_agrees_with_the_hand_stated_outcomes():
    g = dict(np.load(os.path.join(GOLDEN, 'qd_tracker_edges.npz'), allow_pickle=False))
    names = [n for n, c in TC.CASES.items() if c['reference']]
    assert sorted(str(n) for n in g['case_names']) == sorted(names)
    assert not any(TC.CASES[n]['reference'] for n in TC.CASES if n.startswith('equal_') or n.startswith('tie_same') or n == 'tie_other_lane_tracks'), \
        'rows with equal scores: the reference sorts them in an unspecified order'
    for n in names:
        c = TC.CASES[n]
        for t, ((fid, bb, lab, em), e) in enumerate(zip(TC.inputs(c), c['expect'])):
            assert g[f'case_{n}_ids{t}'].tolist() == e['ids'], (n, t)
            assert g[f'case_{n}_labels{t}'].tolist() == e['labels'], (n, t)
            assert np.array_equal(g[f'case_{n}_bboxes{t}'], bb[e['order']].reshape(-1, 5)), (n, t)


# ---------------------------------------------------------------------------------------------------- the ABI, before any launch
def test_backdrop_frame_count_is_bounded_before_any_launch(vkn):
    """memo_backdrop_frames <= 64 (VKN_TRACKER_MAX_BACKDROP_FRAMES): 65 passes every other gate (64 + 65 * 16 <= 4096), so this gate
    alone declines it — size queries 0, every entry VKN_E_SHAPE; checked on the host with fake pointers, nothing is launched."""
    L = vkn._lib.lib()
    assert vkn._lib.CONSTS['VKN_TRACKER_MAX_BACKDROP_FRAMES'] == 64
    p, off = 0x10000, (ctypes.c_size_t * 12)()

    def cfg_of(frames, embed_dim=16):
        return vkn.QuasiDenseEmbedTracker(max_dets=16, max_tracklets=64, memo_backdrop_frames=frames)._make_cfg(embed_dim)

    ok = cfg_of(64)
    nb, nw = L.vkn_qd_tracker_state_bytes(ctypes.byref(ok)), L.vkn_qd_tracker_workspace_bytes(ctypes.byref(ok))
    assert nb > 0 and nw > 0 and L.vkn_qd_tracker_state_layout(ctypes.byref(ok), off) == 0
    for frames in (65, 100):
        bad = cfg_of(frames)
        assert bad.max_tracklets + frames * bad.max_dets <= 4096
        assert L.vkn_qd_tracker_state_bytes(ctypes.byref(bad)) == 0 and L.vkn_qd_tracker_workspace_bytes(ctypes.byref(bad)) == 0
        assert L.vkn_qd_tracker_state_layout(ctypes.byref(bad), off) == -2
        assert L.vkn_qd_tracker_reset(ctypes.byref(bad), p, 1 << 30, None) == -2
        assert L.vkn_qd_tracker_match_f32(ctypes.byref(bad), p, 1 << 30, p, p, p, 4, 0, p, p, p, p, p, 1 << 30, None) == -2
        assert L.vkn_qd_tracker_match_dev_f32(ctypes.byref(bad), p, 1 << 30, p, p, p, p, 4, 0, p, p, p, p, p, 1 << 30, None) == -2
    wide = cfg_of(1, embed_dim=1025)                          # the neighbouring gate of the sweeps: embed_dim <= 1024
    assert L.vkn_qd_tracker_state_bytes(ctypes.byref(wide)) == 0
    assert L.vkn_qd_tracker_match_f32(ctypes.byref(wide), p, 1 << 30, p, p, p, 4, 0, p, p, p, p, p, 1 << 30, None) == -2
    assert L.vkn_qd_tracker_state_bytes(ctypes.byref(cfg_of(1, embed_dim=1024))) > 0


def test_build_tracker_raises_for_65_backdrop_frames(vkn, monkeypatch):
    """`build_tracker(...).match` with 65 frames raises VknError(-2) from the size query, before a buffer exists (the inputs only
    have to look like device tensors: nothing is allocated or launched)."""
    trk = vkn.build_tracker(dict(type='QuasiDenseEmbedTracker', max_dets=16, max_tracklets=64, memo_backdrop_frames=65))

    class FakeCuda(torch.Tensor):
        is_cuda = True

    mk = lambda t: t.as_subclass(FakeCuda)     # noqa: E731
    with pytest.raises(vkn.VknError) as ei:
        trk.match(mk(torch.zeros(2, 5)), mk(torch.zeros(2, dtype=torch.long)), mk(torch.zeros(2, 16)), 0)
    assert ei.value.code == -2 and 'memo_backdrop_frames <= 64' in str(ei.value)
    assert trk._state is None
