"""Hand-made videos for the quasi-dense tracker (csrc/vkn_tracker.hip, oracle/tracker_oracle.py): every case puts ONE decision of the
association exactly on its limit, one step above or one step below, and states the outcome by hand.  The subject of
tests/test_tracker_edge_cases.py (CPU: the oracle gives these outcomes) and of tests/test_gpu_tracker.py (the kernel gives them);
oracle/gen_golden_tracker.py runs the same inputs through the reference's own class.  Nothing here touches the product package.

Every quantity that feeds a decision is exact in fp32 in any evaluation order:
  boxes   small integers (areas, intersections and unions are integers; the IoUs at a limit are 4/8);
  scores  multiples of 2^-6, written as their numerator `s64`;
  embeds  entries in {0, +1, -1} with exactly four non-zeros: norm 2, normalised entries +-0.5, every cosine a multiple of 0.25
          (match_metric='cosine'; softmax and bisoftmax cannot sit on a threshold and appear in the sweeps only).
A det is (box4, s64, label, embed); a frame a list of dets in INPUT order; `expect[t]` holds for frame t
  order   input rows of the surviving detections, in output order          labels / ids   of those rows, as returned
  trk     ids of the live tracklets after the frame, in table order         (optional)
  bd      the backdrop ring after the frame, newest first: [[(frame index, input row), ...], ...]   (optional)
  memo    {id: dict(last, acc, label, box, vel, emb)} after the frame, any subset of keys            (optional)
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

E = 16
STEP = 1.0 / 64
BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0)))
BASE = dict(init_score_thr=0.5, obj_score_thr=0.25, match_score_thr=0.5, memo_tracklet_frames=10, memo_backdrop_frames=1,
            memo_momentum=0.5, nms_conf_thr=0.5, nms_backdrop_iou_thr=0.25, nms_class_iou_thr=0.5, with_cats=True, match_metric='cosine')
CAPS = dict(max_dets=16, max_tracklets=16)


def e4(*signed):
    """four non-zeros: e4(1, 2, -3, 4) has +1 at 1, 2, 4 and -1 at 3 (1-based)"""
    assert len(signed) == 4 and len({abs(i) for i in signed}) == 4
    v = [0.0] * E
    for i in signed:
        v[abs(i) - 1] = 1.0 if i > 0 else -1.0
    return tuple(v)


_FILL = list(itertools.combinations(range(7, 17), 4))


def fill(i):
    """filler embeddings on entries 7..16: cosine 0 with everything written on entries 1..6"""
    return e4(*_FILL[i % len(_FILL)])


def P(k, dx=0, dy=0):
    """2 x 3 box number k of a row of disjoint boxes"""
    return (10 * k + dx, dy, 10 * k + 2 + dx, 3 + dy)


A = e4(1, 2, 3, 4)
A75 = e4(1, 2, 3, 5)      # cosine 0.75 with A
A75b = e4(1, 2, 3, 6)     # cosine 0.75 with A, 0.75 with A75
A50 = e4(1, 2, 5, 6)      # cosine 0.5 with A
A25 = e4(1, 5, 6, 7)      # cosine 0.25 with A, 0.5 with A75
Z = fill(0)               # cosine 0 with all of them
Z2 = fill(209)            # (13, 14, 15, 16): cosine 0 with Z = (7, 8, 9, 10) too

CASES = {}


def case(name, why, frames, expect, cfg=None, caps=None, frame_ids=None, reference=True):
    assert name not in CASES and len(frames) == len(expect)
    CASES[name] = dict(name=name, why=why, frames=frames, expect=expect, cfg=dict(BASE, **(cfg or {})), caps=dict(CAPS, **(caps or {})),
                       frame_ids=list(frame_ids) if frame_ids is not None else list(range(len(frames))), reference=reference)


def ex(order, labels, ids, **more):
    assert len(order) == len(labels) == len(ids)
    return dict(order=list(order), labels=list(labels), ids=list(ids), **more)


def inputs(c):
    """-> [(frame_id, boxes [n,5] fp32, labels [n] int64, embeds [n,E] fp32)]"""
    out = []
    for fid, dets in zip(c['frame_ids'], c['frames']):
        bb = np.asarray([list(d[0]) + [d[1] * STEP] for d in dets], dtype=np.float32).reshape(-1, 5)
        out.append((fid, bb, np.asarray([d[2] for d in dets], dtype=np.int64), np.asarray([d[3] for d in dets], dtype=np.float32).reshape(-1, E)))
    return out


# ------------------------------------------------------------------------------------------------ match_score_thr (phase E, `best > thr`)
_born = [(P(0), 48, 0, A)]
for _n, _emb, _thr, _s, _ids, _why in (
        ('match_at', A50, 0.5, 48, [1], 'best cosine 0.5 == match_score_thr: no match; score 0.75 > init: born as id 1'),
        ('match_at_no_birth', A50, 0.5, 32, [-1], 'as match_at with score == init_score_thr: neither matched nor born'),
        ('match_above', A75, 0.5, 48, [0], 'best cosine 0.75 > 0.5: takes id 0'),
        ('match_below_thr', A50, BELOW_HALF, 48, [0], 'best cosine 0.5 > nextafter(0.5, 0): takes id 0')):
    case(_n, _why, [_born, [(P(0), _s, 0, _emb)]], [ex([0], [0], [0], trk=[0]), ex([0], [0], _ids)], cfg=dict(match_score_thr=_thr))

# ------------------------------------------------------------------------------------------------ obj_score_thr in phase E (`score > thr`)
case('obj_e_at_conf_above', 'score == obj_score_thr with a matching track (0.75): no id; 0.75 > nms_conf_thr: -2, kept out of the backdrops',
     [_born, [(P(0), 16, 0, A75)]], [ex([0], [0], [0]), ex([0], [0], [-2], bd=[[]], memo={0: dict(last=0, acc=0)})])
case('obj_e_at_conf_equal', 'score == obj_score_thr, match 0.5 > match_score_thr 0.25 but == nms_conf_thr: stays -1 and is a backdrop',
     [_born, [(P(0), 16, 0, A50)]], [ex([0], [0], [0]), ex([0], [0], [-1], bd=[[(1, 0)]], memo={0: dict(last=0, acc=0)})],
     cfg=dict(match_score_thr=0.25))
case('obj_e_above', 'score one step above obj_score_thr: takes id 0',
     [_born, [(P(0), 17, 0, A75)]], [ex([0], [0], [0]), ex([0], [0], [0], bd=[[]], memo={0: dict(last=1, acc=1)})])
case('obj_e_below', 'score one step below obj_score_thr: as at the limit, -2',
     [_born, [(P(0), 15, 0, A75)]], [ex([0], [0], [0]), ex([0], [0], [-2], bd=[[]])])

# ------------------------------------------------------------------------------------------------ obj_score_thr in phase B (`score < thr`)
# the better box overlaps by 3/9: between nms_backdrop_iou_thr 0.25 and nms_class_iou_thr 0.5
for _n, _s, _e, _why in (
        ('obj_b_at', 16, ex([0, 1], [0, 0], [0, -1], bd=[[]]), 'score == obj_score_thr is not < it: class limit 0.5, 1/3 survives (no backdrop: 1/3 > 0.25)'),
        ('obj_b_below', 15, ex([0], [0], [0], bd=[[]]), 'score one step below obj_score_thr: backdrop limit 0.25, 1/3 dies'),
        ('obj_b_above', 17, ex([0, 1], [0, 0], [0, -1], bd=[[]]), 'score above obj_score_thr: class limit, survives')):
    case(_n, _why, [[((0, 0, 2, 3), 48, 0, A), ((1, 0, 3, 3), _s, 0, Z)]], [_e])

# ------------------------------------------------------------------------------------------------ IoU equal to a limit (`iou > thr`)
_HALF = ((0, 0, 2, 3), (0, 1, 2, 4))        # areas 6, intersection 4: 4 / 8
_FIVE7 = ((0, 0, 1, 6), (0, 1, 1, 7))       # areas 6, intersection 5: 5 / 7
_THIRD = ((0, 0, 2, 3), (1, 0, 3, 3))       # areas 6, intersection 3: 3 / 9
IOU_PAIRS = {'half': (_HALF, 4, 8), 'five7': (_FIVE7, 5, 7), 'third': (_THIRD, 3, 9)}
for _n, _pair, _thr, _e, _why in (
        ('iou_b_at', _HALF, 0.5, ex([0, 1], [0, 0], [0, 1]), 'IoU 4/8 == nms_class_iou_thr: survives (and is born)'),
        ('iou_b_above', _FIVE7, 0.5, ex([0], [0], [0]), 'IoU 5/7 > nms_class_iou_thr: dies'),
        ('iou_b_below', _THIRD, 0.5, ex([0, 1], [0, 0], [0, 1]), 'IoU 3/9 < nms_class_iou_thr: survives'),
        ('iou_b_below_thr', _HALF, BELOW_HALF, ex([0], [0], [0]), 'IoU 4/8 > nextafter(0.5, 0): dies')):
    case(_n, _why, [[(_pair[0], 48, 0, A), (_pair[1], 40, 0, Z)]], [_e], cfg=dict(nms_class_iou_thr=_thr))
for _n, _pair, _thr, _bd, _why in (
        ('iou_g_at', _HALF, 0.5, [[(0, 1)]], 'unassigned box, IoU 4/8 == nms_backdrop_iou_thr with a better one: kept as a backdrop'),
        ('iou_g_above', _FIVE7, 0.5, [[]], 'IoU 5/7 > nms_backdrop_iou_thr (< class limit 0.75, so it survived phase B): no backdrop'),
        ('iou_g_below', _THIRD, 0.5, [[(0, 1)]], 'IoU 3/9 < nms_backdrop_iou_thr: a backdrop'),
        ('iou_g_below_thr', _HALF, BELOW_HALF, [[]], 'IoU 4/8 > nextafter(0.5, 0): no backdrop')):
    case(_n, _why, [[(_pair[0], 48, 0, A), (_pair[1], 24, 0, Z)]], [ex([0, 1], [0, 0], [0, -1], bd=_bd)],
         cfg=dict(nms_class_iou_thr=0.75, nms_backdrop_iou_thr=_thr))

case('suppressed_suppressor', 'b (24/40 with a) dies; c overlaps b by 16/40 > 0.25 and a by 0: c dies too, suppression is against EVERY better box',
     [[((6, 0, 10, 4), 40, 2, Z), ((0, 0, 6, 4), 56, 0, A), ((0, 0, 10, 4), 48, 1, A50)]], [ex([1], [0], [0], bd=[[]])],
     cfg=dict(nms_class_iou_thr=0.25))

# ------------------------------------------------------------------------------------------------ init_score_thr (phase F, `score > thr`)
case('init_at', 'score == init_score_thr: no birth, id -1, a backdrop', [[(P(0), 32, 0, A)]], [ex([0], [0], [-1], trk=[], bd=[[(0, 0)]])])
case('init_above', 'score one step above init_score_thr: born', [[(P(0), 33, 0, A)]], [ex([0], [0], [0], trk=[0], bd=[[]])])
case('init_below', 'score one step below init_score_thr: no birth', [[(P(0), 31, 0, A)]], [ex([0], [0], [-1], trk=[], bd=[[(0, 0)]])])
case('init_order', 'ids are handed out in score order within the frame, the rows at and below the limit get none',
     [[(P(0), 32, 0, A), (P(1), 33, 0, Z), (P(2), 40, 1, A50), (P(3), 31, 2, Z2), (P(4), 63, 3, A25)]],
     [ex([4, 2, 1, 0, 3], [3, 1, 0, 0, 2], [0, 1, 2, -1, -1], trk=[0, 1, 2], bd=[[(0, 0), (0, 3)]])])

# ------------------------------------------------------------------------------------------------ equal scores (phase A: stable)
case('equal_scores', 'three equal scores keep input order in the outputs and in the ids of their births (a better row first)',
     [[(P(0), 40, 0, A), (P(1), 40, 1, Z), (P(2), 40, 2, Z2), (P(3), 48, 3, A50)]],
     [ex([3, 0, 1, 2], [3, 0, 1, 2], [0, 1, 2, 3], trk=[0, 1, 2, 3])], reference=False)

# ------------------------------------------------------------------------------------------------ equal match scores: the lower column
_tracks = lambda n, tied: [(P(r), 48, 0, tied.get(r, fill(r))) for r in range(n)]     # noqa: E731  (equal scores: ids = rows)
_big = dict(max_dets=80, max_tracklets=80)
case('tie_same_lane_tracks', 'columns 2 and 66 (one lane of the scan) both 0.75: the earlier-created tracklet, id 2',
     [_tracks(70, {2: A75, 66: A75b}), [(P(0), 48, 0, A)]],
     [ex(range(70), [0] * 70, range(70)), ex([0], [0], [2])], caps=_big, reference=False)
case('tie_other_lane_tracks', 'columns 5 and 40 (different lanes, the shuffle reduce) both 0.75: id 5',
     [_tracks(70, {40: A75, 5: A75b}), [(P(0), 48, 0, A)]],
     [ex(range(70), [0] * 70, range(70)), ex([0], [0], [5])], caps=_big, reference=False)
_bds = lambda first, tied: [(P(first + r), 24 - r, 0, tied.get(r, fill(100 + r))) for r in range(4)]     # noqa: E731
case('tie_same_lane_backdrop', '64 tracklets, then 4 backdrops: columns 1 (tracklet) and 65 (backdrop) both 0.75: the tracklet, id 1',
     [_tracks(64, {1: A75}) + _bds(64, {1: A75b}), [(P(0), 48, 0, A)]],
     [ex(range(68), [0] * 68, list(range(64)) + [-1] * 4, bd=[[(0, 64), (0, 65), (0, 66), (0, 67)]]), ex([0], [0], [1])],
     caps=_big, reference=False)
case('tie_other_lane_backdrop', '4 tracklets, 4 backdrops: columns 1 (tracklet) and 6 (backdrop) both 0.75: the tracklet, id 1',
     [[(P(r), 48 - r, 0, {1: A75}.get(r, fill(r))) for r in range(4)] + _bds(4, {2: A75b}), [(P(0), 48, 0, A)]],
     [ex(range(8), [0] * 8, [0, 1, 2, 3, -1, -1, -1, -1]), ex([0], [0], [1])])

# ------------------------------------------------------------------------------------------------ the taken mask
_two = [(P(0), 48, 0, A), (P(1), 47, 0, A25)]
_both = [(P(1), 40, 0, A75), (P(0), 48, 0, A)]       # row 1 (better) takes track 0 with 1.0; row 0 prefers track 0 too (0.75), then 0.5
case('taken_second_choice', 'both prefer track 0; the better-scored takes it, the other reads 0 there and takes track 1 (0.5 > 0.25)',
     [_two, _both], [ex([0, 1], [0, 0], [0, 1]), ex([1, 0], [0, 0], [0, 1], trk=[0, 1])], cfg=dict(match_score_thr=0.25))
case('taken_no_choice', 'as above with match_score_thr 0.5: the second choice 0.5 is not above it: no match, born as id 2',
     [_two, _both], [ex([0, 1], [0, 0], [0, 1]), ex([1, 0], [0, 0], [0, 2], trk=[0, 1, 2])])

# ------------------------------------------------------------------------------------------------ the best column is a backdrop
_bdmemo = [(P(0), 48, 0, Z), (P(1), 24, 0, A)]
case('backdrop_hit_birth', 'best column (0.75) is a backdrop: no id and no -2; score > init: born',
     [_bdmemo, [(P(5), 48, 0, A75)]], [ex([0, 1], [0, 0], [0, -1], bd=[[(0, 1)]]), ex([0], [0], [1], bd=[[]])])
case('backdrop_hit_low', 'best column is a backdrop, score <= obj_score_thr: stays -1 (not -2) and becomes a backdrop itself',
     [_bdmemo, [(P(5), 16, 0, A75)]], [ex([0, 1], [0, 0], [0, -1]), ex([0], [0], [-1], bd=[[(1, 0)]])])

# ------------------------------------------------------------------------------------------------ with_cats
case('cats_on', 'same embedding, other label: with_cats zeroes the score, no match, born as id 1',
     [_born, [(P(0), 48, 1, A)]], [ex([0], [0], [0]), ex([0], [1], [1], trk=[0, 1], memo={0: dict(label=0), 1: dict(label=1)})])
case('cats_off', 'with_cats=False: the label does not block the match, and the track takes the detection\'s label',
     [_born, [(P(0), 48, 1, A)]], [ex([0], [0], [0]), ex([0], [1], [0], trk=[0], memo={0: dict(label=1, acc=1)})], cfg=dict(with_cats=False))

case('empty_memo', 'a backdrop but no tracklet: no matching at all (`not self.empty`); the outcome equals a backdrop hit, stated for the record',
     [[(P(0), 24, 0, A)], [(P(0), 48, 0, A)]], [ex([0], [0], [-1], trk=[], bd=[[(0, 0)]]), ex([0], [0], [0], trk=[0], bd=[[]])])

# ------------------------------------------------------------------------------------------------ expiry (`frame - last >= frames`)
_a, _b = (P(0), 48, 0, A), (P(1), 47, 0, Z)
case('expiry_ge', 'memo_tracklet_frames=3: b, last seen at frame 2, is alive after frame 4 (2 < 3) and gone after frame 5 (3 >= 3); back at 6 it is new',
     [[_a, _b], [_a, _b], [_a, _b], [_a], [_a], [_a], [_a, _b]],
     [ex([0, 1], [0, 0], [0, 1], trk=[0, 1])] * 3 + [ex([0], [0], [0], trk=[0, 1])] * 2 + [ex([0], [0], [0], trk=[0]),
                                                                                           ex([0, 1], [0, 0], [0, 2], trk=[0, 2])],
     cfg=dict(memo_tracklet_frames=3))
_five = lambda t, rows: [(P(r, dx=2 * t), 50 - r, r, e4(1, 2, 3, 7 + r) if t == 0 else e4(1, 2, 4, 7 + r)) for r in rows]     # noqa: E731
_m5 = lambda r: dict(last=2, acc=2, label=r, box=P(r, dx=4) + (np.float32((50 - r) * STEP),), vel=(2, 0, 2, 0, 0), emb=e4(1, 2, 4, 7 + r))  # noqa: E731
case('expiry_compaction', 'rows 0 and 2 of five expire at frame 2 (memo_tracklet_frames=2): rows 1, 3, 4 move up with box, velocity, embedding',
     [_five(0, range(5)), _five(1, (1, 3, 4)), _five(2, (1, 3, 4))],
     [ex(range(5), range(5), range(5), trk=[0, 1, 2, 3, 4]), ex([0, 1, 2], [1, 3, 4], [1, 3, 4], trk=[0, 1, 2, 3, 4]),
      ex([0, 1, 2], [1, 3, 4], [1, 3, 4], trk=[1, 3, 4], memo={1: _m5(1), 3: _m5(3), 4: _m5(4)})],
     cfg=dict(memo_tracklet_frames=2, memo_momentum=1.0))
case('birth_and_expiry', 'frame 2: c is born while a (last seen at 0, memo_tracklet_frames=2) expires',
     [[_a], [_b], [(P(2), 46, 0, Z2)]], [ex([0], [0], [0], trk=[0]), ex([0], [0], [1], trk=[0, 1]), ex([0], [0], [2], trk=[1, 2])],
     cfg=dict(memo_tracklet_frames=2))
case('expiry_zero', 'memo_tracklet_frames=0: every track leaves in the frame it was born, so the same object is new each time',
     [[_a], [_a], [_a]], [ex([0], [0], [0], trk=[]), ex([0], [0], [1], trk=[]), ex([0], [0], [2], trk=[])], cfg=dict(memo_tracklet_frames=0))

# ------------------------------------------------------------------------------------------------ frame gaps and the velocity mean
_gap = [(0, 0, 2, 3), (3, 0, 5, 3), (12, 3, 14, 6), (15, 5, 17, 8)]
case('frame_gaps', 'frame ids 0, 1, 4, 5: velocities (3,0,3,0), (9,3,9,3)/3, (3,2,3,2); running mean with acc = 0, 1, 2',
     [[(b, 48, 0, A)] for b in _gap],
     [ex([0], [0], [0], memo={0: dict(last=0, acc=0, vel=(0, 0, 0, 0, 0))}), ex([0], [0], [0], memo={0: dict(last=1, acc=1, vel=(3, 0, 3, 0, 0))}),
      ex([0], [0], [0], memo={0: dict(last=4, acc=2, vel=(3, 0.5, 3, 0.5, 0))}),
      ex([0], [0], [0], memo={0: dict(last=5, acc=3, vel=(3, 1, 3, 1, 0), box=_gap[3] + (0.75,))})], frame_ids=[0, 1, 4, 5])

# ------------------------------------------------------------------------------------------------ momentum: (1 - m) * A + m * A75
for _m, _emb in ((0.0, A), (1.0, A75), (0.25, tuple(0.75 * x + 0.25 * y for x, y in zip(A, A75)))):
    case(f'momentum_{_m}', f'memo_momentum={_m} is dyadic: the momentum embedding is exact',
         [_born, [(P(0), 48, 0, A75)]], [ex([0], [0], [0]), ex([0], [0], [0], memo={0: dict(emb=_emb, acc=1)})], cfg=dict(memo_momentum=_m))
case('momentum_0.3', 'memo_momentum=0.3 is not dyadic: the embedding is compared with the oracle\'s (same fp32 operation sequence)',
     [_born, [(P(0), 48, 0, A75)]], [ex([0], [0], [0]), ex([0], [0], [0], memo={0: dict(acc=1)})], cfg=dict(memo_momentum=0.3))

# ------------------------------------------------------------------------------------------------ the backdrop ring
RING_COUNTS = (2, 0, 3, 1, 0, 4)     # backdrops of frame t: RING_COUNTS[t % 6]


def _ring(frames_kept, T):
    frames = [[_a] + [(P(1 + r), 24 - r, 0, fill(5 * t + r)) for r in range(RING_COUNTS[t % 6])] for t in range(T)]
    expect = []
    for t in range(T):
        k = RING_COUNTS[t % 6]
        ring = [[(u, 1 + r) for r in range(RING_COUNTS[u % 6])] for u in range(t, max(t - frames_kept, -1), -1)]
        expect.append(ex(range(k + 1), [0] * (k + 1), [0] + [-1] * k, trk=[0], bd=ring))
    return frames, expect


for _f, _T in ((0, 4), (1, 7), (2, 8), (64, 66)):
    case(f'ring_{_f}', f'memo_backdrop_frames={_f}: after frame t the ring holds the backdrops of frames t, t-1, .. (at most {_f}), empty frames included',
         *_ring(_f, _T), cfg=dict(memo_backdrop_frames=_f, memo_tracklet_frames=100), caps=dict(max_dets=8, max_tracklets=16))

# the two cases that also go through the padded / device-count entry
PADDED_CASES = ('taken_second_choice', 'init_order')


# ==================================================================================================== running and checking a case
def cosines(det_emb, memo_emb):
    """the fp32 cosine matrix as the oracle computes it, and in float64"""
    d, m = torch.as_tensor(det_emb), torch.as_tensor(memo_emb)
    f32 = torch.mm(F.normalize(d, p=2, dim=1), F.normalize(m, p=2, dim=1).t())
    f64 = torch.mm(F.normalize(d.double(), p=2, dim=1), F.normalize(m.double(), p=2, dim=1).t())
    return f32, f64


class OracleRunner:
    """`step` / `tracklets` / `backdrops` over oracle/tracker_oracle.py in the vocabulary of `check_case`."""

    def __init__(self, cfg, caps=None):
        from oracle.tracker_oracle import TrackerOracle
        self.ora = TrackerOracle(**cfg)

    def step(self, bb, lab, em, fid):
        b, l_, ids = self.ora.step(torch.from_numpy(bb), torch.from_numpy(lab), torch.from_numpy(em), fid)
        return b.numpy(), l_.numpy(), ids.numpy()

    def tracklets(self):
        o = self.ora
        return [dict(id=o.t_id[i], label=int(o.t_label[i]), last=o.t_last[i], acc=o.t_acc[i], box=o.t_box[i].numpy(), vel=o.t_vel[i].numpy(),
                     emb=o.t_emb[i].numpy()) for i in range(len(o.t_id))]

    def backdrops(self):
        return [dict(box=f['box'].numpy(), emb=f['emb'].numpy(), label=f['label'].numpy()) for f in self.ora.backdrops]


def check_case(c, runner, twin=None):
    """Runs the video through `runner` and asserts the hand-stated outcome of every frame; `twin` (a second runner, the oracle) is
    stepped alongside for what the case leaves to it (the non-dyadic momentum embedding)."""
    ins = inputs(c)
    for t, ((fid, bb, lab, em), e) in enumerate(zip(ins, c['expect'])):
        b, l_, ids = runner.step(bb, lab, em, fid)
        where = (c['name'], t, c['why'])
        assert ids.tolist() == e['ids'], where + (ids.tolist(),)
        assert l_.tolist() == e['labels'], where + (l_.tolist(),)
        assert np.array_equal(b, bb[e['order']].reshape(-1, 5)), where + (b.tolist(),)
        if twin is not None:
            twin.step(bb, lab, em, fid)
        if 'trk' in e or 'memo' in e:
            tr = runner.tracklets()
            if 'trk' in e:
                assert [r['id'] for r in tr] == e['trk'], where + ([r['id'] for r in tr],)
            for tid, want in e.get('memo', {}).items():
                row = next(r for r in tr if r['id'] == tid)
                for k, v in want.items():
                    if k in ('box', 'vel', 'emb'):
                        assert np.array_equal(row[k], np.asarray(v, dtype=np.float32)), where + (tid, k, row[k].tolist())
                    else:
                        assert row[k] == v, where + (tid, k, row[k])
                if twin is not None:
                    ref = next(r for r in twin.tracklets() if r['id'] == tid)
                    assert np.array_equal(row['emb'], ref['emb']) and np.array_equal(row['vel'], ref['vel']), where + (tid, 'twin')
        if 'bd' in e:
            bd = runner.backdrops()
            assert [f['box'].shape[0] for f in bd] == [len(f) for f in e['bd']], where + ([f['box'].shape[0] for f in bd],)
            for got, want in zip(bd, e['bd']):
                for i, (u, r) in enumerate(want):
                    _, ub, ul, ue = ins[u]
                    assert np.array_equal(got['box'][i], ub[r]) and np.array_equal(got['emb'][i], ue[r]) and int(got['label'][i]) == int(ul[r]), \
                        where + ('backdrop', i, u, r)


# ==================================================================================================== sweeps against the oracle (seeded)
def grid_video(T, n, emb, n_cls, seed, persistent=None, lo=0.05, hi=0.99):
    """n detections per frame on a grid of disjoint 20 x 20 boxes (every one survives phase B), shuffled rows, random scores;
    embeddings: persistent codes + noise; with `persistent=k` only the first k objects keep their code, the others get a new one
    in every frame (mostly births)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    cell = np.stack([np.arange(n) % side, np.arange(n) // side], 1).astype(np.float64) * 40.0
    codes = rng.standard_normal((n, emb)).astype(np.float32) * 2.0
    cls = rng.integers(0, n_cls, n)
    frames = []
    for t in range(T):
        if persistent is not None:
            codes[persistent:] = rng.standard_normal((n - persistent, emb)).astype(np.float32) * 2.0
        rows = rng.permutation(n)
        jit = rng.integers(0, 4, (n, 2)).astype(np.float64)
        xy = cell[rows] + jit
        sc = rng.uniform(lo, hi, n)
        boxes = np.concatenate([xy, xy + 20.0, sc[:, None]], 1).astype(np.float32)
        embs = (codes[rows] + rng.standard_normal((n, emb)).astype(np.float32) * 0.4).astype(np.float32)
        frames.append((boxes, cls[rows].astype(np.int64), embs))
    return frames


SWEEP_CFG = dict(init_score_thr=0.5, obj_score_thr=0.35, match_score_thr=0.5, memo_tracklet_frames=3, memo_backdrop_frames=1,
                 memo_momentum=0.8, nms_conf_thr=0.5, nms_backdrop_iou_thr=0.3, nms_class_iou_thr=0.7, with_cats=True, match_metric='bisoftmax')


def _sweeps():
    from oracle.tracker_oracle import random_video
    s = {}
    s['n256'] = dict(cfg=dict(SWEEP_CFG), caps=dict(max_dets=256, max_tracklets=1024), video=lambda: grid_video(3, 256, 16, 3, 11))
    # 8-d random codes: cosine above 0.9 is rare between strangers and sure for an object's own track, so most of the other 240 are births
    s['memo_over_1024'] = dict(cfg=dict(SWEEP_CFG, memo_backdrop_frames=2, memo_tracklet_frames=10, match_metric='cosine', match_score_thr=0.9,
                                        init_score_thr=0.1, obj_score_thr=0.08),
                               caps=dict(max_dets=256, max_tracklets=1400), video=lambda: grid_video(6, 256, 8, 2, 12, persistent=16))
    for e, metric in ((1, 'bisoftmax'), (3, 'bisoftmax'), (3, 'softmax'), (3, 'cosine'), (1024, 'bisoftmax')):
        s[f'embed_{e}_{metric}'] = dict(cfg=dict(SWEEP_CFG, match_metric=metric), caps=dict(max_dets=32, max_tracklets=128),
                                        video=lambda e=e: random_video(5, 24, e, 2, 20 + e))
    for metric in ('bisoftmax', 'softmax', 'cosine'):
        s[f'no_cats_{metric}'] = dict(cfg=dict(SWEEP_CFG, with_cats=False, match_metric=metric), caps=dict(max_dets=64, max_tracklets=512),
                                      video=lambda: random_video(8, 60, 32, 4, 31))
    for mom in (0.3, 1.0):
        s[f'momentum_{mom}'] = dict(cfg=dict(SWEEP_CFG, memo_momentum=mom), caps=dict(max_dets=64, max_tracklets=512),
                                    video=lambda: random_video(8, 60, 32, 4, 32))
    return s


SWEEPS = _sweeps()

# ---- the table exactly full: no expiry, so the births of the video fill `max_tracklets = births` to the last row
FULL_CFG = dict(SWEEP_CFG, memo_tracklet_frames=100, match_metric='cosine')


def full_table_video():
    """(frames, one frame more): the extra frame is a single new object with a top score: one more birth after the video that
    fills the table."""
    from oracle.tracker_oracle import random_video
    frames = random_video(5, 20, 16, 2, 41)
    rng = np.random.default_rng(43)
    extra = (np.asarray([[5000, 5000, 5040, 5040, 0.96875]], dtype=np.float32), np.asarray([0], dtype=np.int64),
             (rng.standard_normal((1, 16)) * 2.0).astype(np.float32))
    return frames, extra


# ---- full table, birth and expiry in one frame: the capacity test comes BEFORE the expiry compaction (hand-stated; the oracle and
#      the reference have no table).  max_tracklets = 2, memo_tracklet_frames = 2.
FULL_EXPIRY = dict(
    cfg=dict(BASE, memo_tracklet_frames=2), caps=dict(max_dets=16, max_tracklets=2),
    frames=[[_a, _b], [_b], [_b, (P(2), 46, 0, Z2)], [_b, (P(2), 46, 0, Z2)]],
    # ids, status of the call, live ids after the frame, ids handed out so far
    expect=[([0, 1], 0, [0, 1], 2), ([1], 0, [0, 1], 2),
            ([1, 2], 1, [1], 3),          # a expires in this frame, yet c's birth found the table full: dropped, id 2 consumed
            ([1, 3], 0, [1, 3], 4)])      # c is unknown to the memo: born again, now with room
