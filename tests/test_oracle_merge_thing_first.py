"""CPU: the oracle's restatement of the thing-first panoptic merge (`oracle.knet_oracle.thing_first_merge` + the host rule around it)
against the `merge_tf_*` fixtures, which hold what the reference's own `merge_stuff_thing` / `merge_stuff_thing_thing_first` returned
for masks made of rectangles (oracle/gen_golden.py: run_merge_thing_first).  Everything here is integer work: every comparison is
exact."""
import numpy as np
import pytest

from helpers import MERGE_TF, load_merge_tf, merge_tf_oracle, pan_info_rows
from oracle.knet_oracle import thing_first_feat_rows


def _bits(x):
    return int(np.asarray(x, dtype=np.float32).reshape(1).view(np.int32)[0])


@pytest.mark.parametrize('name', MERGE_TF)
def test_thing_first_merge_equals_the_reference(name):
    g, a, thr = load_merge_tf(name)
    args, r = merge_tf_oracle(a, thr)
    assert r['panoptic_seg'].dtype == np.int32 and np.array_equal(r['panoptic_seg'], g['panoptic_seg'])
    rows = pan_info_rows(r['segments_info'])
    assert rows.shape == g['info'].shape and np.array_equal(rows, g['info'], equal_nan=True)       # scores: the same double
    assert r['nseg'] == len(g['info'])
    # the per-step table says the same as the segment list
    info = r['info']
    assert info.shape == (len(args['thing_order']) + len(args['stuff_order']), 5)
    kept = info[info[:, 0] > 0]
    assert np.array_equal(kept[:, 0], np.arange(1, r['nseg'] + 1)) and np.array_equal(kept[:, 1] == 0, g['info'][:, 1] == 1)
    assert np.array_equal(kept[:, 2], g['info'][:, 2])
    if 'feat_rows' in g:
        assert np.array_equal(thing_first_feat_rows(args['thing_order'], r['segments_info']), g['feat_rows'])


def test_the_fixtures_hold_what_they_are_for():
    """merge_tf_dupstuff really interleaves labels and emits an area-0 segment; merge_tf_video's scores are unsorted and its embedding
    rows are neither the identity nor the accepted indices; the three empty cases are empty where they say."""
    g, a, thr = load_merge_tf('merge_tf_dupstuff')
    by_score = a['stuff_labels'][np.argsort(-a['stuff_scores'])].tolist()
    assert by_score == [2, 1, 2, 3, 1, 3] and thr['stuff_max_area'] == 0
    stuff = g['info'][g['info'][:, 1] == 0]
    assert stuff[:, 2].tolist() == [2, 1, 3] and stuff[2, 5] == 0 and stuff[0, 5] > 0 and stuff[1, 5] > 0
    m2, m1 = a['stuff_masks'][a['stuff_labels'] == 2], a['stuff_masks'][a['stuff_labels'] == 1]
    assert (m2[1] & ~m2[0]).any() and (m2.any(0) & m1.any(0)).any()       # the OR matters, and so does who comes first
    g, a, thr = load_merge_tf('merge_tf_video')
    order = np.argsort(-a['thing_scores'])
    assert not np.array_equal(order, np.arange(len(order)))
    ids = g['info'][g['info'][:, 1] == 1][:, 3].astype(np.int64)
    assert len(ids) < len(order) and not np.array_equal(g['feat_rows'], ids) and np.array_equal(g['feat_rows'], order[ids])
    for name, kt, ks, things in (('merge_tf_empty_things', 0, 3, 0), ('merge_tf_empty_stuff', 3, 0, 2), ('merge_tf_empty_below', 3, 2, 0)):
        g, a, thr = load_merge_tf(name)
        assert a['thing_masks'].shape[0] == kt and a['stuff_masks'].shape[0] == ks and int((g['info'][:, 1] == 1).sum()) == things
    assert (a['thing_scores'] < thr['instance_score_thr']).all() and a['thing_masks'].any()


# merge_tf_edges / merge_tf_thr step by step, written by hand from the geometry (oracle/gen_golden.py: _mtf_edge_things):
# (array index, label, decision).  Things in paste order A B C D E F G H I J, then the five stuff masks s1 .. s5.
_THINGS = [(2, 0, 'accept'),      # A  8x8 block on an empty map
           (5, 1, 'accept'),      # B  2 of its 4 px in A: 0.5 is not > 0.5 (nor > 0.6) -> clipped to 2 px
           (1, 0, 'C'),           # C  3 of 5 px in A: 0.6 > 0.5 rejects; 3 * 1.0 / 5 is not > 0.6 -> accepted, 2 px
           (9, 0, 'reject'),      # D  5 of 8 px in A: 0.625, one pixel over 4 of 8
           (4, 0, 'reject'),      # E  empty mask
           (8, 1, 'reject'),      # F  inside A
           (0, 1, 'accept'),      # G  union of two rectangles, clear
           (7, 1, 'accept'),      # H  score == threshold: not below it
           (3, 1, 'stop'),        # I  the fp32 value below the threshold: `break`
           (6, 0, 'stop')]        # J  behind the break
_STUFF = [(1, 12, True),          # s1 16 px, 4 under A: 12 == stuff_max_area
          (2, 11, False),         # s2 12 px, 1 under H: one short
          (4, 0, False),          # s3 under A
          (3, None, True),        # s4 the whole image: what is left
          (5, 0, False)]          # s5 behind s4


@pytest.mark.parametrize('name', ['merge_tf_edges', 'merge_tf_thr'])
def test_edge_fixture_decisions_step_by_step(name):
    g, a, thr = load_merge_tf(name)
    args, r = merge_tf_oracle(a, thr)
    c_accepted = name == 'merge_tf_thr'
    tm, sc = a['thing_masks'], a['thing_scores']
    # premises: the inputs sit where the table says they do
    A, B, C, D, Hh, I = (tm[i] for i in (2, 5, 1, 9, 7, 3))
    assert (int((B & A).sum()), int(B.sum())) == (2, 4) and 2 * 1.0 / 4 == 0.5 and not 0.5 > thr['iou_thr']
    assert (int((C & A).sum()), int(C.sum())) == (3, 5) and 3 * 1.0 / 5 == 0.6 and float(np.float32(0.6)) > 0.6     # fp32 on one side flips it
    assert (3 * 1.0 / 5 > thr['iou_thr']) == (not c_accepted)
    assert (int((D & A).sum()), int(D.sum())) == (5, 8) and 5 * 1.0 / 8 > thr['iou_thr'] >= 4 * 1.0 / 8
    assert not tm[4].any() and not (tm[8] & ~A).any() and tm[8].any()
    at = np.float32(0.3 if c_accepted else 0.25)
    assert sc[7] == at and not float(sc[7]) < thr['instance_score_thr']
    assert sc[3] == np.nextafter(at, np.float32(0)) and float(sc[3]) < thr['instance_score_thr']
    assert (float(at) == thr['instance_score_thr']) == (not c_accepted)            # 0.25 is an fp32, 0.3 is not: float32(0.3) > 0.3
    others = tm[[2, 5, 1, 9, 8, 0]].any(0)
    assert Hh.any() and I.any() and not (Hh & others).any() and not (I & (others | Hh)).any()      # both would be painted whole
    # the table
    want, sid = [], 0
    for idx, label, what in _THINGS:
        take = what == 'accept' or (what == 'C' and c_accepted)
        sid += take
        want.append((sid if take else 0, 0, label, idx, _bits(sc[idx])))
    painted = 64 + 2 + (2 if c_accepted else 0) + (80 + 36 - 8) + 16
    for label, area, take in _STUFF:
        area = 24 * 40 - painted - 12 if area is None else area
        sid += take
        want.append((sid if take else 0, 1, label, area, 0))
    assert thr['stuff_max_area'] == 12 and np.array_equal(r['info'], np.array(want, dtype=np.int32))
    assert r['nseg'] == sid == (7 if c_accepted else 6)
    assert np.array_equal(args['thing_order'], [t[0] for t in _THINGS])
