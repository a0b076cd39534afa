"""tests/maskap_ref.py, the restatement of COCO mask AP that judges the device meter (include/vkn_maskap.h): known answers worked by hand
from integer overlap tables.  `pr` carries np.spacing(1) in its denominator, so the expected values are written with the same expression."""
import numpy as np

import maskap_ref as R
from mask_ap_cases import EPS, P, img, match_cases

ONE = 1.0 / (1.0 + EPS)


def _mean_of(values_and_counts, shape):
    """np.mean of an array [T, 101] whose rows hold the values in the given multiplicities (the order of summation is the meter's)"""
    row = np.concatenate([np.full((n,), v) for v, n in values_and_counts])
    return float(np.mean(np.broadcast_to(row, shape).copy()))


def test_one_perfect_detection_is_ap_one_at_every_threshold():
    out = R.evaluate([img(1, [[100]], [100], [100], [0.9], [0], [0])], 1)
    assert np.all(out['precision'][:, :, 0, 0, :] == ONE) and np.all(out['recall'][:, 0, 0, :] == 1.0)
    # (a mean over 1010 equal values and one over 101 may differ in the last bit: each is compared with the mean of its own shape)
    assert out['stats'][0] == _mean_of([(ONE, 101)], (10, 101)) and out['stats'][1] == _mean_of([(ONE, 101)], (1, 101))
    # COCOeval selects a threshold with `iouThr == iouThrs`: np.arange(0.5, 0.96, 0.05), the reference's default, holds 0.5 but not 0.75
    # (0.7500000000000002), so mAP_75 is -1 with it and a number with np.linspace(0.5, 0.95, 10)
    assert R.COCO_THRS[5] != 0.75 and out['stats'][2] == -1.0
    lin = R.evaluate([img(1, [[100]], [100], [100], [0.9], [0], [0])], 1, thrs=np.linspace(0.5, 0.95, 10))
    assert lin['stats'][2] == lin['stats'][1] == out['stats'][1]
    assert out['stats'][8] == 1.0 and abs(out['stats'][0] - 1.0) < 1e-15
    assert out['stats'][3] == out['stats'][0] and out['stats'][4] == out['stats'][5] == -1.0          # 100 px: small
    assert out['classwise'][0] == out['stats'][0] and out['npig'].tolist() == [[1, 1, 0, 0]]


def test_tp_fp_tp_on_two_ground_truths():
    out = R.evaluate([img(1, [[100, 0], [0, 0], [0, 100]], [100] * 3, [100] * 2, [0.9, 0.8, 0.7], [0] * 3, [0] * 2)], 1)
    p2 = 2.0 / (1.0 + 2.0 + EPS)
    want = np.array([ONE] * 51 + [p2] * 50)
    assert np.array_equal(out['precision'][:, :, 0, 0, 2], np.broadcast_to(want, (10, 101)))
    assert out['stats'][0] == float(np.mean(np.broadcast_to(want, (10, 101)).copy())) and abs(out['stats'][0] - (51 + 50 * 2 / 3) / 101) < 1e-12
    assert np.all(out['recall'][:, 0, 0, :] == 1.0)


def test_crowd_matches_are_ignored_not_false_positives():
    # gt 0 is a crowd region of 1000 px, gt 1 an object; detections 0 and 1 lie inside the crowd only, detection 2 is the object
    im = img(1, [[100, 0], [80, 0], [0, 100]], [100, 80, 100], [1000, 100], [0.9, 0.8, 0.7], [0] * 3, [0] * 2, crowd=[1, 0])
    e = R.evaluate_img(im['tables'], im['dt_scores'], im['dt_labels'], im['gt_labels'], im['gt_iscrowd'], None, 0, R.COCO_AREAS[0], R.COCO_THRS, 100)
    assert e['npig'] == 1 and all(row == [True, True, True] for row in e['matched']) and all(row == [True, True, False] for row in e['ignored'])
    assert all(row == [0, 0, 1] for row in e['gt_of'])                      # both on the one crowd region: it is never used up
    out = R.evaluate([im], 1)
    assert np.all(out['precision'][:, :, 0, 0, 2] == ONE) and out['npig'][0, 0] == 1
    # the crowd alone: nothing is counted
    alone = R.evaluate([img(1, [[100]], [100], [1000], [0.9], [0], [0], crowd=[1])], 1)
    assert np.all(alone['precision'] == -1) and alone['npig'].sum() == 0 and alone['stats'][0] == -1.0
    # the stated deviation: I = 0 against a crowd is IoU 0 with no division, also for an empty detection
    assert R.iou_of(0, 0, 1000, True) == 0.0 and R.iou_of(0, 0, 0, False) == 0.0


def test_every_matching_rule_by_hand():
    for name, case in match_cases().items():
        im, want = case['image'], case['want']
        e = R.evaluate_img(im['tables'], im['dt_scores'], im['dt_labels'], im['gt_labels'], im['gt_iscrowd'], im['gt_area'], 0, case['area'],
                           case['thrs'], case.get('max_det', 100))
        for key, value in want.items():
            assert e[key] == value, (name, key, e[key], value)


def test_area_ranges_on_a_30_by_30_ground_truth():
    # 900 px: small.  In the medium range the ground truth is ignored and so is the detection matched to it; the unmatched second
    # detection (900 px, outside the medium range) is ignored there too, and a false positive in `all` and `small`
    im = img(1, [[900], [0]], [900, 900], [900], [0.9, 0.8], [0, 0], [0])
    out = R.evaluate([im], 1)
    assert out['npig'].tolist() == [[1, 1, 0, 0]]
    assert np.all(out['precision'][:, :, 0, 2:, :] == -1) and np.all(out['precision'][:, :, 0, :2, :] == ONE)
    for a, ig in ((0, [False, False]), (1, [False, False]), (2, [True, True]), (3, [True, True])):
        e = R.evaluate_img(im['tables'], im['dt_scores'], im['dt_labels'], im['gt_labels'], [0], None, 0, R.COCO_AREAS[a], R.COCO_THRS, 100)
        assert all(row == ig for row in e['ignored']) and all(row == [True, False] for row in e['matched']), a
    # the annotation's area decides, not the pixel count: 1100 (medium) for the same 900 px
    e = R.evaluate_img(im['tables'], im['dt_scores'], im['dt_labels'], im['gt_labels'], [0], [1100.0], 0, R.COCO_AREAS[2], R.COCO_THRS, 100)
    assert e['npig'] == 1 and all(row == [False, True] for row in e['ignored'])


def test_rank_beyond_max_det_is_dropped():
    # the better-scored detection is a false positive, the second one the true positive: at maxDet = 1 only the first is seen
    out = R.evaluate([img(1, [[0], [100]], [100, 100], [100], [0.9, 0.8], [0, 0], [0])], 1, max_dets=(1, 10, 100))
    assert np.all(out['recall'][:, 0, 0, 0] == 0.0) and np.all(out['recall'][:, 0, 0, 1:] == 1.0)
    assert np.all(out['precision'][:, :, 0, 0, 0] == 0.0) and np.all(out['precision'][:, :, 0, 0, 1] == 1.0 / (1.0 + 1.0 + EPS))
    assert out['stats'][6] == 0.0 and out['stats'][7] == out['stats'][8] == 1.0


def test_images_without_ground_truth_and_without_detections():
    ims = [img(3, np.zeros((1, 0)), [100], [], [0.95], [0], []),                      # no ground truth: its detection is a false positive
           img(1, np.zeros((0, 1)), [], [100], [], [], [0]),                          # no detection: its ground truth counts
           img(2, [[100]], [100], [100], [0.9], [0], [0])]
    out = R.evaluate(ims, 2)
    assert out['npig'].tolist() == [[2, 2, 0, 0], [0, 0, 0, 0]] and np.all(out['precision'][:, :, 1] == -1) and np.isnan(out['classwise'][1])
    # sorted by score: FP (0.95), TP (0.9): recall 1/2, precision 1/2 up to recall 0.5, nothing beyond
    want = np.array([1.0 / (1.0 + 1.0 + EPS)] * 51 + [0.0] * 50)
    assert np.array_equal(out['precision'][:, :, 0, 0, 2], np.broadcast_to(want, (10, 101))) and np.all(out['recall'][:, 0, 0, 2] == 0.5)
    # the order in which the images arrive does not matter
    again = R.evaluate(ims[::-1], 2)
    assert np.array_equal(again['precision'], out['precision']) and again['stats'] == out['stats']


def test_overlaps_count_pixels():
    dt = np.zeros((2, 5, 70), bool)
    gt = np.zeros((1, 5, 70), bool)
    dt[0, 1:3, 60:68], dt[1, :, :], gt[0, 2:5, 62:70] = True, True, True
    inter, ad, ag = R.overlaps(dt, gt)
    assert inter.tolist() == [[6], [24]] and ad.tolist() == [16, 350] and ag.tolist() == [24]
    assert R.overlaps(dt[:0], gt)[0].shape == (0, 1) and R.overlaps(dt, gt[:0])[0].shape == (2, 0)
    assert P == 101
