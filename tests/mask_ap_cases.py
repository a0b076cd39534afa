"""Hand-built images for the mask-AP tests: integer overlap tables instead of masks, so that every rule of include/vkn_maskap.h can be
set up exactly.  tests/test_maskap_refs.py runs them through tests/maskap_ref.py, tests/test_gpu_maskap.py through the C ABI."""
import numpy as np

EPS = np.spacing(1)
P = 101


def img(image_id, inter, area_dt, area_gt, scores, dt_labels, gt_labels, crowd=None, area=None):
    """an image dict as maskap_ref.evaluate takes it, with `tables` given by hand"""
    K, G = len(area_dt), len(area_gt)
    tables = (np.asarray(inter, dtype=np.int64).reshape(K, G), np.asarray(area_dt, dtype=np.int64).reshape(K), np.asarray(area_gt, dtype=np.int64).reshape(G))
    return dict(image_id=image_id, tables=tables, dt_scores=np.asarray(scores, dtype=np.float32).reshape(K), dt_labels=np.asarray(dt_labels, dtype=np.int32).reshape(K),
                gt_labels=np.asarray(gt_labels, dtype=np.int32).reshape(G), gt_iscrowd=np.asarray(crowd if crowd is not None else [0] * G, dtype=np.uint8).reshape(G),
                gt_area=np.asarray(area, dtype=np.float64).reshape(G) if area is not None else None)


ALL = (0.0, 1e10)


def match_cases():
    """{name: dict(image, area, thrs, [max_det], want)}: `want` holds the fields of maskap_ref.evaluate_img worked out by hand for
    category 0 (dt: detections in score order; matched, ignored, gt_of: [T][len(dt)])"""
    T, F = True, False
    return {
        # IoU 1/3 with both ground truths: the LATER one is taken, the next detection gets the earlier
        'equal_iou_moves_to_the_later': dict(image=img(1, [[50, 50], [50, 50]], [100, 100], [100, 100], [0.9, 0.8], [0, 0], [0, 0]), area=ALL, thrs=[0.3],
                                             want=dict(dt=[0, 1], gt_of=[[1, 0]], matched=[[T, T]], ignored=[[F, F]], npig=2)),
        # gt 1 is ignored (annotation area 5000 > 1000) and has the higher IoU (380/420 against 300/500): at 0.5 the non-ignored match is
        # kept (the walk stops), at 0.7 only the ignored one qualifies and the detection is ignored with it
        'break_keeps_the_non_ignored_match': dict(image=img(1, [[300, 380]], [400], [400, 400], [0.9], [0], [0, 0], area=[500.0, 5000.0]), area=(0.0, 1000.0),
                                                  thrs=[0.5, 0.7], want=dict(dt=[0], gt_of=[[0], [1]], matched=[[T], [T]], ignored=[[F], [T]], npig=1)),
        # I / U = 1/2 and 3/4 exactly: matched at 0.5 and 0.75, not a hair above
        'iou_exactly_at_the_threshold': dict(image=img(1, [[1, 0], [0, 3]], [2, 4], [1, 3], [0.9, 0.8], [0, 0], [0, 0]), area=ALL, thrs=[0.5, 0.75, 0.5000001, 0.7500001],
                                             want=dict(dt=[0, 1], gt_of=[[0, 1], [-1, 1], [-1, 1], [-1, -1]], matched=[[T, T], [F, T], [F, T], [F, F]],
                                                       ignored=[[F, F]] * 4, npig=2)),
        # threshold 1.0 is min(1, 1 - 1e-10): IoU 1 matches, 99/100 does not
        'iou_one_at_threshold_one': dict(image=img(1, [[100, 0], [0, 99]], [100, 100], [100, 99], [0.9, 0.8], [0, 0], [0, 0]), area=ALL, thrs=[1.0],
                                         want=dict(dt=[0, 1], gt_of=[[0, -1]], matched=[[T, F]], ignored=[[F, F]], npig=2)),
        # three detections of one score on one ground truth: input order is kept, the first takes it
        'tied_scores_keep_input_order': dict(image=img(1, [[100], [100], [100]], [100] * 3, [100], [0.5, 0.5, 0.5], [0] * 3, [0]), area=ALL, thrs=[0.5, 0.9],
                                             want=dict(dt=[0, 1, 2], gt_of=[[0, -1, -1]] * 2, matched=[[T, F, F]] * 2, ignored=[[F, F, F]] * 2, npig=1)),
        # medium range: the unmatched 900 px detection is outside it and ignored; the 2000 px one inside is a false positive
        'unmatched_outside_the_range_is_ignored': dict(image=img(1, [[0], [0]], [900, 2000], [2000], [0.9, 0.8], [0, 0], [0]), area=(1024.0, 9216.0), thrs=[0.5],
                                                       want=dict(dt=[0, 1], gt_of=[[-1, -1]], matched=[[F, F]], ignored=[[T, F]], npig=1)),
        # a 30 x 30 ground truth in the medium range: ignored, and so is the detection matched to it
        'small_ground_truth_in_the_medium_range': dict(image=img(1, [[900]], [900], [900], [0.9], [0], [0]), area=(1024.0, 9216.0), thrs=[0.5, 0.95],
                                                       want=dict(dt=[0], gt_of=[[0], [0]], matched=[[T], [T]], ignored=[[T], [T]], npig=0)),
        # two detections inside one crowd region (IoU = I / area_dt), one object beside it; detection 3 belongs to category 1
        'crowd_is_shared_and_ignored': dict(image=img(1, [[100, 0], [80, 0], [0, 100], [0, 100]], [100, 80, 100, 100], [1000, 100], [0.9, 0.8, 0.7, 0.95], [0, 0, 0, 1],
                                                      [0, 0], crowd=[1, 0]), area=ALL, thrs=[0.5, 0.95],
                                            want=dict(dt=[0, 1, 2], gt_of=[[0, 0, 1]] * 2, matched=[[T, T, T]] * 2, ignored=[[T, T, F]] * 2, npig=1)),
        # the first max_det in score order are kept
        'max_det_keeps_the_best': dict(image=img(1, [[100], [100], [0]], [100] * 3, [100], [0.1, 0.9, 0.5], [0] * 3, [0]), area=ALL, thrs=[0.5], max_det=2,
                                       want=dict(dt=[1, 2], gt_of=[[0, -1]], matched=[[T, F]], ignored=[[F, F]], npig=1)),
    }
