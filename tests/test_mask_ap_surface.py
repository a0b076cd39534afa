"""The Python surface of the mask-AP meter, as far as a machine without a GPU sees it: `MaskAPMeter` is exported with COCO's defaults,
refuses what is outside the envelope and host tensors like every op, names its stats as mmdet does, and both instance heads carry
`get_seg_masks_device` with `get_seg_masks`' parameters while every existing method keeps its signature."""
import inspect

import numpy as np
import pytest
import torch


def test_export_and_constructor_defaults(vkn):
    assert vkn.MaskAPMeter is vkn.mask_ap_meter.MaskAPMeter
    m = vkn.MaskAPMeter(80)
    assert m.num_classes == 80 and m.max_dets == (100, 300, 1000) and m.capacity == 1 << 20 and m.device is None
    assert np.array_equal(m.iou_thrs, np.arange(0.5, 0.96, 0.05)) and m.iou_thrs.dtype == np.float64 and len(m.iou_thrs) == 10
    assert m.area_ranges == ((0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10)) == vkn.mask_ap_meter.COCO_AREA_RANGES
    want = ['self', 'num_classes', 'iou_thrs', 'max_dets', 'area_ranges', 'capacity', 'device']
    assert list(inspect.signature(vkn.MaskAPMeter.__init__).parameters) == want
    assert list(inspect.signature(vkn.MaskAPMeter.update).parameters) == ['self', 'image_id', 'dt_masks', 'dt_scores', 'dt_labels', 'gt_masks', 'gt_labels',
                                                                          'gt_iscrowd', 'gt_area', 'thr']
    assert list(inspect.signature(vkn.ops.mask_overlap).parameters) == ['dt', 'gt', 'thr', 'out']
    # nothing was updated: no state, no device, empty tables, and a result without a number in it
    c, r = m.counts(), m.records()
    assert c['records'] == 0 and c['status'] == 0 and c['npig'].shape == (80, 4) and not c['npig'].any()
    assert all(len(r[k]) == 0 for k in ('image', 'label', 'score', 'rank')) and r['matched'].shape == (0, 4) == r['ignored'].shape
    out = m.result()
    assert out['precision'].shape == (10, 101, 80, 4, 3) and out['recall'].shape == (10, 80, 4, 3) and np.all(out['precision'] == -1) and np.all(out['recall'] == -1)
    assert all(v == -1.0 for v in out['stats'].values()) and np.isnan(out['classwise']).all()
    m.check_status()
    m.reset()


def test_stats_carry_mmdets_names(vkn):
    names = ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l', 'AR@100', 'AR@300', 'AR@1000', 'AR_s@1000', 'AR_m@1000', 'AR_l@1000')
    assert vkn.mask_ap_meter.stats_names((100, 300, 1000)) == names and tuple(vkn.MaskAPMeter(3).result()['stats']) == names
    assert vkn.mask_ap_meter.stats_names((1, 10, 100))[6:] == ('AR@1', 'AR@10', 'AR@100', 'AR_s@100', 'AR_m@100', 'AR_l@100')
    assert vkn.MaskAPMeter(3, area_ranges=((0, 1e10),)).result()['stats'] == {}              # COCO's twelve need its four ranges and three maxDets


def test_refusals(vkn):
    for kw in (dict(num_classes=0), dict(num_classes=257), dict(num_classes=3, max_dets=()), dict(num_classes=3, max_dets=(100, 10)), dict(num_classes=3, max_dets=(0, 1)),
               dict(num_classes=3, max_dets=(1, 1025)), dict(num_classes=3, iou_thrs=()), dict(num_classes=3, iou_thrs=[0.5] * 17), dict(num_classes=3, area_ranges=()),
               dict(num_classes=3, area_ranges=((0, 1),) * 5), dict(num_classes=3, capacity=0), dict(num_classes=3, capacity=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            vkn.MaskAPMeter(**kw)
    m = vkn.MaskAPMeter(3)
    masks, gts = torch.zeros((2, 5, 7), dtype=torch.bool), torch.zeros((1, 5, 7), dtype=torch.bool)
    with pytest.raises(vkn.VknLibraryError):
        m.update(0, masks, torch.zeros(2), torch.zeros(2, dtype=torch.int64), gts, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(vkn.VknLibraryError):
        vkn.ops.mask_overlap(masks, gts)
    with pytest.raises(vkn.VknLibraryError):
        vkn.ops.mask_overlap(torch.zeros((2, 5, 7)), gts, thr=0.5)
    assert m.counts()['records'] == 0
    # the envelope reaches Python through the size query
    assert vkn.ops.mask_overlap_workspace_bytes(3, 2, 5, 131) == 368 + 240 and vkn.ops.mask_overlap_workspace_bytes(1025, 1, 1, 1) == 0
    with pytest.raises(vkn.VknError):
        vkn.ops.mask_ap_cfg(3, [0.5], [(0, 1e10)], 2000, 64)


def test_both_heads_have_the_method_with_get_seg_masks_parameters(vkn):
    want = ['self', 'masks_per_img', 'labels_per_img', 'scores_per_img', 'test_cfg', 'img_meta']
    for cls in (vkn.KernelUpdateHead, vkn.KernelUpdateHeadVideo, vkn.VideoKernelUpdateHead):
        assert list(inspect.signature(cls.get_seg_masks_device).parameters) == list(inspect.signature(cls.get_seg_masks).parameters) == want, cls
        assert list(inspect.signature(cls.get_seg_masks_rle).parameters) == want, cls
    assert 'get_seg_masks_device' in vars(vkn.KernelUpdateHead) and 'get_seg_masks_device' in vars(vkn.KernelUpdateHeadVideo)
    assert list(inspect.signature(vkn.KernelUpdateHead.segm2result).parameters) == ['self', 'mask_preds', 'det_labels', 'cls_scores']


def test_constants_reach_python(vkn):
    C = vkn._lib.MASKAP
    assert C['VKN_MASKAP_RECORD_INTS'] == C['VKN_MASKAP_REC_WORDS'] + 2 * C['VKN_MASKAP_MAX_AREAS'] == 12 and C['VKN_MASKAP_MAX_THRS'] == 16
    cfg = vkn.ops.mask_ap_cfg(3, np.arange(0.5, 0.96, 0.05), vkn.mask_ap_meter.COCO_AREA_RANGES, 1000, 1 << 20)
    assert (cfg.num_classes, cfg.T, cfg.A, cfg.max_det, cfg.cap_records) == (3, 10, 4, 1000, 1 << 20)
    assert list(cfg.iou_thrs)[:10] == np.arange(0.5, 0.96, 0.05).tolist() and list(cfg.area_hi) == [1e10, 1024.0, 9216.0, 1e10]
    nbytes, off = vkn.ops.mask_ap_layout(cfg)
    assert off == [0, 256, 256 + 96] and nbytes == off[2] + 48 * (1 << 20)
