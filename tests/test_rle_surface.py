"""The Python surface of the device run-length encoder, as far as a machine without a GPU sees it: `MaskRLE` and `encode_mask_results`
are exported and refuse host tensors like every op, K = 0 needs neither a launch nor the library, and both instance heads carry
`get_seg_masks_rle` with `get_seg_masks`' parameters while every existing method keeps its signature."""
import inspect

import pytest
import torch


def test_exports_and_cpu_tensors_are_refused(vkn):
    assert vkn.MaskRLE is vkn.mask_rle.MaskRLE and vkn.encode_mask_results is vkn.mask_rle.encode_mask_results
    enc = vkn.MaskRLE()
    for t in (torch.zeros((2, 5, 7), dtype=torch.bool), torch.zeros((2, 5, 7), dtype=torch.uint8)):
        with pytest.raises(vkn.VknLibraryError):
            enc(t)
    with pytest.raises(vkn.VknLibraryError):
        enc(torch.zeros((2, 5, 7)), thr=0.5)
    with pytest.raises(vkn.VknLibraryError):
        vkn.encode_mask_results([[torch.zeros((5, 7), dtype=torch.bool)], []])
    with pytest.raises(vkn.VknLibraryError):
        vkn.ops.rle_encode(torch.zeros((2, 5, 7), dtype=torch.uint8), *[torch.zeros((18,), dtype=torch.int32)] * 2, torch.zeros((8,), dtype=torch.uint8),
                           torch.zeros((1,), dtype=torch.int32), torch.zeros((8,), dtype=torch.uint8))
    with pytest.raises(ValueError):
        enc(torch.zeros((5, 7), dtype=torch.bool))
    with pytest.raises(RuntimeError):
        vkn.MaskRLE().counts()


def test_no_masks_need_no_launch(vkn):
    enc = vkn.MaskRLE()
    assert enc(torch.zeros((0, 720, 1280), dtype=torch.bool)) == [] and enc.device_calls == 0
    assert enc.counts() == [] and enc.counts(uncompressed=True) == [] and enc.areas().shape == (0,) and enc.bboxes().shape == (0, 4)
    assert vkn.encode_mask_results([[], [], []]) == [[], [], []] and vkn.encode_mask_results(([[]], None)) == ([[]], None)


def test_both_heads_have_the_method_with_get_seg_masks_parameters(vkn):
    want = ['self', 'masks_per_img', 'labels_per_img', 'scores_per_img', 'test_cfg', 'img_meta']
    for cls in (vkn.KernelUpdateHead, vkn.KernelUpdateHeadVideo, vkn.VideoKernelUpdateHead):
        assert list(inspect.signature(cls.get_seg_masks_rle).parameters) == list(inspect.signature(cls.get_seg_masks).parameters) == want, cls
    assert 'get_seg_masks_rle' in vars(vkn.KernelUpdateHead) and 'get_seg_masks_rle' in vars(vkn.KernelUpdateHeadVideo)
    # what was there stays as it was
    assert list(inspect.signature(vkn.KernelUpdateHead.segm2result).parameters) == ['self', 'mask_preds', 'det_labels', 'cls_scores']
    assert list(inspect.signature(vkn.KernelUpdateHead.rescale_masks).parameters) == ['self', 'masks_per_img', 'img_meta']
    assert list(inspect.signature(vkn.KernelUpdateHeadVideo.get_seg_masks_tracking).parameters) == want[:4] + ['ids_per_img'] + want[4:]
    assert list(inspect.signature(vkn.KernelIterHead.get_panoptic).parameters) == ['self', 'cls_scores', 'mask_preds', 'test_cfg', 'img_meta']


def test_constants_reach_python(vkn):
    C = vkn._lib.RLE
    assert C['VKN_RLE_STRIP_COLS'] == 64 and C['VKN_RLE_RECORD_INTS'] == C['VKN_RLE_REC_BBOX'] + 4 == 9
    assert vkn.ops.rle_workspace_bytes(1, 1, 1) > 0 and vkn.ops.rle_workspace_bytes(0, 1, 1) == 0 and vkn.ops.rle_workspace_bytes(1025, 1, 1) == 0
