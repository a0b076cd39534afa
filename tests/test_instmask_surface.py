"""The Python surface of the fused instance-mask rescale, on the CPU: the new keyword paths default to today's behaviour, CPU tensors
take the torch path, and `get_seg_masks_tracking_rle` packs like mmtrack's `outs2results` (ids in front of the box rows, detections with
id < 0 dropped before anything is encoded).  The device encoder is replaced by tests/rle_ref.py here; tests/test_gpu_instmask.py runs the
real one."""
import inspect

import numpy as np
import pytest
import torch

import instmask_ref as R
import rle_ref


class _HostEncoder:
    """stands in for `mask_rle.MaskRLE` on the CPU: the reference encoder on `masks > thr`; records what it was asked"""

    def __init__(self, vkn):
        self.vkn, self.calls = vkn, []

    def __call__(self, masks, thr=None):
        self.calls.append(('call', tuple(masks.shape)))
        m = (masks > thr) if thr is not None else masks.bool()
        return [rle_ref.encode(x) for x in m.numpy()]

    def encode_logits(self, logits, img_meta, thr, rows=None, up=1):
        self.calls.append(('encode_logits', None if rows is None else [int(r) for r in rows]))
        sel = logits if rows is None else logits[torch.as_tensor(rows).long()]
        return self(self.vkn.ops.rescale_masks_torch(sel, img_meta, up), thr)


@pytest.fixture
def host_encoder(vkn, monkeypatch):
    enc = _HostEncoder(vkn)
    monkeypatch.setattr(vkn.mask_rle, 'default_encoder', lambda: enc)
    return enc


def _head(vkn, video):
    cls = vkn.KernelUpdateHeadVideo if video else vkn.KernelUpdateHead
    head = cls.__new__(cls)
    head.num_classes = 3
    return head


def test_keyword_defaults(vkn):
    for cls in (vkn.KernelUpdateHead, vkn.KernelUpdateHeadVideo):
        p = inspect.signature(cls.get_seg_masks_tracking_rle).parameters
        assert p['fused_rescale'].default is False and list(p)[-1] == 'fused_rescale', cls
        # `get_seg_masks_rle` keeps `get_seg_masks`'s parameter list (tests/test_rle_surface.py pins it): the fused path is a method beside it
        assert list(inspect.signature(cls.get_seg_masks_rle_fused).parameters) == list(inspect.signature(cls.get_seg_masks_rle).parameters) == list(inspect.signature(cls.get_seg_masks).parameters)
        assert list(inspect.signature(cls.get_seg_masks_tracking_rle).parameters)[:7] == list(inspect.signature(cls.get_seg_masks_tracking).parameters)
    for fn in (vkn.ops.instance_mask_bits, vkn.MaskRLE.encode_logits, vkn.MaskAPMeter.update_logits):
        p = inspect.signature(fn).parameters
        assert p['rows'].default is None and p['up'].default == 1, fn
    assert list(inspect.signature(vkn.ops.instance_mask_bits).parameters)[:5] == ['logits', 'img_meta', 'thr', 'rows', 'up']
    assert list(inspect.signature(vkn.MaskAPMeter.update_logits).parameters)[1:7] == ['image_id', 'logits', 'img_meta', 'thr', 'dt_scores', 'dt_labels']


@pytest.mark.parametrize('name', ['crop_down', 'strong_down', 'strip_128'])
def test_cpu_tensors_take_the_torch_path(vkn, name):
    c = R.partition(name)
    assert not vkn.ops.instance_bits_fused(c['logits'], c['meta'], 5, c['up'])
    bits = vkn.ops.instance_mask_bits(c['logits'], c['meta'], 0.5, up=c['up'])
    Ho, Wo = c['geom'][5]
    assert bits.dtype == torch.int64 and tuple(bits.shape) == (5, R.strips_of(Wo), Ho) and not bits.is_cuda
    got, tail = R.unpack_bits(bits.numpy(), Wo)
    assert not tail and np.array_equal(got, c['mask'])
    rows = [3, 0, 3]
    got, _ = R.unpack_bits(vkn.ops.instance_mask_bits(c['logits'], c['meta'], 0.5, rows=rows, up=c['up']).numpy(), Wo)
    assert np.array_equal(got, c['mask'][rows])
    assert tuple(vkn.ops.instance_mask_bits(c['logits'], c['meta'], 0.5, rows=[], up=c['up']).shape) == (0, R.strips_of(Wo), Ho)
    # the encoder and the meter have no CPU path of their own: the torch rescale, then the refusal that their existing calls give
    with pytest.raises(vkn.VknLibraryError, match='no CPU fallback'):
        vkn.MaskRLE().encode_logits(c['logits'], c['meta'], 0.5, up=c['up'])
    with pytest.raises(vkn.VknLibraryError, match='no CPU fallback'):
        vkn.MaskAPMeter(3).update_logits(0, c['logits'], c['meta'], 0.5, torch.ones(5), torch.zeros(5), torch.zeros((1, Ho, Wo), dtype=torch.bool), torch.zeros(1))
    assert vkn.MaskRLE().encode_logits(c['logits'][:0], c['meta'], 0.5, up=c['up']) == []


@pytest.mark.parametrize('video', [False, True])
@pytest.mark.parametrize('fused', [False, True])
def test_tracking_rle_packs_like_outs2results(vkn, host_encoder, video, fused):
    c = R.partition('strong_down')                     # up = 1: what the heads hand on
    head = _head(vkn, video)
    labels, scores = torch.tensor([0, 2, 1, 0, 2]), torch.linspace(0.9, 0.5, 5)
    ids = torch.tensor([4, -1, 0, 7, -1])
    cfg = dict(mask_thr=0.5)
    bbox, segm = head.get_seg_masks_tracking_rle(c['logits'], labels, scores, ids, cfg, c['meta'], fused_rescale=fused)
    # against the mask path: the same boxes, and the RLE of every mask that `outs2results` kept, class by class in the same order
    bbox0, segm0 = head.get_seg_masks_tracking(c['logits'], labels, scores, ids, cfg, c['meta'])
    assert len(bbox) == len(bbox0) == 3 and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(bbox, bbox0))
    assert segm == [[rle_ref.encode(m) for m in cls] for cls in segm0]
    assert [r[:, 0].tolist() for r in bbox] == [[4.0, 7.0], [0.0], []] and [len(s) for s in segm] == [2, 1, 0]
    keep = [0, 2, 3]
    assert host_encoder.calls[0] == (('encode_logits', keep) if fused else ('call', (3, 20, 33)))      # dropped ids are never rescaled or encoded
    tracks = vkn.knet_vis.outs2results(bboxes=torch.cat([torch.zeros(5, 4), scores[:, None]], 1), labels=labels, masks=torch.from_numpy(c['mask']), ids=ids, num_classes=3)
    assert all(np.array_equal(a, b) for a, b in zip(bbox, tracks['bbox_results']))
    assert segm == [[rle_ref.encode(m) for m in cls] for cls in tracks['mask_results']]
    # every id dropped: nothing is encoded
    host_encoder.calls.clear()
    bbox, segm = head.get_seg_masks_tracking_rle(c['logits'], labels, scores, torch.full((5,), -1), cfg, c['meta'], fused_rescale=fused)
    assert segm == [[], [], []] and all(b.shape == (0, 6) for b in bbox) and not host_encoder.calls


@pytest.mark.parametrize('video', [False, True])
def test_get_seg_masks_rle_default_is_the_unfused_call(vkn, host_encoder, video):
    c = R.partition('strong_down')
    head = _head(vkn, video)
    labels, scores = torch.tensor([0, 2, 1, 0, 2]), torch.linspace(0.9, 0.5, 5)
    d = head.get_seg_masks_rle(c['logits'], labels, scores, dict(mask_thr=0.5), c['meta'])
    f = head.get_seg_masks_rle_fused(c['logits'], labels, scores, dict(mask_thr=0.5), c['meta'])
    assert [k for k, _ in host_encoder.calls] == ['call', 'encode_logits', 'call']
    want = [rle_ref.encode(m) for m in c['mask']]
    assert d[1] == f[1] == [[want[0], want[3]], [want[2]], [want[1], want[4]]] and all(np.array_equal(a, b) for a, b in zip(d[0], f[0]))
