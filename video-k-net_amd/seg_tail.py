"""The dense semantic loss of the kernel-initialisation head without the up-scaled logits (include/vkn_seg_loss.h).

The reference's `ConvKernelHead.forward_train` (knet/det/kernel_head.py:278-292, 404-426, 446-462) up-scales the semantic logits
[B, ncls, h, w] by `feat_downsample_stride`, paints `seg_targets` per image, makes a contiguous [B S h S w, ncls] copy and runs
`loss_seg` on it.  `SegLossTail` computes the same `loss_rpn_seg`, and its gradient w.r.t. the LOW-RES logits, from

  `targets`   one launch: the painted map as one byte per pixel, straight from the step's ground truth and the assigner's `gt_inds`
              (no `nonzero`, no gather of matched masks, no host read) + the number of dense positives as a device integer;
  `loss`      `autograd.SegLossFn`: two launches forward, one backward; every up-scaled logit exists in registers only.

It restates the two losses the shipped configs build, checked BY VALUE as `train_tail._shipped_losses` does: the sigmoid focal loss
(this package's or mmdet's `FocalLoss(use_sigmoid=True, reduction='mean')`) and the soft-max `CrossEntropyLoss(use_sigmoid=False,
use_mask=False, class_weight=None, reduction='mean')` of knet/cross_entropy_loss.py.  With any other loss module, or outside the kernels'
envelope (`ops.seg_loss_supported`), both methods run the torch composition of `ConvKernelHead` — same values as without this class —
and `.fused` says which path ran last."""
import torch
import torch.nn.functional as F

from . import autograd as vag
from . import ops


def _focal_by_value(ls):
    from . import losses as L
    if type(ls) is not L.FocalLoss and not (type(ls).__name__ == 'FocalLoss' and type(ls).__module__.startswith('mmdet.')):
        return False
    try:
        return (ls.use_sigmoid is True and ls.reduction == 'mean' and not getattr(ls, 'activated', False) and float(ls.gamma) >= 0.0
                and 0.0 <= float(ls.alpha) <= 1.0 and float(ls.loss_weight) == float(ls.loss_weight))
    except (AttributeError, TypeError, ValueError):
        return False


def _softmax_ce_by_value(ls):
    """ours, or the reference's own class (registered over mmdet's under real mmdet): same constructor arguments, same formula"""
    from . import losses as L
    if type(ls) is not L.CrossEntropyLoss and type(ls).__name__ != 'CrossEntropyLoss':
        return False
    try:
        return (not ls.use_sigmoid and not ls.use_mask and ls.class_weight is None and ls.reduction == 'mean'
                and float(ls.loss_weight) == float(ls.loss_weight))
    except (AttributeError, TypeError, ValueError):
        return False


def paint_targets(shape, num_classes, device, gt_sem_seg, gt_sem_cls, gt_masks, gt_labels, gt_inds):
    """`seg_targets` of one image as torch ops (int64 [H, W]): the stuff masks in order, then the matched instances in the order of
    their proposals; the last layer covering a pixel wins — `ConvKernelHead._image_targets`' masked arg-max."""
    layers, labels = [], []
    if gt_sem_cls is not None and gt_sem_seg is not None and len(gt_sem_cls) > 0:
        layers.append(gt_sem_seg.to(device).bool())
        labels.append(gt_sem_cls.to(device).long())
    pos = torch.nonzero(gt_inds > 0, as_tuple=False).squeeze(-1)
    if pos.numel() > 0:
        g = gt_inds[pos] - 1
        layers.append(gt_masks[g].bool())
        labels.append(gt_labels[g].long())
    if not layers:
        return torch.full(tuple(shape), num_classes, dtype=torch.long, device=device)
    stack, lab = torch.cat(layers), torch.cat(labels)
    order = torch.arange(stack.shape[0], device=device, dtype=torch.int32).view(-1, 1, 1)
    top = torch.where(stack, order, order.new_full((), -1)).amax(dim=0).long()
    return torch.where(top >= 0, lab[top.clamp(min=0)], lab.new_full((), num_classes))


def composed_loss(loss_seg, seg_preds_lowres, seg_targets, num_classes, stride):
    """`loss_rpn_seg` as `ConvKernelHead.forward_train` + `.loss` compose it (knet/det/kernel_head.py:278-292, 404-426)."""
    seg = seg_preds_lowres
    if stride > 1:
        seg = F.interpolate(seg, scale_factor=stride, mode='bilinear', align_corners=False)
    ch = seg.shape[1]
    flat = seg.view(-1, ch, seg.shape[-2] * seg.shape[-1]).permute(0, 2, 1).reshape(-1, ch)
    tgt = seg_targets.reshape(-1).long()
    if loss_seg.use_sigmoid:
        dense_pos = ((tgt >= 0) & (tgt < num_classes)).sum().float().clamp(min=1.0)
        return loss_seg(flat, tgt, avg_factor=dense_pos)
    return loss_seg(flat, tgt, ignore_index=num_classes)


class SegLossTail:

    def __init__(self, num_classes, stride, loss_seg):
        self.num_classes, self.loss_seg = int(num_classes), loss_seg
        self.stride = int(stride) if int(stride) == stride else stride      # a non-integer stride is the composition's
        self.mode = (ops.SEG_LOSS_FOCAL if _focal_by_value(loss_seg) else ops.SEG_LOSS_CE if _softmax_ce_by_value(loss_seg) else None)
        self.fused = False

    # -------------------------------------------------------------------------------------------------------------------------
    def _shapes_ok(self, B, H, W, device):
        S = self.stride
        return (self.mode is not None and device.type == 'cuda' and isinstance(S, int) and S >= 1 and H % S == 0 and W % S == 0
                and ops.seg_loss_supported(B, self.num_classes, H // S, W // S, S))

    def targets(self, gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, assign_results):
        """The dense target map of the batch: uint8 [B, H, W] on the fused path (background / ignore = num_classes), int64 [B, H, W]
        as `get_targets` returns it otherwise.  gt_masks: per image [G_b, H, W] at the up-scaled size; assign_results: per image the
        assigner's result (or its `gt_inds` tensor)."""
        gt_inds = [getattr(a, 'gt_inds', a) for a in assign_results]
        B = len(gt_masks)
        H, W = (int(v) for v in gt_masks[0].shape[-2:])
        dev = gt_inds[0].device
        ok = (self._shapes_ok(B, H, W, dev) and all(g.dtype == torch.int64 and g.numel() <= ops.SEG_MAX_ROWS for g in gt_inds)
              and all(torch.is_tensor(m) and m.is_cuda and m.dim() == 3 and tuple(m.shape[1:]) == (H, W) and m.shape[0] <= ops.SEG_MAX_ROWS
                      for m in gt_masks))
        if gt_sem_seg is not None and gt_sem_cls is not None:
            ok = ok and all(s is None or c is None or c.numel() == 0 or (torch.is_tensor(s) and s.is_cuda and tuple(s.shape) == (c.numel(), H, W)
                                                                         and c.numel() <= ops.SEG_MAX_ROWS)
                            for s, c in zip(gt_sem_seg, gt_sem_cls))
        if not ok:
            self.fused = False
            sem = gt_sem_seg if gt_sem_seg is not None and gt_sem_cls is not None else [None] * B
            cls = gt_sem_cls if gt_sem_seg is not None and gt_sem_cls is not None else [None] * B
            return torch.stack([paint_targets((H, W), self.num_classes, dev, sem[b], cls[b], gt_masks[b], gt_labels[b], gt_inds[b])
                                for b in range(B)], 0)
        masks = [m if m.dtype == torch.float32 else m.float() for m in gt_masks]
        sem = None
        if gt_sem_seg is not None and gt_sem_cls is not None:
            sem = [None if s is None else (s if s.dtype == torch.float32 else s.float()) for s in gt_sem_seg]
        labels = [l.long() for l in gt_labels]
        cls = None if sem is None else [None if c is None else c.to(dev).long() for c in gt_sem_cls]
        tgt, dense_pos = ops.seg_targets(masks, labels, sem, cls, gt_inds, self.num_classes, (H, W))
        tgt._vkn_dense_pos = dense_pos
        self.fused = True
        return tgt

    def loss(self, seg_preds_lowres, targets):
        """`loss_rpn_seg` (0-d, with autograd to the low-res logits) from seg_preds_lowres [B, ncls, h, w] and the map of `targets`."""
        B, ncls, h, w = (int(v) for v in seg_preds_lowres.shape)
        S = self.stride
        ok = (targets.dtype == torch.uint8 and ncls == self.num_classes and seg_preds_lowres.dtype == torch.float32
              and isinstance(S, int) and tuple(targets.shape) == (B, S * h, S * w) and self._shapes_ok(B, S * h, S * w, seg_preds_lowres.device))
        if not ok:
            self.fused = False
            return composed_loss(self.loss_seg, seg_preds_lowres, targets, self.num_classes, S)
        dense_pos = getattr(targets, '_vkn_dense_pos', None)
        if dense_pos is None and self.mode == ops.SEG_LOSS_FOCAL:           # a map of the caller's own
            dense_pos = (targets < self.num_classes).sum().to(torch.int32).reshape(1)
        ls = self.loss_seg
        alpha, gamma = (float(ls.alpha), float(ls.gamma)) if self.mode == ops.SEG_LOSS_FOCAL else (0.0, 0.0)
        self.fused = True
        return vag.seg_loss(seg_preds_lowres, targets, dense_pos, self.mode, S, alpha, gamma, float(ls.loss_weight))
