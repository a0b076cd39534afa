"""`MaskAPMeter`: COCO mask AP (`metric=['segm']`) from device masks (include/vkn_maskap.h, csrc/vkn_maskap.hip).

What the reference's `evaluate` reaches through `COCOeval(cocoGt, cocoDt, 'segm')` (external/cityscape_panoptic.py:453-568, the same
text in external/cityscapes_vps.py) is split in two.  `COCOeval.evaluateImg` runs on the device, image by image: the pairwise overlap of
the K detections and G ground truths at full resolution as exact integers, then the greedy matching per (category, area range, IoU
threshold), which leaves one small record per detection in a log in device memory.  `COCOeval.accumulate` and `summarize` are float64
and are restated here on the host, from ONE read of that log.  pycocotools is not a dependency: its rules are restated in
include/vkn_maskap.h, and tests/maskap_ref.py restates them once more, independently, from boolean NumPy masks.

One stated deviation: an intersection of 0 gives IoU 0 without a division (pycocotools divides 0 by 0 for an empty detection against
a crowd region).  Not built: bbox IoU, `useCats = 0`, a YouTube-VIS scorer on top of the tube tables, IoU on RLE strings.
"""
import numpy as np
import torch

from . import _lib, ops

_C = _lib.MASKAP
_REC = _C['VKN_MASKAP_RECORD_INTS']
COCO_AREA_RANGES = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))      # all, small, medium, large
_BITS = (('VKN_MASKAP_STATUS_FULL', 'FULL: the log of records (capacity) overflowed'),
         ('VKN_MASKAP_STATUS_LABEL_RANGE', 'LABEL_RANGE: a label outside [0, num_classes)'),
         ('VKN_MASKAP_STATUS_SCORE_NAN', 'SCORE_NAN: a NaN score'))


def stats_names(max_dets):
    """mmdet's names of COCOeval's twelve stats (external/cityscape_panoptic.py:481-494), for these three maxDets"""
    a, b, c = max_dets
    return ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l', f'AR@{a}', f'AR@{b}', f'AR@{c}', f'AR_s@{c}', f'AR_m@{c}', f'AR_l@{c}')


class MaskAPMeter:
    """num_classes: labels are 0 .. num_classes - 1 (the index into the dataset's cat_ids); iou_thrs, max_dets, area_ranges: COCOeval's
    iouThrs, maxDets and areaRng as the reference sets them; capacity: records of the log, one per detection of every image (default
    2^20); what overflows is reported by `result()` / `check_status()`, never silently.

        meter.update(image_id, dt_masks, dt_scores, dt_labels, gt_masks, gt_labels, gt_iscrowd, gt_area)     # per image, device only
        out = meter.result()      # precision [T,101,C,A,M], recall [T,C,A,M], stats {name: value}, classwise [C]
    """

    def __init__(self, num_classes, iou_thrs=np.arange(0.5, 0.96, 0.05), max_dets=(100, 300, 1000), area_ranges=COCO_AREA_RANGES, capacity=None,
                 device=None):
        self.num_classes = int(num_classes)
        self.iou_thrs = np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
        self.max_dets = tuple(int(m) for m in max_dets)
        self.area_ranges = tuple((float(lo), float(hi)) for lo, hi in area_ranges)
        self.capacity = int(capacity) if capacity is not None else 1 << 20
        if not self.max_dets or list(self.max_dets) != sorted(set(self.max_dets)) or self.max_dets[0] < 1:
            raise ValueError(f'max_dets must be positive and strictly ascending, got {max_dets}')
        if not 1 <= self.num_classes <= _C['VKN_MASKAP_MAX_CLASSES']:
            raise ValueError(f'num_classes must be in 1..{_C["VKN_MASKAP_MAX_CLASSES"]}, got {num_classes}')
        if not 1 <= len(self.iou_thrs) <= _C['VKN_MASKAP_MAX_THRS'] or not 1 <= len(self.area_ranges) <= _C['VKN_MASKAP_MAX_AREAS']:
            raise ValueError(f'1 to {_C["VKN_MASKAP_MAX_THRS"]} IoU thresholds and 1 to {_C["VKN_MASKAP_MAX_AREAS"]} area ranges, got '
                             f'{len(self.iou_thrs)} and {len(self.area_ranges)}')
        if self.max_dets[-1] > _C['VKN_MASKAP_MAX_MASKS'] or not 1 <= self.capacity <= 1 << 24:
            raise ValueError(f'max_dets up to {_C["VKN_MASKAP_MAX_MASKS"]} and a capacity in 1..2^24, got {self.max_dets} and {self.capacity}')
        self.device = torch.device(device) if device is not None else None
        self._cfg = self._state_t = self._layout = None

    # ---- counting: device only
    def _state(self, device):
        if self._state_t is None:
            self._cfg = ops.mask_ap_cfg(self.num_classes, self.iou_thrs, self.area_ranges, self.max_dets[-1], self.capacity)
            self._layout = ops.mask_ap_layout(self._cfg)
            self._state_t = ops.mask_ap_state(self._cfg, torch.device(device))
            self.device = self._state_t.device
        return self._state_t

    def reset(self):
        if self._state_t is not None:
            ops.mask_ap_reset(self._cfg, self._state_t)

    def update(self, image_id, dt_masks, dt_scores, dt_labels, gt_masks, gt_labels, gt_iscrowd=None, gt_area=None, thr=None):
        """One image.  dt_masks bool / uint8 [K,H,W], or float32 with `thr` (set iff v > thr); dt_scores [K]; dt_labels [K]; gt_masks bool /
        uint8 [G,H,W]; gt_labels [G]; gt_iscrowd [G] or None (none is); gt_area [G] or None (the annotation's area; None: the pixel
        count): CUDA tensors.  Two library calls (overlap, match) on the current stream, nothing is read back.  -> the overlap tables."""
        for t, name in ((dt_masks, 'dt_masks'), (gt_masks, 'gt_masks'), (dt_scores, 'dt_scores'), (dt_labels, 'dt_labels'), (gt_labels, 'gt_labels')):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise _lib.VknLibraryError(f'MaskAPMeter.update: {name}: expected a CUDA/HIP tensor — the MI355X path has no CPU fallback')
        dev = dt_masks.device
        state = self._state(self.device if self.device is not None else dev)
        if dev != state.device:
            raise ValueError(f'MaskAPMeter.update: the meter lives on {state.device}, the masks on {dev}')
        return self._match(image_id, ops.mask_overlap(dt_masks, gt_masks, thr=thr), dt_scores, dt_labels, gt_masks, gt_labels, gt_iscrowd, gt_area)

    def update_logits(self, image_id, logits, img_meta, thr, dt_scores, dt_labels, gt_masks, gt_labels, gt_iscrowd=None, gt_area=None, rows=None, up=1):
        """`update` with the detections straight from the head's mask logits: their masks, `rescale_masks(logits[rows]) > thr`, come as
        bits (`ops.instance_mask_bits`, include/vkn_instmask.h) and only the ground truths are packed (vkn_bits_mask_overlap).  logits
        float32 [N,Hm,Wm]: with up = 1 the scaled mask predictions, with up in (2, 4) the stride-8 logits; rows: the K detections' rows
        (None: every row); dt_scores, dt_labels [K].  Geometries outside the kernel's envelope take the torch rescale and `update`."""
        for t, name in ((logits, 'logits'), (gt_masks, 'gt_masks'), (dt_scores, 'dt_scores'), (dt_labels, 'dt_labels'), (gt_labels, 'gt_labels')):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise _lib.VknLibraryError(f'MaskAPMeter.update_logits: {name}: expected a CUDA/HIP tensor — the MI355X path has no CPU fallback')
        if rows is not None:
            rows = torch.as_tensor(rows, device=logits.device).reshape(-1)
        K = int(logits.shape[0]) if rows is None else int(rows.numel())
        if K == 0:
            empty = torch.zeros((0, *(int(v) for v in img_meta['ori_shape'][:2])), dtype=torch.bool, device=logits.device)
            return self.update(image_id, empty, dt_scores, dt_labels, gt_masks, gt_labels, gt_iscrowd, gt_area)
        if not ops.instance_bits_fused(logits, img_meta, K, up):
            sel = logits if rows is None else logits.index_select(0, rows.long())
            return self.update(image_id, ops.rescale_masks_torch(sel.float(), img_meta, up), dt_scores, dt_labels, gt_masks, gt_labels, gt_iscrowd, gt_area,
                               thr=float(thr))
        dev = logits.device
        state = self._state(self.device if self.device is not None else dev)
        if dev != state.device:
            raise ValueError(f'MaskAPMeter.update_logits: the meter lives on {state.device}, the logits on {dev}')
        bits = ops.instance_mask_bits(logits, img_meta, thr, rows=rows, up=up)
        tables = ops.mask_overlap_bits(bits, int(img_meta['ori_shape'][1]), gt_masks)
        return self._match(image_id, tables, dt_scores, dt_labels, gt_masks, gt_labels, gt_iscrowd, gt_area)

    def _match(self, image_id, tables, dt_scores, dt_labels, gt_masks, gt_labels, gt_iscrowd, gt_area):
        dev, state = gt_masks.device, self._state_t
        G = int(gt_masks.shape[0])
        crowd = gt_iscrowd.to(device=dev, dtype=torch.uint8) if gt_iscrowd is not None else torch.zeros((G,), dtype=torch.uint8, device=dev)
        area = gt_area.to(device=dev, dtype=torch.float64) if gt_area is not None else None
        ops.mask_ap_match(self._cfg, state, tables, dt_scores.to(torch.float32), dt_labels.to(torch.int32), gt_labels.to(torch.int32), crowd, area,
                          image_seq=int(image_id))
        return tables

    # ---- reading: one device -> host copy
    def _host(self):
        if self._state_t is None:
            return dict(status=0, count=0, rec=np.zeros((0, _REC), np.int32), npig=np.zeros((self.num_classes, len(self.area_ranges)), np.int64))
        _, off = self._layout
        raw = self._state_t[:off[2]].cpu().numpy()                         # the header and npig; then the used part of the log
        status, count = (int(v) for v in raw[0:8].view(np.uint32))
        A = len(self.area_ranges)
        npig = raw[off[1]:off[1] + self.num_classes * A * 8].view(np.int64).reshape(self.num_classes, A).copy()
        n = min(count, self.capacity)
        rec = self._state_t[off[2]:off[2] + n * _REC * 4].cpu().numpy().view(np.int32).reshape(n, _REC).copy()
        return dict(status=status, count=count, rec=rec, npig=npig)

    def state_bytes(self):
        """the device state as bytes (uint8 NumPy array): two meters fed the same updates hold the same bytes"""
        return self._state_t.cpu().numpy().copy() if self._state_t is not None else np.zeros((0,), np.uint8)

    def records(self):
        """dict of the log's columns, one entry per detection in update order: image, label int32; score float32; rank int32 (-1 beyond
        the largest maxDet); matched, ignored uint32 [n, A]: bit t = IoU threshold t."""
        rec = self._host()['rec']
        words = rec[:, _C['VKN_MASKAP_REC_WORDS']:_C['VKN_MASKAP_REC_WORDS'] + 2 * len(self.area_ranges)].view(np.uint32)
        return dict(image=rec[:, _C['VKN_MASKAP_REC_IMAGE']].copy(), label=rec[:, _C['VKN_MASKAP_REC_LABEL']].copy(),
                    score=rec[:, _C['VKN_MASKAP_REC_SCORE']].copy().view(np.float32), rank=rec[:, _C['VKN_MASKAP_REC_RANK']].copy(),
                    matched=words[:, 0::2].copy(), ignored=words[:, 1::2].copy())

    def counts(self):
        """dict(npig int64 [C, A]: ground truths that are not ignored; records: detections logged so far; status)"""
        h = self._host()
        return dict(npig=h['npig'], records=h['count'], status=h['status'])

    def check_status(self):
        """Raises VknError when a status bit is set (reads the header: a synchronisation)."""
        if self._state_t is not None:
            self._raise_on(int(self._state_t[0:4].cpu().numpy().view(np.uint32)[0]))

    @staticmethod
    def _raise_on(status):
        if status:
            text = '; '.join(t for name, t in _BITS if status & _C[name])
            raise _lib.VknError(_lib.CONSTS['VKN_E_RANGE'], f'MaskAPMeter: status {status:#x}: {text}')

    def result(self):
        """`COCOeval.accumulate` and `summarize` in float64 -> dict(precision [T,101,C,A,M], recall [T,C,A,M], stats {mmdet's name: value}
        (the twelve of COCOeval when there are four area ranges and three maxDets), classwise [C]: per-class AP as the reference's
        `classwise` branch computes it (nan for a class without ground truth)).  Raises VknError when a status bit is set."""
        h = self._host()
        self._raise_on(h['status'])
        T, C, A, M = len(self.iou_thrs), self.num_classes, len(self.area_ranges), len(self.max_dets)
        rec_thrs = np.linspace(0.0, 1.0, 101)
        precision, recall = -np.ones((T, 101, C, A, M)), -np.ones((T, C, A, M))
        rec = h['rec']
        image, label, rank = (rec[:, _C[k]] for k in ('VKN_MASKAP_REC_IMAGE', 'VKN_MASKAP_REC_LABEL', 'VKN_MASKAP_REC_RANK'))
        score = rec[:, _C['VKN_MASKAP_REC_SCORE']].copy().view(np.float32)
        order = np.lexsort((rank, image))                                  # image id, then rank: COCOeval's concatenation over imgIds
        bits = np.arange(T, dtype=np.uint32)
        for c in range(C):
            of_c = order[(label[order] == c) & (rank[order] >= 0)]
            for a in range(A):
                npig = int(h['npig'][c, a])
                if npig == 0:
                    continue
                w = _C['VKN_MASKAP_REC_WORDS'] + 2 * a
                for m, max_det in enumerate(self.max_dets):
                    sel = of_c[rank[of_c] < max_det]
                    sel = sel[np.argsort(-score[sel], kind='mergesort')]
                    matched = (rec[sel, w].view(np.uint32)[None, :] >> bits[:, None] & 1).astype(bool)          # [T, nd]
                    ignored = (rec[sel, w + 1].view(np.uint32)[None, :] >> bits[:, None] & 1).astype(bool)
                    tp_sum = np.cumsum(matched & ~ignored, axis=1).astype(np.float64)
                    fp_sum = np.cumsum(~matched & ~ignored, axis=1).astype(np.float64)
                    nd = len(sel)
                    for t in range(T):
                        tp, fp = tp_sum[t], fp_sum[t]
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[t, c, a, m] = rc[-1] if nd else 0
                        pr = np.maximum.accumulate(pr[::-1])[::-1]         # the backward running maximum
                        inds = np.searchsorted(rc, rec_thrs, side='left')
                        q = np.zeros((101,))
                        ok = inds < nd
                        q[ok] = pr[inds[ok]]
                        precision[t, :, c, a, m] = q
        out = dict(precision=precision, recall=recall, stats={}, classwise=np.full((C,), np.nan))
        for c in range(C):
            p = precision[:, :, c, 0, -1]
            p = p[p > -1]
            if p.size:
                out['classwise'][c] = np.mean(p)
        if A == 4 and M == 3:
            def summary(ap, iou=None, a=0, m=M - 1):
                s = precision[:, :, :, a, m] if ap else recall[:, :, a, m]
                if iou is not None:
                    s = s[np.where(iou == self.iou_thrs)[0]]
                s = s[s > -1]
                return float(np.mean(s)) if s.size else -1.0
            values = [summary(True), summary(True, iou=0.5), summary(True, iou=0.75), summary(True, a=1), summary(True, a=2), summary(True, a=3),
                      summary(False, m=0), summary(False, m=1), summary(False, m=2), summary(False, a=1), summary(False, a=2), summary(False, a=3)]
            out['stats'] = dict(zip(stats_names(self.max_dets), values))
        return out
