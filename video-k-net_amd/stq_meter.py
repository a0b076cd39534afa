"""`STQMeter`: Segmentation and Tracking Quality from device maps (include/vkn_stq.h, csrc/vkn_stq.hip).

The counting half of the reference's `STQuality` (tools/utils/STQ.py:106-188, fed as tools/eval_dstq_step.py:36-60 feeds it) runs on
the device, one launch per `update_state`, without a synchronisation: the four integer tables of every sequence live in one device
state and equal the reference's bit for bit.  `result()` copies each state to the host once and restates `STQuality.result()`
(STQ.py:190-283) in float64 from those tables.
"""
import numpy as np
import torch

from . import _lib, ops
from ._map_meter import MapMeter

_BITS = (('VKN_STQ_STATUS_ID_RANGE', 'ID_RANGE: an instance id outside [0, 2^label_bit_shift)'),
         ('VKN_STQ_STATUS_CLASS_RANGE', 'CLASS_RANGE: a class outside the confusion matrix'),
         ('VKN_STQ_STATUS_FULL_GT', 'FULL: the gt table (capacity["gt"]) overflowed'),
         ('VKN_STQ_STATUS_FULL_PRED', 'FULL: the pred table (capacity["pred"]) overflowed'),
         ('VKN_STQ_STATUS_FULL_PAIR', 'FULL: the pair table (capacity["pair"]) overflowed'))
_EPSILON = 1e-15


class STQMeter(MapMeter):
    """num_classes, things_list, ignore_label, label_bit_shift, offset: `STQuality`'s arguments, and its ValueError for a small offset.
    drop_ignored_gt=True: pixels whose gt class is `ignore_label` do not exist, as the evaluation scripts mask them; False: `STQuality`
    on unmasked maps.  capacity: slots (powers of two, 16 .. 2^20) of the tube and intersection tables of ONE sequence; a table that
    overflows is reported by `result()` / `check_status()`, never silently."""
    _BITS, _CONSTS, _new_state = _BITS, _lib.STQ, staticmethod(ops.stq_state)

    def __init__(self, num_classes, things_list, ignore_label, label_bit_shift, offset, drop_ignored_gt=True, capacity=None, device=None):
        lower_bound = num_classes << label_bit_shift
        if offset < lower_bound:
            raise ValueError('The provided offset %d is too small. No guarantess about the correctness of the results can be made. Please choose '
                             'an offset that is higher than num_classes * max_instances_per_category = %d' % (offset, lower_bound))
        things = sorted({int(c) for c in things_list})
        if things and (things[0] < 0 or things[-1] >= num_classes):
            raise ValueError(f'things_list must name classes in [0, {num_classes}), got {things}')
        cap = dict(gt=2048, pred=8192, pair=32768)
        cap.update(capacity or {})
        if set(cap) != {'gt', 'pred', 'pair'}:
            raise ValueError(f'capacity takes the keys gt, pred, pair, got {sorted(cap)}')
        self.num_classes, self.ignore_label, self.label_bit_shift, self.offset = int(num_classes), int(ignore_label), int(label_bit_shift), int(offset)
        self.things_list, self.drop_ignored_gt, self.capacity = things, bool(drop_ignored_gt), cap
        super().__init__(device)
        self._cfg = ops.stq_cfg(num_classes, ignore_label, label_bit_shift, offset, drop_ignored_gt, cap['gt'], cap['pred'], cap['pair'])
        self._bytes, self._off = ops.stq_layout(self._cfg)
        self.n = num_classes + 1 if ignore_label >= num_classes else num_classes
        if ignore_label >= num_classes:
            self._include = np.arange(num_classes)
        else:
            self._include = np.array([i for i in range(num_classes) if i != ignore_label], dtype=np.int64)
        thing = np.zeros((self.n,), dtype=np.uint8)
        thing[things] = 1
        self._is_thing = torch.from_numpy(thing).to(self.device)

    # ---- counting: device only
    def update_state(self, gt_sem, gt_ins, pred_sem, pred_ins, sequence_id=0):
        """int32 CUDA maps [H,W] or [B,H,W]: frames of ONE sequence.  pred_sem / pred_ins: `TrackTail`'s semantic_map / track_map as
        they come.  Enqueues one launch on the current stream; nothing is read back."""
        ops.stq_update(self._cfg, self._state(sequence_id), self._is_thing, gt_sem, gt_ins, pred_sem, pred_ins)

    # ---- reading: one device -> host copy per state
    def _host(self, sequence_id):
        raw = self._states[sequence_id].cpu().numpy()
        o, n, cap = self._off, self.n, self.capacity
        out = dict(status=int(raw[0:4].view(np.uint32)[0]), frames=int(raw[4:8].view(np.uint32)[0]),
                   confusion=raw[o[1]:o[1] + n * n * 8].view(np.int64).reshape(n, n).copy())
        for i, t in enumerate(('gt', 'pred', 'pair')):
            keys = raw[o[2 + 2 * i]:o[2 + 2 * i] + 8 * cap[t]].view(np.int64)
            counts = raw[o[3 + 2 * i]:o[3 + 2 * i] + 8 * cap[t]].view(np.int64)
            used = np.flatnonzero(keys >= 0)
            used = used[np.argsort(keys[used], kind='stable')]
            out[t + '_keys'], out[t + '_counts'] = keys[used].copy(), counts[used].copy()
        return out

    def tables(self, sequence_id=0):
        """dict(confusion int64 [n,n] as accumulated, gt_keys / gt_counts, pred_keys / pred_counts, pair_keys / pair_counts sorted by key,
        status, frames) of one sequence."""
        return self._host(sequence_id)

    def result(self):
        """`STQuality.result()` (STQ.py:190-283) in float64 from the device tables; the same eight entries.  AQ is summed over the
        intersection table in ascending key order."""
        hosts = {sid: self._host(sid) for sid in self._states}
        for sid, h in hosts.items():
            self._raise_on(sid, h['status'])
        num_tubes, aq_per_seq, iou_per_seq, ids, lengths = [], [], [], [], []
        total = np.zeros((self.n, self.n), dtype=np.int64)
        for sid, h in hosts.items():
            gk, gc, pk, pc, ik, ic = (h[k] for k in ('gt_keys', 'gt_counts', 'pred_keys', 'pred_counts', 'pair_keys', 'pair_counts'))
            outer = 0.0
            if ik.size:
                gi, pi = np.searchsorted(gk, ik // self.offset), np.searchsorted(pk, ik % self.offset)
                tpa, gsz, psz = ic, gc[gi], pc[pi]
                terms = tpa * (tpa / (psz + gsz - tpa))
                inner = np.bincount(gi, weights=terms, minlength=gk.size)          # adds in the order given: ascending key
                for g in range(gk.size):
                    outer += 1.0 / gc[g] * inner[g]
            num_tubes.append(int(gk.size))
            aq_per_seq.append(outer)
            ids.append(sid)
            lengths.append(h['frames'])
            conf = h['confusion'].copy()
            keep = np.zeros((self.n, 1), dtype=np.int64)
            keep[self._include] = 1
            conf *= keep
            total += conf
            iou_per_seq.append(self._miou(conf, 1e-15))
        aq_mean = np.sum(aq_per_seq) / np.maximum(np.sum(num_tubes), _EPSILON)
        aq_per_seq = aq_per_seq / np.maximum(num_tubes, _EPSILON)
        iou_mean = self._miou(total, _EPSILON)
        return {'STQ': np.sqrt(aq_mean * iou_mean), 'AQ': aq_mean, 'IoU': float(iou_mean), 'STQ_per_seq': np.sqrt(aq_per_seq * iou_per_seq),
                'AQ_per_seq': aq_per_seq, 'IoU_per_seq': iou_per_seq, 'ID_per_seq': ids, 'Length_per_seq': lengths}

    @staticmethod
    def _miou(conf, eps):
        inter = conf.diagonal()
        unions = inter + (conf.sum(axis=0) - inter) + (conf.sum(axis=1) - inter)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.sum(inter.astype(np.double) / np.maximum(unions, eps).astype(np.double)) / np.count_nonzero(unions)
