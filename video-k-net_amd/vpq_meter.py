"""`VPQMeter`: video panoptic quality from device maps (include/vkn_vpq.h, csrc/vkn_vpq.hip).

`vpq_eval` of the reference's evaluation scripts (tools/eval_dvpq_step.py:21-97, the same text in tools/eval_dvpq_vipseg.py:310-386), fed
as `eval()` / `read_to_eval()` feed it, runs on the device for every window of every window length at once: each frame is counted once,
the windows follow from per-frame tables, and nothing is read back.  tp, fn and fp are integer tables; the float64 sum of IoUs is rebuilt
on the host from the log of true positives in the scripts' order, so `counts()` equals the scripts' arrays bit for bit.  `result()`
restates their last lines (eval_dvpq_step.py:207-222, eval_dvpq_vipseg.py:469-485).

Two deliberate departures: ids are 64-bit throughout (eval_dvpq_step.py:56 wraps in int32), and a sequence shorter than k contributes no
window of that k (eval_dvpq_vipseg.py:441 shortens k instead, for that sequence and every later one).
"""
import warnings

import numpy as np

from . import _lib, ops
from ._map_meter import MapMeter

_BITS = (('VKN_VPQ_STATUS_ID_RANGE', 'ID_RANGE: an instance id outside [0, 2^label_bit_shift)'),
         ('VKN_VPQ_STATUS_CLASS_RANGE', 'CLASS_RANGE: a class outside the bins'),
         ('VKN_VPQ_STATUS_FULL_GT', 'FULL: a gt table (capacity["gt"]) overflowed'),
         ('VKN_VPQ_STATUS_FULL_PRED', 'FULL: a pred table (capacity["pred"]) overflowed'),
         ('VKN_VPQ_STATUS_FULL_PAIR', 'FULL: a pair table (capacity["pair"]) overflowed'),
         ('VKN_VPQ_STATUS_FULL_LOG', 'FULL: the log of true positives (capacity["log"]) overflowed'))
_EPSILON = 1e-10


class VPQMeter(MapMeter):
    """num_classes: the bins are num_classes + 1 (`num_cat`: 20 for STEP, 125 for VIP-Seg); things_list: the thing classes of
    PQ_thing / PQ_stuff; ks: window lengths, ascending (`--eval_frames`; (1, 2, 4, 6) in the VIP-Seg script); ign_id, label_bit_shift,
    offset: the scripts' constants.  capacity: slots (powers of two, 16 .. 2^20) of the gt / pred / pair tables of ONE frame and of ONE
    window, and records of the TP log of one sequence; what overflows is reported by `result()` / `check_status()`, never silently."""
    _BITS, _CONSTS, _new_state = _BITS, _lib.VPQ, staticmethod(ops.vpq_state)

    def __init__(self, num_classes, things_list, ks=(1,), ign_id=255, label_bit_shift=16, offset=2 ** 30, capacity=None, device=None):
        things = sorted({int(c) for c in things_list})
        if things and (things[0] < 0 or things[-1] >= num_classes):
            raise ValueError(f'things_list must name classes in [0, {num_classes}), got {things}')
        cap = dict(gt=512, pred=512, pair=2048, log=131072)
        cap.update(capacity or {})
        if set(cap) != {'gt', 'pred', 'pair', 'log'}:
            raise ValueError(f'capacity takes the keys gt, pred, pair, log, got {sorted(cap)}')
        self.num_classes, self.num_cat, self.ks = int(num_classes), int(num_classes) + 1, tuple(int(k) for k in ks)
        self.ign_id, self.label_bit_shift, self.offset = int(ign_id), int(label_bit_shift), int(offset)
        self.things_list, self.capacity = things, cap
        super().__init__(device)
        self._cfg = ops.vpq_cfg(self.num_cat, self.ks, ign_id, label_bit_shift, offset, cap['gt'], cap['pred'], cap['pair'], cap['log'])
        self._bytes, self._off = ops.vpq_layout(self._cfg)

    # ---- counting: device only
    def update_state(self, gt_sem, gt_ins, pred_sem, pred_ins, sequence_id=0):
        """int32 CUDA maps [H,W] or [B,H,W]: CONSECUTIVE frames of ONE sequence, behind the frames of earlier calls.  pred_sem / pred_ins:
        `TrackTail`'s semantic_map / track_map as they come.  Enqueues on the current stream; nothing is read back."""
        ops.vpq_update(self._cfg, self._state(sequence_id), gt_sem, gt_ins, pred_sem, pred_ins)

    # ---- reading: the public parts of a state, one device -> host copy
    def _host(self, sequence_id):
        o, nk, nc = self._off, len(self.ks), self.num_cat
        raw = self._states[sequence_id][:o[3]].cpu().numpy()
        status, frames, used = (int(v) for v in raw[0:12].view(np.uint32))
        acc = raw[o[1]:o[1] + nk * 3 * nc * 8].view(np.int64).reshape(nk, 3, nc).copy()
        log = raw[o[2]:o[2] + 32 * min(used, self.capacity['log'])].view(np.int64).reshape(-1, 4)
        log = log[np.lexsort((log[:, 1], log[:, 0]))].copy()
        return dict(status=status, frames=frames, acc=acc, log=log)

    def tables(self, sequence_id=0):
        """dict(acc int64 [nk, 3, num_cat]: tp, fn, fp per window length; log int64 [n, 4] sorted by its first two fields:
        (k_index << 48) | window_ordinal, pair key, int_area, union; frames; status) of one sequence."""
        return self._host(sequence_id)

    def _counts(self, hosts):
        nk, nc, shift = len(self.ks), self.num_cat, self.label_bit_shift
        iou, acc = np.zeros((nk, nc), np.float64), np.zeros((nk, 3, nc), np.int64)
        for h in hosts:
            acc += h['acc']
            log = h['log']
            # a window's row is summed in ascending pair key (np.unique's order, eval_dvpq_step.py:63), the rows are added window after
            # window (`np.stack(...).sum(axis=0)`, :198-208), sequence after sequence (:225)
            bounds = np.flatnonzero(np.r_[True, log[1:, 0] != log[:-1, 0], True]) if len(log) else np.zeros((1,), np.int64)
            for a, b in zip(bounds[:-1], bounds[1:]):
                row = np.zeros((nc,), np.float64)
                for _, key, ia, union in log[a:b]:
                    row[int(key) // self.offset >> shift] += ia / union
                iou[int(log[a, 0]) >> 48] += row
        return [dict(iou=iou[i].copy(), tp=acc[i, 0].astype(np.float64), fn=acc[i, 1].astype(np.float64), fp=acc[i, 2].astype(np.float64))
                for i in range(nk)]

    def counts(self):
        """Per window length, in the order of `ks`: dict(iou, tp, fn, fp) float64 [num_cat], the scripts' four arrays summed over every
        window of every sequence (sequences in order of first appearance)."""
        return self._counts([self._host(sid) for sid in self._states])

    def result(self):
        """The scripts' last lines (eval_dvpq_step.py:207-222) per window length: {k: dict(PQ, PQ_thing, PQ_stuff, sq, rq, pq)} over the
        first num_classes bins, and 'VPQ': the mean of PQ over `ks`.  Raises VknError when any status bit is set."""
        hosts = {sid: self._host(sid) for sid in self._states}
        for sid, h in hosts.items():
            self._raise_on(sid, h['status'])
        things = np.zeros((self.num_classes,), bool)
        things[self.things_list] = True
        out = {}
        with np.errstate(invalid='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)               # the mean of no class (no things, or no stuff) is nan
            for k, c in zip(self.ks, self._counts(list(hosts.values()))):
                iou, tp, fn, fp = (c[n][:self.num_classes] for n in ('iou', 'tp', 'fn', 'fp'))
                sq = iou / (tp + _EPSILON)
                rq = tp / (tp + 0.5 * fn + 0.5 * fp + _EPSILON)
                pq = sq * rq
                out[k] = dict(PQ=pq.mean(), PQ_thing=pq[things].mean(), PQ_stuff=pq[np.logical_not(things)].mean(), sq=sq, rq=rq, pq=pq)
        out['VPQ'] = np.mean([out[k]['PQ'] for k in self.ks])
        return out
