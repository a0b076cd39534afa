#!/usr/bin/env python
"""Generate tests/golden/stq_*.npz from the REFERENCE ITSELF (needs the reference checkout; CPU only; never imported by a test).

    VKN_REFERENCE=<reference checkout> python tools/gen_golden_stq.py

The reference's tools/utils/STQ.py is loaded UNMODIFIED (`np.bool`, which newer NumPy dropped, is given back to it as an alias) and
fed exactly as tools/eval_dstq_step.py:47-60 feeds it: `valid = gt_cls != ignore`, `pred_cls[valid] * 2**16 + pred_ins[valid]`,
`gt_cls[valid] * 2**16 + gt_ins[valid]`, `update_state(gt, pred, seq_id)` (mode 1), and on the unmasked maps (mode 0).  A fixture holds
data only:

  stq_<case>.npz   num_classes, things, ignore_label, label_bit_shift, offset, seq_ids;
                   gt_sem, gt_ins, pred_sem, pred_ins int32 [S, F, H, W]: S sequences of F frames;
                   per mode m in (0, 1) and sequence s:  m<m>_s<s>_confusion int64 [n, n] AS ACCUMULATED (before result() zeroes rows),
                   m<m>_s<s>_{gt,pred,pair}_{keys,counts}: the three dicts sorted by key;
                   per mode: m<m>_STQ, _AQ, _IoU, _STQ_per_seq, _AQ_per_seq, _IoU_per_seq, _ID_per_seq, _Length_per_seq: `result()`.
The same seeds give the same bytes.
"""
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if not os.environ.get('VKN_REFERENCE'):
    raise SystemExit('set VKN_REFERENCE to the reference checkout')

import numpy as np  # noqa: E402

if not hasattr(np, 'bool'):
    np.bool = bool                                                        # STQ.py:159 spells the dtype the old way
_spec = importlib.util.spec_from_file_location('ref_stq', os.path.join(os.environ['VKN_REFERENCE'], 'tools', 'utils', 'STQ.py'))
ref_stq = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_stq)

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SHIFT, OFFSET = 16, 2 ** 16 * 256
CASES = {
    'kitti': dict(num_classes=19, things=list(range(11, 19)), ignore=255, S=2, F=3, H=24, W=39, seed=11, seq_ids=(2, 6), nt=2, ids=3),     # at most 2 x 2 gt tubes x 2 x 2 pred tubes = 16 intersections per sequence
    'city': dict(num_classes=19, things=list(range(0, 8)), ignore=255, S=1, F=2, H=16, W=32, seed=12, seq_ids=(0,)),
    'vipseg': dict(num_classes=124, things=list(range(66, 124)), ignore=200, S=1, F=2, H=12, W=20, seed=13, seq_ids=(0,)),
    'ign_in': dict(num_classes=5, things=[1, 2, 3], ignore=2, S=1, F=2, H=9, W=7, seed=14, seq_ids=(0,)),
    'ign_eq': dict(num_classes=6, things=[4, 5], ignore=6, S=1, F=2, H=9, W=7, seed=15, seq_ids=(0,)),
}


def frame(rng, p, drift):
    """One frame (gt_sem, gt_ins, pred_sem, pred_ins): segments of 3 x 4 pixels; `nt` thing classes carry ids 0 .. `ids` - 1 (0 = crowd in the ground truth);
    the prediction is the ground truth with a share of its segments redrawn (so tubes intersect, and predicted things lie over stuff);
    an ignore stripe down a gt column band and along a pred row band."""
    H, W, nc = p['H'], p['W'], p['num_classes']
    hb, wb = -(-H // 3), -(-W // 4)
    up = lambda a: np.kron(a, np.ones((3, 4), np.int64))[:H, :W]            # noqa: E731
    # few classes per case, so that tubes recur over frames: half things, half stuff
    stuff = [c for c in range(nc) if c not in p['things']]
    nt, ids = p.get('nt', 3), p.get('ids', 4)
    palette = np.array(p['things'][:nt] + stuff[:3])
    gsem = palette[rng.integers(0, len(palette), (hb, wb))]
    gins = rng.integers(0, ids, (hb, wb))
    redraw = rng.random((hb, wb)) < drift
    psem = np.where(redraw, palette[rng.integers(0, len(palette), (hb, wb))], gsem)
    pins = np.where(redraw, rng.integers(1, ids, (hb, wb)), np.maximum(gins, 1))
    gsem, gins, psem, pins = up(gsem), up(gins), up(psem), up(pins)
    gsem[:, W // 3:W // 3 + 2] = p['ignore']
    psem[H // 2:H // 2 + 1, :] = p['ignore']
    gins = np.where(np.isin(gsem, p['things']), gins, 0)
    pins = np.where(np.isin(psem, p['things']), pins, 0)
    return [a.astype(np.int32) for a in (gsem, gins, psem, pins)]


def run_case(name, p):
    rng = np.random.default_rng(p['seed'])
    maps = np.stack([np.stack([np.stack(frame(rng, p, 0.3)) for _ in range(p['F'])]) for _ in range(p['S'])])      # [S, F, 4, H, W]
    out = dict(num_classes=np.int64(p['num_classes']), things=np.array(p['things'], np.int64), ignore_label=np.int64(p['ignore']),
               label_bit_shift=np.int64(SHIFT), offset=np.int64(OFFSET), seq_ids=np.array(p['seq_ids'], np.int64),
               gt_sem=maps[:, :, 0], gt_ins=maps[:, :, 1], pred_sem=maps[:, :, 2], pred_ins=maps[:, :, 3])
    for mode in (0, 1):
        obj = ref_stq.STQuality(p['num_classes'], p['things'], p['ignore'], SHIFT, OFFSET)
        for s, sid in enumerate(p['seq_ids']):
            for f in range(p['F']):
                gt_cls, gt_ins, pred_cls, pred_ins = maps[s, f]
                valid = gt_cls != p['ignore'] if mode else np.ones_like(gt_cls, dtype=bool)
                pred_ps = pred_cls[valid] * (2 ** 16) + pred_ins[valid]
                gt_ps = gt_cls[valid] * (2 ** 16) + gt_ins[valid]
                obj.update_state(gt_ps, pred_ps, sid)
        for s, sid in enumerate(p['seq_ids']):
            out[f'm{mode}_s{s}_confusion'] = obj._iou_confusion_matrix_per_sequence[sid].astype(np.int64).copy()     # result() zeroes rows in place
            for t, d in (('gt', obj._ground_truth), ('pred', obj._predictions), ('pair', obj._intersections)):
                keys = sorted(int(k) for k in d[sid])
                out[f'm{mode}_s{s}_{t}_keys'] = np.array(keys, np.int64)
                out[f'm{mode}_s{s}_{t}_counts'] = np.array([int(d[sid][k]) for k in keys], np.int64)
        with np.errstate(all='ignore'):
            res = obj.result()
        for k, v in res.items():
            out[f'm{mode}_{k}'] = np.asarray(v, dtype=np.int64 if k in ('ID_per_seq', 'Length_per_seq') else np.float64)
        print(f'{name} mode {mode}: STQ={float(res["STQ"]):.6f} AQ={float(res["AQ"]):.6f} IoU={float(res["IoU"]):.6f}  '
              f'tubes gt/pred/pair={[len(d[sid]) for sid in p["seq_ids"] for d in (obj._ground_truth, obj._predictions, obj._intersections)]}')
    path = os.path.join(GOLDEN, f'stq_{name}.npz')
    np.savez_compressed(path, **out)
    print(f'  {path}: {os.path.getsize(path)} bytes')


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    for name, p in CASES.items():
        run_case(name, p)


if __name__ == '__main__':
    sys.exit(main())
