#!/usr/bin/env python
"""Generate tests/golden/vpq_*.npz from the REFERENCE ITSELF (needs the reference checkout; CPU only; never imported by a test).

    VKN_REFERENCE=<reference checkout> python tools/gen_golden_vpq.py

Both evaluation scripts are loaded UNMODIFIED: tools/eval_dvpq_step.py parses `sys.argv` at import, so it is given a dummy
`result_path`; tools/eval_dvpq_vipseg.py imports `mmcv`, which oracle/standins provides.  Their `vpq_eval` is fed window by window as
`eval()` (eval_dvpq_step.py:100-141) / `read_to_eval()` (eval_dvpq_vipseg.py:389-409) feed it — the k frames of a window side by side,
`pred = cat * 2**16 + ins` in int32 — except that the ground-truth ids are int64 (as in the VIP-Seg script), so that
eval_dvpq_step.py:56 does not wrap.  A sequence shorter than k gets no window of that k.  A fixture holds data only:

  vpq_<case>.npz   num_classes, things, ks, ign_id, label_bit_shift, offset, seq_ids;
                   gt_sem, gt_ins, pred_sem, pred_ins int32 [S, F, H, W]: S sequences of F frames (vipseg: raw_pan, the raw panoptic
                   map that the reference's own `vip2hb` turned into gt_sem / gt_ins);
                   per window length index i and sequence s:  k<i>_s<s>_{iou,tp,fn,fp} float64 [windows, num_cat]: the rows as `vpq_eval`
                   returned them;  per i: k<i>_{iou,tp,fn,fp} [num_cat]: the rows of all sequences concatenated and summed as
                   eval_dvpq_step.py:225-228 sums them, and k<i>_{PQ,PQ_thing,PQ_stuff}: eval_dvpq_step.py:230-235.
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


def _load(name, argv, extra_path=()):
    saved, path = sys.argv, list(sys.path)
    sys.argv, sys.path = argv, list(extra_path) + sys.path
    try:
        spec = importlib.util.spec_from_file_location('ref_' + name, os.path.join(os.environ['VKN_REFERENCE'], 'tools', name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.argv, sys.path = saved, path
    return mod


ref_step = _load('eval_dvpq_step', ['eval_dvpq_step.py', 'no_such_result_path'])
ref_vip = _load('eval_dvpq_vipseg', ['eval_dvpq_vipseg.py'], [os.path.join(ROOT, 'oracle', 'standins')])

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SHIFT, OFFSET, IGN = 16, 2 ** 30, 255


def video(rng, F, H, W, things, stuff, void_class, ids=3, keep=0.85, hit=0.7):
    """F frames of 3 x 4-pixel segments: the ground truth of a frame is the frame before with a share of its segments redrawn, the
    prediction is the ground truth with a share redrawn (so most segments match and some do not); an ignored column band in the
    ground truth, and a row band of class `void_class` in the prediction."""
    hb, wb = -(-H // 3), -(-W // 4)
    up = lambda a: np.kron(a, np.ones((3, 4), np.int64))[:H, :W]            # noqa: E731
    palette = np.array(list(things) + list(stuff))

    def draw():
        return palette[rng.integers(0, len(palette), (hb, wb))], rng.integers(1, ids + 1, (hb, wb))
    gsem, gins = draw()
    out = []
    for _ in range(F):
        nsem, nins = draw()
        stay = rng.random((hb, wb)) < keep
        gsem, gins = np.where(stay, gsem, nsem), np.where(stay, gins, nins)
        nsem, nins = draw()
        same = rng.random((hb, wb)) < hit
        psem, pins = np.where(same, gsem, nsem), np.where(same, gins, nins)
        gs, gi, ps, pi = up(gsem), up(gins), up(psem), up(pins)
        gs[:, W // 3:W // 3 + 2] = IGN
        ps[H // 2:H // 2 + 1, :] = void_class
        gi = np.where(np.isin(gs, things), gi, 0)
        pi = np.where(np.isin(ps, things), pi, 0)
        out.append(np.stack([gs, gi, ps, pi]))
    return np.stack(out).astype(np.int32)                                      # [F, 4, H, W]


def kitti():
    rng = np.random.default_rng(31)
    maps = np.stack([video(rng, 5, 24, 39, (11, 13), (0, 1, 7), 19) for _ in range(2)])
    return dict(num_classes=19, things=[11, 13], ks=(1, 2, 4), seq_ids=(2, 6), maps=maps, vpq_eval=ref_step.vpq_eval)


def vipseg():
    """the ground truth comes from a raw panoptic map (class id + 1 for stuff, (class id + 1) * 100 + instance for things, 0 and 200
    void) through the reference's own vip2hb (eval_dvpq_vipseg.py:275-293), as read_to_eval has it (:399-406)"""
    rng = np.random.default_rng(32)
    F, H, W = 7, 12, 20
    hb, wb = -(-H // 3), -(-W // 4)
    up = lambda a: np.kron(a, np.ones((3, 4), np.int64))[:H, :W]            # noqa: E731
    raw_palette = np.array([1, 2, 14, 300, 301, 6100, 6102, 0, 200])          # wall, ceiling, floor, two doors, two persons, void twice
    cells = raw_palette[rng.integers(0, len(raw_palette), (hb, wb))]
    raws, frames = [], []
    for _ in range(F):
        stay = rng.random((hb, wb)) < 0.85
        cells = np.where(stay, cells, raw_palette[rng.integers(0, len(raw_palette), (hb, wb))])
        raw = up(cells).astype(np.int64)
        pan = ref_vip.vip2hb(raw)
        gs, gi = pan // ref_vip.DIVISOR_NEW, pan % ref_vip.DIVISOR_NEW
        same = up(rng.random((hb, wb)) < 0.7).astype(bool)
        ps = np.where(same & (gs != IGN), gs, up(np.array([0, 12, 66, 118])[rng.integers(0, 4, (hb, wb))]))
        pi = np.where(same & (gs != IGN), gi, up(rng.integers(1, 3, (hb, wb))))
        pi = np.where(ps >= ref_vip.NUM_STUFF, pi, 0)
        raws.append(raw)
        frames.append(np.stack([gs, gi, ps, pi]))
    maps = np.stack(frames).astype(np.int32)[None]
    return dict(num_classes=124, things=list(range(ref_vip.NUM_STUFF, 124)), ks=(1, 2, 4, 6), seq_ids=(0,), maps=maps,
                vpq_eval=ref_vip.vpq_eval, raw_pan=np.stack(raws).astype(np.int32)[None])


# vpq_edges: two hand-made frames of 9 x 7, as runs (pixels, gt class, gt id, pred class, pred id) in raster order
EDGE_FRAMES = (
    ((1, 0, 0, 19, 0), (2, 0, 0, 0, 0), (1, 5, 0, 0, 0),                      # class 0: gt 3, pred 3, both 2: IoU exactly 1/2, no TP; a pixel in bin 19
     (1, 11, 1, 6, 0), (3, 11, 1, 11, 1), (1, 5, 0, 11, 1),                   # class 11: gt 4, pred 4, both 3: 2 * 3 = 5 + 1, a TP by one pixel
     (2, 13, 2, 13, 7), (1, IGN, 0, 13, 7), (1, 5, 0, 13, 7),                 # class 13: gt 2, pred 4, both 2: 1/2 without the void pixel, 2/3 with it
     (1, IGN, 0, 2, 0), (1, IGN, 5, 2, 0), (2, 5, 0, 2, 0),                   # pred class 2: 2 of 4 pixels ignored (one under an ignored id with instance 5): fp
     (1, IGN, 0, 3, 0), (2, IGN, 5, 3, 0), (1, 5, 0, 3, 0),                   # pred class 3: 3 of 4 pixels ignored: skipped
     (20, 1, 0, 1, 0), (22, 5, 0, 6, 0)),
    ((4, 0, 0, 0, 0), (2, 11, 1, 11, 1), (2, 11, 1, 11, 2), (2, 11, 3, 11, 2), (3, 13, 2, 13, 7), (2, IGN, 5, 3, 0), (2, IGN, 0, 2, 0),
     (2, 5, 0, 2, 0), (20, 1, 0, 1, 0), (24, 5, 0, 6, 0)),
)


def edges():
    frames = []
    for runs in EDGE_FRAMES:
        flat = np.concatenate([np.tile(np.array(r[1:], np.int32)[:, None], (1, r[0])) for r in runs], axis=1)
        assert flat.shape == (4, 63)
        frames.append(flat.reshape(4, 9, 7))
    return dict(num_classes=19, things=[11, 13], ks=(1, 2, 4), seq_ids=(0,), maps=np.stack(frames)[None], vpq_eval=ref_step.vpq_eval)


def run_case(name, p):
    maps, ks, num_cat = p['maps'], p['ks'], p['num_classes'] + 1               # maps [S, F, 4, H, W]
    S, F = maps.shape[:2]
    out = dict(num_classes=np.int64(p['num_classes']), things=np.array(p['things'], np.int64), ks=np.array(ks, np.int64), ign_id=np.int64(IGN),
               label_bit_shift=np.int64(SHIFT), offset=np.int64(OFFSET), seq_ids=np.array(p['seq_ids'], np.int64),
               gt_sem=maps[:, :, 0], gt_ins=maps[:, :, 1], pred_sem=maps[:, :, 2], pred_ins=maps[:, :, 3])
    if 'raw_pan' in p:
        out['raw_pan'] = p['raw_pan']
    things_index = np.zeros((p['num_classes'],), bool)
    things_index[p['things']] = True
    for i, k in enumerate(ks):
        every = [[], [], [], []]
        for s in range(S):
            rows = [[], [], [], []]
            for w in range(F - k + 1):                                          # eval_dvpq_step.py:187
                gs, gi, ps, pi = (np.concatenate(list(maps[s, w:w + k, m]), axis=1) for m in range(4))     # :106-107, :138
                pred = ps.astype(np.int32) * (2 ** SHIFT) + pi.astype(np.int32)                            # :108
                gt = gs.astype(np.int64) * (2 ** SHIFT) + gi.astype(np.int64)
                res = p['vpq_eval']([pred, gt])
                for r, v in zip(rows, res):
                    assert v.shape == (num_cat,) and v.dtype == np.float64
                    r.append(v)
            for n, r, e in zip(('iou', 'tp', 'fn', 'fp'), rows, every):
                out[f'k{i}_s{s}_{n}'] = np.stack(r) if r else np.zeros((0, num_cat), np.float64)
                e.append(out[f'k{i}_s{s}_{n}'])
        iou, tp, fn, fp = (np.concatenate(e, axis=0).sum(axis=0) for e in every)                           # :225-228
        out[f'k{i}_iou'], out[f'k{i}_tp'], out[f'k{i}_fn'], out[f'k{i}_fp'] = iou, tp, fn, fp
        epsilon, n = 1e-10, p['num_classes']
        sq = iou[:n] / (tp[:n] + epsilon)
        rq = tp[:n] / (tp[:n] + 0.5 * fn[:n] + 0.5 * fp[:n] + epsilon)
        pq = sq * rq
        out[f'k{i}_PQ'], out[f'k{i}_PQ_thing'], out[f'k{i}_PQ_stuff'] = pq.mean(), pq[things_index].mean(), pq[np.logical_not(things_index)].mean()
        print(f'{name} k={k}: windows={[len(out[f"k{i}_s{s}_tp"]) for s in range(S)]} tp={tp.sum():.0f} fn={fn.sum():.0f} fp={fp.sum():.0f} '
              f'PQ={pq.mean():.6f}')
    path = os.path.join(GOLDEN, f'vpq_{name}.npz')
    np.savez_compressed(path, **out)
    print(f'  {path}: {os.path.getsize(path)} bytes')


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    for name, make in (('kitti', kitti), ('vipseg', vipseg), ('edges', edges)):
        run_case(name, make())


if __name__ == '__main__':
    sys.exit(main())
