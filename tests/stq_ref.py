"""NumPy restatement of the STQ metric for the tests: the per-pixel rules of include/vkn_stq.h (`update_state`) and the float64 ratios
(`result`).  Plain module, no import of the package under test and none of the reference: tests/test_stq_refs.py pins it to the
fixtures tests/golden/stq_*.npz, which tools/gen_golden_stq.py wrote from the reference itself."""
import os

import numpy as np

ID_RANGE, CLASS_RANGE = 1, 2          # the status bits this restatement can raise (a dict is never full)


def confusion_size(num_classes, ignore_label):
    return num_classes + 1 if ignore_label >= num_classes else num_classes


class STQRef:
    def __init__(self, num_classes, things_list, ignore_label, label_bit_shift, offset, drop_ignored_gt=True):
        if offset < num_classes << label_bit_shift:
            raise ValueError('offset too small')
        self.nc, self.things, self.ignore, self.shift, self.offset, self.drop = num_classes, list(things_list), ignore_label, label_bit_shift, offset, drop_ignored_gt
        self.n = confusion_size(num_classes, ignore_label)
        self.include = np.array([i for i in range(num_classes) if ignore_label >= num_classes or i != ignore_label], dtype=np.int64)
        self.seqs = {}                # id -> dict(confusion, gt, pred, pair, frames, status), in order of first appearance

    def update_state(self, gt_sem, gt_ins, pred_sem, pred_ins, sequence_id=0):
        """int maps of one shape: [H,W], or [B,H,W] = B frames of the sequence"""
        gs, gi, ps, pi = (np.asarray(a).astype(np.int64) for a in (gt_sem, gt_ins, pred_sem, pred_ins))
        frames = gs.shape[0] if gs.ndim == 3 else 1
        gs, gi, ps, pi = gs.ravel(), gi.ravel(), ps.ravel(), pi.ravel()
        seq = self.seqs.setdefault(sequence_id, dict(confusion=np.zeros((self.n, self.n), np.int64), gt={}, pred={}, pair={}, frames=0, status=0))
        seq['frames'] += frames
        live = gs != self.ignore if self.drop else np.ones(gs.shape, bool)
        sl, sp = gs.copy(), ps.copy()
        if self.ignore > self.nc:
            sl[gs == self.ignore], sp[ps == self.ignore] = self.nc, self.nc
        bad_class = (sl < 0) | (sl >= self.n) | (sp < 0) | (sp >= self.n)
        bad_id = (gi < 0) | (gi >= 1 << self.shift) | (pi < 0) | (pi >= 1 << self.shift)
        seq['status'] |= (CLASS_RANGE if (live & bad_class).any() else 0) | (ID_RANGE if (live & bad_id).any() else 0)
        live &= ~bad_class & ~bad_id
        gs, gi, ps, pi, sl, sp = (a[live] for a in (gs, gi, ps, pi, sl, sp))
        np.add.at(seq['confusion'], (sl, sp), 1)
        lm, pm = np.isin(sl, self.things), np.isin(sp, self.things)
        crowd = lm & (gi == 0)
        lm, pm = lm & ~crowd, pm & ~crowd
        yt, yp = (gs << self.shift) + gi, (ps << self.shift) + pi
        for table, keys in ((seq['pred'], yp[pm]), (seq['gt'], yt[lm]), (seq['pair'], yt[lm & pm] * self.offset + yp[lm & pm])):
            for k, c in zip(*np.unique(keys, return_counts=True)):
                table[int(k)] = table.get(int(k), 0) + int(c)

    def tables(self, sequence_id=0):
        """confusion as accumulated, and the three dicts as sorted key / count arrays"""
        seq = self.seqs[sequence_id]
        out = dict(confusion=seq['confusion'].copy(), frames=seq['frames'], status=seq['status'])
        for t in ('gt', 'pred', 'pair'):
            keys = sorted(seq[t])
            out[t + '_keys'], out[t + '_counts'] = np.array(keys, dtype=np.int64), np.array([seq[t][k] for k in keys], dtype=np.int64)
        return out

    def pairs(self, sequence_id=0):
        """the number of summed terms of the sequence's AQ: the size of its intersection table"""
        return len(self.seqs[sequence_id]['pair'])

    def result(self):
        tubes, aq, iou, ids, lengths = [], [], [], [], []
        total = np.zeros((self.n, self.n), np.int64)
        for sid, seq in self.seqs.items():
            outer = 0.0
            for g in sorted(seq['gt']):
                inner = 0.0
                for p in sorted(seq['pred']):
                    tpa = seq['pair'].get(self.offset * g + p)
                    if tpa is not None:
                        inner += tpa * (tpa / (seq['pred'][p] + seq['gt'][g] - tpa))
                outer += 1.0 / seq['gt'][g] * inner
            tubes.append(len(seq['gt']))
            aq.append(outer)
            ids.append(sid)
            lengths.append(seq['frames'])
            conf = seq['confusion'].copy()
            keep = np.zeros((self.n, 1), np.int64)
            keep[self.include] = 1
            conf *= keep
            total += conf
            iou.append(_miou(conf))
        aq_mean = np.sum(aq) / np.maximum(np.sum(tubes), 1e-15)
        aq = aq / np.maximum(tubes, 1e-15)
        iou_mean = _miou(total)
        return {'STQ': np.sqrt(aq_mean * iou_mean), 'AQ': aq_mean, 'IoU': float(iou_mean), 'STQ_per_seq': np.sqrt(aq * iou), 'AQ_per_seq': aq,
                'IoU_per_seq': iou, 'ID_per_seq': ids, 'Length_per_seq': lengths}


def _miou(conf):
    inter = conf.diagonal()
    unions = inter + (conf.sum(axis=0) - inter) + (conf.sum(axis=1) - inter)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.sum(inter.astype(np.double) / np.maximum(unions, 1e-15).astype(np.double)) / np.count_nonzero(unions)


# ---- seeded inputs shared by tests/test_stq_refs.py (the premises) and tests/test_gpu_stq.py (the runs)
KITTI = dict(num_classes=19, things_list=list(range(11, 19)), ignore_label=255, label_bit_shift=16, offset=2 ** 16 * 256)


def blocky(rng, H, W, num_classes, things, ignore_label, n_ids=6, cell=8, ignore_share=0.05):
    """(sem, ins) int32 [H,W] of rectangular segments: classes and ids drawn per `cell` x `cell` block; id 0 (crowd) occurs; stuff has id 0"""
    hb, wb = -(-H // cell), -(-W // cell)
    sem_b = rng.integers(0, num_classes, (hb, wb))
    sem_b[rng.random((hb, wb)) < ignore_share] = ignore_label
    ins_b = rng.integers(0, n_ids, (hb, wb))
    sem = np.kron(sem_b, np.ones((cell, cell), np.int64))[:H, :W]
    ins = np.kron(ins_b, np.ones((cell, cell), np.int64))[:H, :W]
    ins = np.where(np.isin(sem, things), ins, 0)
    return sem.astype(np.int32), ins.astype(np.int32)


def seeded_maps(seed, H, W, cfg=KITTI, **kw):
    """gt_sem, gt_ins, pred_sem, pred_ins int32 [H,W]: two independent blocky maps, so that every kind of count occurs"""
    rng = np.random.default_rng(seed)
    g = blocky(rng, H, W, cfg['num_classes'], cfg['things_list'], cfg['ignore_label'], **kw)
    p = blocky(rng, H, W, cfg['num_classes'], cfg['things_list'], cfg['ignore_label'], **kw)
    return g[0], g[1], p[0], p[1]


def noisy_maps(seed, H, W, cfg=KITTI, n_ids=64):
    """per-pixel random things with `n_ids` ids each side: thousands of distinct pair keys in a few thousand pixels (LDS overflow, capacity)"""
    rng = np.random.default_rng(seed)
    things = np.array(cfg['things_list'])
    out = []
    for _ in range(2):
        out += [things[rng.integers(0, len(things), (H, W))].astype(np.int32), rng.integers(1, n_ids + 1, (H, W)).astype(np.int32)]
    return tuple(out)


def dominant_maps(seed, H, W, cfg=KITTI):
    """one gt tube matched by one pred tube over the upper two thirds of the frame, blocky maps below: one pair key in most workgroups"""
    gs, gi, ps, pi = seeded_maps(seed, H, W, cfg)
    cut = (2 * H) // 3
    t = cfg['things_list'][0]
    gs[:cut], gi[:cut], ps[:cut], pi[:cut] = t, 7, t, 9
    return gs, gi, ps, pi


# ---- the fixtures tests/golden/stq_<case>.npz (tools/gen_golden_stq.py)
CASES = ('kitti', 'city', 'vipseg', 'ign_in', 'ign_eq')
RESULT_KEYS = ('STQ', 'AQ', 'IoU', 'STQ_per_seq', 'AQ_per_seq', 'IoU_per_seq', 'ID_per_seq', 'Length_per_seq')
TABLE_KEYS = ('confusion', 'gt_keys', 'gt_counts', 'pred_keys', 'pred_counts', 'pair_keys', 'pair_counts')
LDS_OVERFLOW = dict(seed=21, H=96, W=96)            # noisy_maps: one full span and a short one
CAPACITY = dict(seed=22, H=16, W=24)                # noisy_maps, against cap_pair = 16
CONTENTION = dict(seed=23, H=375, W=1242)           # dominant_maps at KITTI-STEP's raw size


def load_case(name):
    """(constructor arguments, sequence ids, the four maps [S,F,H,W], the npz)"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', f'stq_{name}.npz'))
    args = dict(num_classes=int(z['num_classes']), things_list=[int(t) for t in z['things']], ignore_label=int(z['ignore_label']),
                label_bit_shift=int(z['label_bit_shift']), offset=int(z['offset']))
    return args, [int(s) for s in z['seq_ids']], tuple(z[k] for k in ('gt_sem', 'gt_ins', 'pred_sem', 'pred_ins')), z


def assert_tables(got, z, mode, s, what):
    """the four tables of sequence index `s` equal the fixture's, at zero tolerance"""
    for k in TABLE_KEYS:
        want = z[f'm{mode}_s{s}_{k}']
        assert got[k].dtype == np.int64 and got[k].shape == want.shape and np.array_equal(got[k], want), f'{what}: {k} of sequence {s} differs'


def assert_result(res, z, mode, terms, what):
    """every entry of result(): integers exact, floats within terms x 2^-52 relative — the re-ordering bound of a sum of `terms` non-negative
    doubles; terms = the summed pairs (per sequence, and all of them for the totals), at least 1"""
    assert tuple(res) == RESULT_KEYS
    assert [int(i) for i in res['ID_per_seq']] == z[f'm{mode}_ID_per_seq'].tolist() and [int(n) for n in res['Length_per_seq']] == z[f'm{mode}_Length_per_seq'].tolist()
    total = max(sum(terms), 1)
    for k in ('STQ', 'AQ', 'IoU'):
        want = float(z[f'm{mode}_{k}'])
        assert abs(float(res[k]) - want) <= total * 2.0 ** -52 * abs(want), f'{what}: {k} = {float(res[k])!r}, the reference has {want!r}'
    for k in ('STQ_per_seq', 'AQ_per_seq', 'IoU_per_seq'):
        want, got = z[f'm{mode}_{k}'], np.asarray(res[k], dtype=np.float64)
        assert got.shape == want.shape
        for s in range(len(want)):
            assert abs(got[s] - want[s]) <= max(terms[s], 1) * 2.0 ** -52 * abs(want[s]), f'{what}: {k}[{s}] = {got[s]!r}, the reference has {want[s]!r}'
