"""NumPy restatement of the windowed VPQ metric for the tests: the per-pixel rules and the matching of include/vkn_vpq.h in integers
(`update_state`), the scripts' float64 sums (`counts`) and last lines (`result`).  Plain module, no import of the package under test
and none of the reference: tests/test_vpq_refs.py pins it to the fixtures tests/golden/vpq_*.npz, which tools/gen_golden_vpq.py wrote
from the reference itself."""
import os

import numpy as np

ID_RANGE, CLASS_RANGE = 1, 2          # the status bits this restatement can raise (a dict is never full)
DEFAULT_CAPACITY = dict(gt=512, pred=512, pair=2048, log=131072)      # `VPQMeter`'s defaults


class VPQRef:
    def __init__(self, num_classes, things_list, ks=(1,), ign_id=255, label_bit_shift=16, offset=2 ** 30):
        self.n, self.num_cat, self.things, self.ks = num_classes, num_classes + 1, list(things_list), tuple(ks)
        self.ign, self.shift, self.offset = ign_id, label_bit_shift, offset
        assert offset >= self.num_cat << label_bit_shift and list(self.ks) == sorted(set(self.ks))
        self.seqs = {}                # id -> dict, in order of first appearance
        self.largest = dict(gt=0, pred=0, pair=0)       # the most keys any frame's or window's table held

    def _seq(self, sequence_id):
        nk = len(self.ks)
        return self.seqs.setdefault(sequence_id, dict(frames=[], status=0, acc=np.zeros((nk, 3, self.num_cat), np.int64), log=[],
                                                      rows=[[] for _ in range(nk)], trace=[]))

    def update_state(self, gt_sem, gt_ins, pred_sem, pred_ins, sequence_id=0):
        """int maps of one shape: [H,W], or [B,H,W] = B consecutive frames of the sequence"""
        maps = [np.asarray(a).astype(np.int64) for a in (gt_sem, gt_ins, pred_sem, pred_ins)]
        if maps[0].ndim == 2:
            maps = [m[None] for m in maps]
        seq = self._seq(sequence_id)
        for b in range(maps[0].shape[0]):
            gs, gi, ps, pi = (m[b].ravel() for m in maps)
            bad_class = (ps < 0) | (ps >= self.num_cat) | (((gs < 0) | (gs >= self.num_cat)) & (gs != self.ign))
            bad_id = (gi < 0) | (gi >= 1 << self.shift) | (pi < 0) | (pi >= 1 << self.shift)
            seq['status'] |= (CLASS_RANGE if bad_class.any() else 0) | (ID_RANGE if bad_id.any() else 0)
            live = ~bad_class & ~bad_id
            yt, yp = ((gs << self.shift) + gi)[live], ((ps << self.shift) + pi)[live]
            frame = {}
            for name, keys in (('gt', yt), ('pred', yp), ('pair', yt * self.offset + yp)):
                frame[name] = {int(k): int(c) for k, c in zip(*np.unique(keys, return_counts=True))}
                self.largest[name] = max(self.largest[name], len(frame[name]))
            seq['frames'].append(frame)
            f = len(seq['frames']) - 1
            for i, k in enumerate(self.ks):
                if f + 1 >= k:
                    self._window(seq, i, f + 1 - k, seq['frames'][f + 1 - k:f + 1])

    def _window(self, seq, i, ordinal, frames):
        win = {}
        for name in ('gt', 'pred', 'pair'):
            win[name] = {}
            for fr in frames:
                for key, c in fr[name].items():
                    win[name][key] = win[name].get(key, 0) + c
            self.largest[name] = max(self.largest[name], len(win[name]))
        gt, pred, pair = win['gt'], win['pred'], win['pair']
        iou, tp, fn, fp = (np.zeros((self.num_cat,), np.float64) for _ in range(4))
        void_id = self.ign << self.shift
        gt_matched, pred_matched, events = set(), set(), []
        for key in sorted(pair):
            ia = pair[key]
            gt_id, pred_id = key // self.offset, key % self.offset
            cat = gt_id >> self.shift
            if cat != pred_id >> self.shift:
                continue
            void = pair.get(void_id * self.offset + pred_id, 0)
            union = gt[gt_id] + pred[pred_id] - ia - void
            hit = 2 * ia > union
            events.append(('pair', cat, ia, union, void, hit))
            if hit:
                tp[cat] += 1
                iou[cat] += np.int64(ia) / np.int64(union)
                gt_matched.add(gt_id)
                pred_matched.add(pred_id)
                seq['acc'][i, 0, cat] += 1
                seq['log'].append(((i << 48) | ordinal, key, ia, union))
        for gt_id in gt:
            cat = gt_id >> self.shift
            if gt_id not in gt_matched and cat != self.ign:
                fn[cat] += 1
                seq['acc'][i, 1, cat] += 1
        ign_ids = [g for g in gt if g >> self.shift == self.ign]
        for pred_id, area in pred.items():
            if pred_id in pred_matched:
                continue
            ignored = sum(pair.get(g * self.offset + pred_id, 0) for g in ign_ids)
            events.append(('pred', pred_id >> self.shift, ignored, area, 2 * ignored > area))
            if 2 * ignored > area:
                continue
            fp[pred_id >> self.shift] += 1
            seq['acc'][i, 2, pred_id >> self.shift] += 1
        seq['rows'][i].append((iou, tp, fn, fp))
        seq['trace'].append(dict(k=self.ks[i], ordinal=ordinal, ign_ids=ign_ids, events=events))

    def tables(self, sequence_id=0):
        """acc int64 [nk, 3, num_cat], the TP records int64 [n, 4] sorted by their first two fields, frames, status"""
        seq = self.seqs[sequence_id]
        log = np.array(sorted(seq['log']), dtype=np.int64).reshape(-1, 4)
        return dict(acc=seq['acc'].copy(), log=log, frames=len(seq['frames']), status=seq['status'])

    def rows(self, sequence_id, i):
        """the four per-window arrays of window length index i, each float64 [windows, num_cat]"""
        rows = self.seqs[sequence_id]['rows'][i]
        return tuple(np.stack([r[m] for r in rows]) if rows else np.zeros((0, self.num_cat), np.float64) for m in range(4))

    def counts(self):
        """per window length: iou, tp, fn, fp float64 [num_cat]: the rows of all sequences concatenated and summed"""
        out = []
        for i in range(len(self.ks)):
            every = [np.concatenate([self.rows(sid, i)[m] for sid in self.seqs], axis=0).sum(axis=0) for m in range(4)]
            out.append(dict(zip(('iou', 'tp', 'fn', 'fp'), every)))
        return out

    def result(self):
        things = np.zeros((self.n,), bool)
        things[self.things] = True
        out = {}
        for k, c in zip(self.ks, self.counts()):
            iou, tp, fn, fp = (c[m][:self.n] for m in ('iou', 'tp', 'fn', 'fp'))
            sq = iou / (tp + 1e-10)
            rq = tp / (tp + 0.5 * fn + 0.5 * fp + 1e-10)
            pq = sq * rq
            out[k] = dict(PQ=pq.mean(), PQ_thing=pq[things].mean(), PQ_stuff=pq[~things].mean(), sq=sq, rq=rq, pq=pq)
        out['VPQ'] = np.mean([out[k]['PQ'] for k in self.ks])
        return out


# ---- seeded inputs shared by tests/test_vpq_refs.py (the premises) and tests/test_gpu_vpq.py (the runs)
KITTI = dict(num_classes=19, things_list=[11, 13], ks=(1, 2, 4))
LONG = dict(seed=51, F=10, H=96, W=312, cell=12)        # 29952 pixels: 15 spans per frame, the last one short
SMALL = dict(seed=52, F=6, H=23, W=39, cell=4)          # 897 pixels, odd: frame bases that no 16-byte load can start at
LDS_OVERFLOW = dict(seed=54, F=1, H=96, W=96, n_ids=256, capacity=dict(gt=1024, pred=1024, pair=16384))     # noisy_maps: more keys per span than LDS slots
NOISY = dict(seed=53, F=2, H=16, W=24)                  # per-pixel random segments: more keys than 16 slots of any table


def video_maps(seed, F, H, W, cell=8, cfg=KITTI, ids=4, keep=0.9, hit=0.75, ign_id=255):
    """gt_sem, gt_ins, pred_sem, pred_ins int32 [F,H,W]: `cell` x `cell` segments; a frame's ground truth is the frame before with a share
    redrawn, the prediction the ground truth with a share redrawn; some ignored ground truth, with and without an instance part"""
    rng = np.random.default_rng(seed)
    hb, wb, nc = -(-H // cell), -(-W // cell), cfg['num_classes']
    up = lambda a: np.kron(a, np.ones((cell, cell), np.int64))[:H, :W]      # noqa: E731
    draw = lambda: (rng.integers(0, nc + 1, (hb, wb)), rng.integers(0, ids, (hb, wb)))      # noqa: E731  (class nc: the last bin)
    gsem, gins = draw()
    out = []
    for _ in range(F):
        nsem, nins = draw()
        stay = rng.random((hb, wb)) < keep
        gsem, gins = np.where(stay, gsem, nsem), np.where(stay, gins, nins)
        nsem, nins = draw()
        same = rng.random((hb, wb)) < hit
        psem, pins = np.where(same, gsem, nsem), np.where(same, gins, nins)
        void = rng.random((hb, wb))
        gs, gi = np.where(void < 0.08, ign_id, gsem), np.where(void < 0.04, 0, gins)
        gs, gi, ps, pi = up(gs), up(gi), up(psem), up(pins)
        gi = np.where(np.isin(gs, cfg['things_list'] + [ign_id]), gi, 0)
        pi = np.where(np.isin(ps, cfg['things_list']), pi, 0)
        out.append(np.stack([gs, gi, ps, pi]))
    m = np.stack(out).astype(np.int32)
    return tuple(np.ascontiguousarray(m[:, j]) for j in range(4))


def noisy_maps(seed, F, H, W, cfg=KITTI, n_ids=64):
    """per-pixel random things with `n_ids` ids each side, the prediction equal to the ground truth on half of the pixels"""
    rng = np.random.default_rng(seed)
    things = np.array(cfg['things_list'])
    gs, gi = things[rng.integers(0, len(things), (F, H, W))], rng.integers(1, n_ids + 1, (F, H, W))
    same = rng.random((F, H, W)) < 0.5
    ps, pi = np.where(same, gs, things[rng.integers(0, len(things), (F, H, W))]), np.where(same, gi, rng.integers(1, n_ids + 1, (F, H, W)))
    return tuple(a.astype(np.int32) for a in (gs, gi, ps, pi))


# ---- the fixtures tests/golden/vpq_<case>.npz (tools/gen_golden_vpq.py)
CASES = ('kitti', 'vipseg', 'edges')
ROW_KEYS = ('iou', 'tp', 'fn', 'fp')


def load_case(name):
    """(constructor arguments, sequence ids, the four maps [S,F,H,W], the npz)"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', f'vpq_{name}.npz'))
    args = dict(num_classes=int(z['num_classes']), things_list=[int(t) for t in z['things']], ks=tuple(int(k) for k in z['ks']),
                ign_id=int(z['ign_id']), label_bit_shift=int(z['label_bit_shift']), offset=int(z['offset']))
    return args, [int(s) for s in z['seq_ids']], tuple(z[k] for k in ('gt_sem', 'gt_ins', 'pred_sem', 'pred_ins')), z


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def assert_counts(counts, z, what):
    """`counts()` against the fixture's totals: every float64 bit for bit"""
    assert len(counts) == len(z['ks'])
    for i, c in enumerate(counts):
        for m in ROW_KEYS:
            assert same_bits(c[m], z[f'k{i}_{m}']), f'{what}: {m} of window length index {i} differs'


def assert_result(res, z, what):
    ks = [int(k) for k in z['ks']]
    assert list(res) == ks + ['VPQ']
    for i, k in enumerate(ks):
        for m in ('PQ', 'PQ_thing', 'PQ_stuff'):
            assert same_bits(res[k][m], z[f'k{i}_{m}']), f'{what}: {m} at k = {k}: {res[k][m]!r}, the reference has {float(z[f"k{i}_{m}"])!r}'
        assert all(res[k][m].shape == (int(z['num_classes']),) for m in ('sq', 'rq', 'pq'))
    assert same_bits(res['VPQ'], np.mean([z[f'k{i}_PQ'] for i in range(len(ks))])), what


def assert_same_tables(got, want, what):
    assert got['acc'].dtype == np.int64 and got['acc'].shape == want['acc'].shape and np.array_equal(got['acc'], want['acc']), f'{what}: acc differs'
    assert got['log'].dtype == np.int64 and got['log'].shape == want['log'].shape and np.array_equal(got['log'], want['log']), f'{what}: the TP log differs'
    assert got['frames'] == want['frames'] and got['status'] == want['status'], f'{what}: frames / status'
