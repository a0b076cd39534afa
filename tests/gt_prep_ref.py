"""NumPy restatement of the ground-truth preparation of a training step (`vkn.GtPrep`, include/vkn_gt.h), float64 where arithmetic
occurs, and the cases its tests share: the fixtures tests/golden/gt_prep_*.npz (inputs and the reference's own outputs, written by
tools/gen_golden_gt_prep.py) and hand-built edge cases.  Checked against the fixtures in tests/test_gt_prep_refs.py."""
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FIXTURES = ('city_s4', 'vipseg_s4', 'kitti_s2', 'generic_s8', 'generic_s1', 'nosem_s2')
STATUS_RANGE = 1


# ------------------------------------------------------------------------------------------------------------- the restatement
def table(dataset, T, S, ignore=255, things=None):
    """label of semantic class c = 0..255, -1: not listed (the three `sem2ins_masks*` variants)"""
    out = np.full(256, -1, np.int64)
    for c in range(256):
        if c == ignore:
            continue
        if dataset == 'generic':
            if c != (0 if things is None else things):
                out[c] = c + T - 1
        elif dataset == 'kitti_step':
            th = (11, 13) if things is None else things
            if c not in th:
                out[c] = c - sum(c > t for t in th) + 2
        else:
            if not (S <= c < S + T if things is None else c in things):
                out[c] = c + T
    return out


def down(x, s):
    """bilinear, align_corners=False, to 1 / s at s = 1 or even: the mean of the 2 x 2 centre pixels of every s x s cell.  [N,H,W] float64"""
    if s == 1:
        return x.copy()
    assert s % 2 == 0 and x.shape[1] % s == 0 and x.shape[2] % s == 0
    o = s // 2 - 1
    return (x[:, o::s, o::s] + x[:, o::s, o + 1::s] + x[:, o + 1::s, o::s] + x[:, o + 1::s, o + 1::s]) * 0.25


def prepare(masks, sem, valid, pad, s, tab):
    """masks: per image uint8 [G,Hm,Wm]; sem [B,Hp,Wp] integer or None; valid: per image (h, w); tab: `table(...)`.
    -> namespace(bank fp32 [G_total,aH,aW], thing_row0, sem_row0, n_sem, classes, labels (per image int64), status)"""
    Hp, Wp = pad
    rows, thing_row0, sem_row0, n_sem, classes, labels, status = [], [], [], [], [], [], 0
    row = 0
    for b, m in enumerate(masks):
        full = np.zeros((m.shape[0], Hp, Wp), np.float64)
        full[:, :m.shape[1], :m.shape[2]] = m
        thing_row0.append(row)
        rows.append(down(full, s))
        row += m.shape[0]
        sem_row0.append(row)
        listed = []
        if sem is not None:
            seg = sem[b].astype(np.int64)
            if ((seg < 0) | (seg > 255)).any():
                status |= STATUS_RANGE
            seg = np.where((seg < 0) | (seg > 255), -1, seg)
            seg[valid[b][0]:, :] = -1
            seg[:, valid[b][1]:] = -1
            listed = [int(c) for c in np.unique(seg) if c >= 0 and tab[c] >= 0]
            if listed:
                rows.append(down(np.stack([(seg == c).astype(np.float64) for c in listed]), s))
        n_sem.append(len(listed))
        classes.append(listed)
        labels.append(np.array([tab[c] for c in listed], np.int64))
        row += len(listed)
    bank = np.concatenate(rows).astype(np.float32) if rows else np.zeros((0, Hp // s, Wp // s), np.float32)
    return types.SimpleNamespace(bank=bank, thing_row0=thing_row0, sem_row0=sem_row0, n_sem=n_sem, classes=classes, labels=labels,
                                 status=status)


def match(keys, refs):
    """per image: the first position of every key id among the reference ids, else -1"""
    out = []
    for k, r in zip(keys, refs):
        r = list(np.asarray(r).tolist())
        out.append(np.array([r.index(i) if i in r else -1 for i in np.asarray(k).tolist()], np.int64))
    return out


# ----------------------------------------------------------------------------------------------------------------- the cases
class Bitmap:
    """mmdet's BitmapMasks as far as `preprocess_gt_masks` reads it"""

    def __init__(self, masks):
        self.masks, self.height, self.width = masks, int(masks.shape[1]), int(masks.shape[2])


def case(name, dataset, stride, pad, T, S, things, masks, img_shape, sem, **out):
    return types.SimpleNamespace(name=name, dataset=dataset, stride=int(stride), pad=(int(pad[0]), int(pad[1])), T=int(T), S=int(S),
                                 things=things, masks=masks, img_shape=[(int(h), int(w)) for h, w in img_shape], sem=sem, B=len(masks),
                                 **out)


def load(name):
    """a fixture: the inputs and out_masks / out_sem_cls / out_sem_seg, what the reference returned (None without a map)"""
    g = np.load(os.path.join(GOLDEN, f'gt_prep_{name}.npz'))
    B = int(g['B'])
    sem = g['sem'] if 'sem' in g.files else None
    things = int(g['things'])
    return case(name, str(g['dataset']), g['stride'], g['pad'], g['T'], g['S'], None if things < 0 else things,
                [g[f'masks{b}'] for b in range(B)], [g[f'img_shape{b}'] for b in range(B)], sem,
                out_masks=[g[f'out_masks{b}'] for b in range(B)],
                out_sem_cls=None if sem is None else [g[f'out_sem_cls{b}'] for b in range(B)],
                out_sem_seg=None if sem is None else [g[f'out_sem_seg{b}'] for b in range(B)])


def reference(c):
    return prepare(c.masks, c.sem, c.img_shape, c.pad, c.stride, table(c.dataset, c.T, c.S, 255, c.things))


def metas(c):
    return [dict(batch_input_shape=c.pad, img_shape=c.img_shape[b] + (3,)) for b in range(c.B)]


def make_prep(vkn, c):
    return vkn.GtPrep(c.stride, c.T, c.S, ignore_label=255, dataset=c.dataset, thing_label_in_seg=c.things)


def run(vkn, c, device, prep=None):
    """`GtPrep.preprocess_gt_masks` on the case: host bitmap masks, labels and the map on `device` -> (prep, masks, sem_cls, sem_seg)"""
    import torch
    prep = prep or make_prep(vkn, c)
    labels = [torch.zeros(m.shape[0], dtype=torch.int64, device=device) for m in c.masks]
    sem = None if c.sem is None else torch.from_numpy(c.sem.copy())[:, None].to(device)
    return (prep,) + tuple(prep.preprocess_gt_masks(metas(c), [Bitmap(m) for m in c.masks], labels, sem))


def blobs(rng, G, H, W, value=1):
    m = (rng.random((G, H, W)) > 0.6).astype(np.uint8) * value
    m[:, -1, :] = value            # the last row and column are set: a 2 x 2 centre that straddles the mask's edge shows
    m[:, :, -1] = value
    return m


def sem_map(rng, B, H, W, classes, block=5, dtype=np.uint8):
    classes = np.asarray(classes)
    coarse = classes[rng.integers(0, len(classes), (B, (H + block - 1) // block, (W + block - 1) // block))]
    sem = np.repeat(np.repeat(coarse, block, 1), block, 2)[:, :H, :W].copy()
    noise = rng.random((B, H, W)) > 0.93
    sem[noise] = classes[rng.integers(0, len(classes), int(noise.sum()))]
    return sem.astype(dtype)


def class_edges(dtype):
    """stride 4 at pad 32 x 72, img_shape (29, 59), generic with the special thing label 3 (label = c + 3): the centre rows / columns of
    a cell are 1, 2 (mod 4).  Class 9 only inside the ignore region (not listed), class 20 only at non-centre pixels (listed, an
    all-zero row), class 21 at exactly one centre pixel (a single 0.25), classes 0 and 254 present, byte masks holding 255."""
    rng = np.random.default_rng(11)
    sem = np.full((1, 32, 72), 7, dtype)
    sem[0, 30, 5:20] = 9
    sem[0, 5, 62] = 9
    sem[0, 0, 0] = sem[0, 4, 8] = sem[0, 3, 3] = 20
    sem[0, 5, 6] = 21
    sem[0, 8:16, 8:24] = 0
    sem[0, 16:24, 30:50] = 254
    sem[0, 24:29, 0:10] = 255
    sem[0, 27:32, 50:72] = 3
    return case(f'class_edges_{np.dtype(dtype).name}', 'generic', 4, (32, 72), 4, 9, 3, [blobs(rng, 2, 30, 61, value=255)], [(29, 59)], sem)


def out_of_range():
    """an int64 map holding -1 and 300 (and values far outside): the status bit, the pixels count as ignore"""
    rng = np.random.default_rng(12)
    sem = sem_map(rng, 2, 32, 72, [1, 2, 5, 255], dtype=np.int64)
    sem[0, 1, 1], sem[0, 2, 2], sem[1, 5, 6], sem[1, 9, 9] = -1, 300, 2 ** 40, -2 ** 40
    return case('out_of_range', 'cityscapes', 4, (32, 72), 8, 11, None, [blobs(rng, 1, 32, 72), blobs(rng, 2, 32, 72)],
                [(32, 72), (32, 72)], sem)


def aligned(s, dtype):
    """pad 64 x 128: every row pitch is a multiple of 4 s and of 16, so the vector loads and stores run; the second image's masks are
    48 x 96 (a vector that ends past the mask), img_shape (61, 117) cuts vectors of the map"""
    rng = np.random.default_rng(20 + s)
    sem = sem_map(rng, 2, 64, 128, [0, 1, 2, 5, 10, 11, 12, 13, 14, 18, 255], dtype=dtype)
    return case(f'aligned_s{s}_{np.dtype(dtype).name}', 'kitti_step', s, (64, 128), 2, 17, None,
                [blobs(rng, 3, 64, 128), blobs(rng, 2, 48, 96, value=255)], [(64, 128), (61, 117)], sem)


def wide():
    """stride 2 at pad 16 x 1040: aW = 520, three column blocks of the fill; four row blocks"""
    rng = np.random.default_rng(31)
    sem = sem_map(rng, 1, 16, 1040, list(range(19)) + [255])
    return case('wide_s2', 'cityscapes', 2, (16, 1040), 8, 11, None, [blobs(rng, 2, 16, 1040)], [(15, 1033)], sem)


def ragged():
    """B = 4 at stride 4, pad 32 x 72: three mask sizes, an image without things, an image whose map is all ignore"""
    rng = np.random.default_rng(32)
    sem = sem_map(rng, 4, 32, 72, list(range(19)) + [255])
    sem[3] = 255
    return case('ragged_s4', 'cityscapes', 4, (32, 72), 8, 11, None,
                [blobs(rng, 2, 30, 61), np.zeros((0, 32, 72), np.uint8), blobs(rng, 3, 17, 40), blobs(rng, 1, 32, 72)],
                [(29, 59), (32, 72), (17, 40), (32, 72)], sem)


EDGE_CASES = {
    'class_edges_uint8': lambda: class_edges(np.uint8), 'class_edges_int64': lambda: class_edges(np.int64),
    'out_of_range': out_of_range, 'wide_s2': wide, 'ragged_s4': ragged,
    **{f'aligned_s{s}_{np.dtype(d).name}': (lambda s=s, d=d: aligned(s, d)) for s in (1, 2, 4, 8) for d in (np.uint8, np.int64)},
}

MATCH_LISTS = [([5, 7, 9, 5], [9, 5, 5]), ([], [1, 2]), ([3, 4], []), ([11, 12, 13], [13, 12, 11, 12])]


def load_match():
    g = np.load(os.path.join(GOLDEN, 'gt_prep_match.npz'))
    n = int(g['n'])
    return [g[f'key{i}'] for i in range(n)], [g[f'ref{i}'] for i in range(n)], [g[f'pids{i}'] for i in range(n)]
