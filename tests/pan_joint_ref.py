"""Float64 reference of the joint panoptic merge (`vkn_panoptic_joint_f32`, include/vkn.h) with its tie rules written out, and seeded
builders of inputs whose answer is DECIDED: every pixel's arg-max and every `prob >= 0.5` test hold with a float64 margin of at least
FLOOR, so that the library's int32 outputs can be compared with `array_equal` (tests/test_gpu_pan_joint_pins.py).  The premises — the
margins, the agreement with oracle.knet_oracle.panoptic_joint, the survivor counts of the dense cases, the pixel counts of the crisp
cases — are asserted on the CPU by tests/test_pan_joint_refs.py.  No GPU in this file."""
import numpy as np
import torch
import torch.nn.functional as F

FLOOR = 1e-4          # 100 x the 1e-6 that helpers.assert_pan_matches_oracle treats as fp32 resampling noise
TILE_W, TILE_H = 64, 16   # output tile of k_pan_argmax (csrc/vkn_panoptic.hip)
EMPTY_BOX = (-1, -1, 10, 10)


def _stable_desc(scores):
    """indices by (score descending, index ascending)"""
    return np.argsort(-np.asarray(scores, dtype=np.float64), kind='stable')


def joint_ref(cls, logits, Np, T, Kt, inst_thr, overlap_thr, meta, up):
    """One frame in float64: oracle.knet_oracle.panoptic_joint restated with the documented tie rules — (score descending, flat index
    ascending) for the thing top-k, the stuff sort and the merge order; first maximum for the arg-max — returning what the ABI returns.
    cls [N, ncls] fp32 probabilities, logits [N, Hm, Wm] fp32.  Scores stay the fp32 values (as float64); the thing threshold is tested
    in fp32, the overlap ratio in Python floats."""
    cls = np.asarray(cls.detach().cpu().numpy() if torch.is_tensor(cls) else cls)
    assert cls.dtype == np.float32
    lg = torch.as_tensor(logits).detach().cpu()
    N = cls.shape[0]
    nstuff = N - Np
    # selection
    thing = cls[:Np, :T].reshape(-1)
    tsel = _stable_desc(thing)[:Kt]
    ssc = np.array([cls[Np + j, T + j] for j in range(nstuff)], dtype=np.float32)
    ssel = _stable_desc(ssc)
    sel_row = np.concatenate([tsel // T, Np + ssel]).astype(np.int32)
    sel_label = np.concatenate([tsel % T, T + ssel]).astype(np.int32)
    sel_score = np.concatenate([thing[tsel], ssc[ssel]]).astype(np.float32)
    K = sel_row.shape[0]
    # resampling chain
    x = lg.double()[torch.from_numpy(sel_row).long()][None]
    if up > 1:
        x = F.interpolate(x, scale_factor=up, mode='bilinear', align_corners=False)
    h, w = meta['img_shape'][:2]
    x = F.interpolate(x.sigmoid(), size=tuple(meta['batch_input_shape']), mode='bilinear', align_corners=False)[:, :, :h, :w]
    prob = F.interpolate(x, size=tuple(meta['ori_shape'][:2]), mode='bilinear', align_corners=False)[0].numpy()
    prod = sel_score.astype(np.float64)[:, None, None] * prob
    ids = prod.argmax(0).astype(np.int32)                         # numpy: the first maximum
    area = np.bincount(ids.reshape(-1), minlength=K).astype(np.int32)
    orig = (prob >= 0.5).reshape(K, -1).sum(1).astype(np.int32)
    # margins: entries of one duplicate class (bit-equal score, bit-identical plane) are bitwise equal everywhere by construction
    planes = lg.numpy()
    keys = {}
    dup = np.array([keys.setdefault((sel_score[k].tobytes(), planes[sel_row[k]].tobytes()), len(keys)) for k in range(K)])
    other = np.where(dup[:, None, None] == dup[ids][None], -np.inf, prod)
    margin = float((prod.max(0) - other.max(0)).min()) if len(keys) > 1 else float('inf')
    half_margin = float(np.abs(prob - 0.5).min())
    # merge
    seg_of = np.zeros(K, dtype=np.int32)
    cur = 0
    for k in _stable_desc(sel_score):
        if sel_label[k] < T and sel_score[k] < np.float32(inst_thr):
            continue
        a, o = int(area[k]), int(orig[k])
        if a > 0 and o > 0 and not (a / o < overlap_thr):
            cur += 1
            seg_of[k] = cur
    seg = seg_of[ids].astype(np.int32)
    bbox = np.tile(np.array(EMPTY_BOX, dtype=np.int32), (K, 1))
    for k in np.nonzero(seg_of)[0]:
        ys, xs = np.nonzero(ids == k)
        bbox[k] = (xs.min(), ys.min(), xs.max(), ys.max())
    info = np.stack([sel_row, sel_label, seg_of, area, orig, sel_score.view(np.int32)], 1).astype(np.int32)
    return dict(sel_row=sel_row, sel_label=sel_label, sel_score=sel_score, ids=ids, area=area, orig=orig, seg_of=seg_of,
                panoptic_seg=seg, nseg=cur, bbox=bbox, info=info, margin=margin, half_margin=half_margin)


def case_ref(case, **over):
    a = {**case, **over}
    return joint_ref(a['cls'], a['logits'], a['Np'], a['T'], a['Kt'], a['inst_thr'], a['overlap_thr'], a['meta'], a['up'])


def _meta(img, bis, ori):
    return dict(img_shape=(img[0], img[1], 3), batch_input_shape=tuple(bis), ori_shape=(ori[0], ori[1], 3))


def _case(cls, logits, Np, T, Kt, meta, up, inst_thr=0.25, overlap_thr=0.6):
    return dict(cls=torch.from_numpy(np.ascontiguousarray(cls, dtype=np.float32)),
                logits=torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)), Np=Np, T=T, Kt=Kt, meta=meta, up=up,
                inst_thr=inst_thr, overlap_thr=overlap_thr)


# ------------------------------------------------------------------------------------------------------------------ partition cases
def partition_case(Hm, Wm, up, bis, img, ori, Np, T, nstuff, seed, Kt=None, cell=3, low_rows=0):
    """Every selected row owns cells of the low-res map (cut into `cell` x `cell` cells): logit +8 in its cells, -8 elsewhere, plus
    uniform noise of +-0.5.  Scores are a permutation of an evenly spaced grid in (0.15, 0.95), so no two are equal.  (With 15 rows
    the grid step is 0.05 and one score is exactly 0.25f, the shipped thing threshold: kept if it falls on a thing.)
    Kt None: max_per_img = Np; every thing row has ONE grid score (random class), its other class scores are <= 0.03.
    Kt given (> Np): every (row, class) pair has a grid score — rows are selected up to T times; the `low_rows` first rows take the
    lowest SELECTED grid values, so that entries at the end of the thing selection are their row's best and win its cells."""
    rng = np.random.default_rng(seed)
    N, ncls = Np + nstuff, T + nstuff
    cls = rng.uniform(0.0, 0.03, size=(N, ncls)).astype(np.float32)
    if Kt is None:
        Kt = Np
        grid = rng.permutation(np.linspace(0.15, 0.95, N + 2)[1:-1])
        cls[np.arange(Np), rng.integers(0, T, Np)] = grid[:Np]
        stuff_scores = grid[Np:]
    else:
        grid = np.sort(np.linspace(0.15, 0.95, Np * T + nstuff + 2)[1:-1])[::-1]
        pick = rng.permutation(Np * T + nstuff)
        stuff_scores = grid[pick[:nstuff]]
        tv = np.sort(grid[pick[nstuff:]])[::-1]                           # the thing values, descending: the first Kt are selected
        low = tv[Kt - low_rows * T:Kt]
        rest = rng.permutation(np.concatenate([tv[:Kt - low_rows * T], tv[Kt:]]))
        cls[:Np, :T] = np.concatenate([rng.permutation(low), rest]).reshape(Np, T)
    cls[Np + np.arange(nstuff), T + np.arange(nstuff)] = stuff_scores
    # rows that will be selected, then one owner per cell (every such row first, while cells last)
    thing = cls[:Np, :T].reshape(-1)
    rows = np.unique(np.concatenate([_stable_desc(thing)[:Kt] // T, Np + np.arange(nstuff)]))
    ncy, ncx = -(-Hm // cell), -(-Wm // cell)
    ncell = ncy * ncx
    must = np.arange(low_rows)
    owners = np.concatenate([must, rng.permutation(np.setdiff1d(rows, must)), rng.choice(rows, size=max(ncell - rows.size, 0))])[:ncell]
    owners = rng.permutation(owners).reshape(ncy, ncx)
    own = np.repeat(np.repeat(owners, cell, 0), cell, 1)[:Hm, :Wm]
    logits = np.where(own[None] == np.arange(N)[:, None, None], 8.0, -8.0) + rng.uniform(-0.5, 0.5, size=(N, Hm, Wm))
    return _case(cls, logits, Np, T, Kt, _meta(img, bis, ori), up)


def dense_case(Hm, Wm, Np, nstuff, seed, cell=3):
    """A crowded frame for the survivor chunks of k_pan_argmax: a partition case at identity geometry (up = 1, output = logits) whose
    cell owners are drawn from ALL Np + nstuff rows, so that one 64 x 16 tile holds the cells of dozens of kernels."""
    return partition_case(Hm, Wm, 1, (Hm, Wm), (Hm, Wm), (Hm, Wm), Np, 2, nstuff, seed, cell=cell)


def live_lower_bound(case):
    """[tile rows, tile columns]: the number of selected kernels whose logit is >= 0 somewhere strictly inside the tile's own pixels.
    Identity geometry only (the footprint of a tile contains the tile): such a kernel reaches prob >= 0.5 there, so whatever the prune
    rule is, it must keep it."""
    Hm, Wm = case['logits'].shape[-2:]
    assert case['up'] == 1 and tuple(case['meta']['batch_input_shape']) == tuple(case['meta']['ori_shape'][:2]) == (Hm, Wm)
    r = case_ref(case)
    lg = case['logits'].numpy()[r['sel_row']]
    nty, ntx = -(-Hm // TILE_H), -(-Wm // TILE_W)
    return np.array([[int((lg[:, ty * TILE_H:(ty + 1) * TILE_H, tx * TILE_W:(tx + 1) * TILE_W] >= 0).any((1, 2)).sum())
                      for tx in range(ntx)] for ty in range(nty)])


# ---------------------------------------------------------------------------------------------------------------------- crisp cases
def crisp_case(H, W, things, stuff, T=2, Kt=None, inst_thr=0.25, overlap_thr=0.6, lo=-30.0):
    """Identity geometry, logits `lo` with rectangles at +30 (sigmoid = 1.0 / 1e-13 in fp32 and float64 alike): areas and overlaps are
    pixel counts.  things: one (scores {class: score}, rects) per proposal row; stuff: one (score, rects) per stuff row; a rect is
    (y0, y1, x0, x1), ends exclusive, or (y0, y1, x0, x1, level) for another logit than +30.  Unlisted class scores are 0;
    max_per_img defaults to the number of listed (row, class) pairs."""
    Np, nstuff = len(things), len(stuff)
    cls = np.zeros((Np + nstuff, T + nstuff), dtype=np.float32)
    logits = np.full((Np + nstuff, H, W), lo, dtype=np.float32)
    for i, (scores, rects) in enumerate(list(things) + [({T + j: s}, r) for j, (s, r) in enumerate(stuff)]):
        for c, s in scores.items():
            cls[i, c] = s
        for rc in rects:
            logits[i, rc[0]:rc[1], rc[2]:rc[3]] = rc[4] if len(rc) > 4 else 30.0
    if Kt is None:
        Kt = sum(len(s) for s, _ in things)
    return _case(cls, logits, Np, T, Kt, _meta((H, W), (H, W), (H, W)), 1, inst_thr, overlap_thr)


# ------------------------------------------------------------------------------------------------------------------- the pinned cases
# name: (Hm, Wm, up, batch_input, img, ori).  Seeds: the first of 0..11 at which tests/test_pan_joint_refs.py's premises hold.
GEOMS = {
    'partial_tile_x2': (5, 9, 1, (10, 18), (10, 18), (10, 18)),            # one partial tile, level 1 x2 up
    'three_levels_up': (8, 16, 2, (64, 128), (60, 120), (90, 180)),        # three levels, up-scale, ragged 90 % 16, 180 % 64
    'down_under_a_tile': (6, 10, 4, (48, 80), (45, 77), (17, 29)),         # x2.65 down, output under one tile
    'anisotropic': (7, 20, 2, (56, 160), (50, 150), (131, 67)),            # rows x2.6 up, columns x2.2 down
    'crop_only': (9, 40, 4, (36, 160), (33, 150), (33, 150)),              # two levels, level-1 identity, crop only
    'level1_down': (12, 40, 4, (24, 80), (24, 80), (24, 80)),              # level 1 DOWN-scales (up * Hm = 2 Hb)
    'one_row': (1, 33, 2, (8, 264), (8, 264), (8, 264)),                   # one-row logits, Ho < 16
    'one_column': (33, 1, 2, (264, 8), (264, 8), (264, 8)),                # one-column logits, Wo < 64
    'ragged_1': (16, 65, 1, (16, 65), (16, 65), (17, 129)),                # Wo % 64 = 1, Ho % 16 = 1
    'ragged_63_15': (8, 32, 2, (16, 64), (15, 63), (31, 127)),             # Wo % 64 = 63, Ho % 16 = 15
}
K15 = dict(Np=10, T=2, nstuff=5)       # K = 15
K60 = dict(Np=40, T=2, nstuff=20)      # K = 60
# case name -> (geometry, rows, seed)
SWEEP = {
    'partial_tile_x2': ('partial_tile_x2', K15, 4),
    'three_levels_up': ('three_levels_up', K15, 8),
    'three_levels_up_k60': ('three_levels_up', K60, 5),
    'down_under_a_tile': ('down_under_a_tile', K15, 4),
    'down_under_a_tile_k60': ('down_under_a_tile', K60, 2),
    'anisotropic': ('anisotropic', K15, 6),
    'crop_only': ('crop_only', K15, 0),
    'level1_down': ('level1_down', K15, 0),
    'one_row': ('one_row', K15, 4),
    'one_column': ('one_column', K15, 4),
    'ragged_1': ('ragged_1', K15, 0),
    'ragged_63_15': ('ragged_63_15', K15, 5),
    # second frames of the B = 2 runs
    'three_levels_up_b': ('three_levels_up', K15, 10),
    'ragged_63_15_b': ('ragged_63_15', K15, 11),
}
PAIRS = [('three_levels_up', 'three_levels_up_b'), ('ragged_63_15', 'ragged_63_15_b')]    # B = 2: two frames of one geometry


def sweep_case(name):
    geom, rows, seed = SWEEP[name]
    return partition_case(*GEOMS[geom], seed=seed, **rows)


# survivor chunks: name -> (Hm, Wm, Np, nstuff, seed, cell, live kernels one tile must reach)
DENSE = {
    'dense_k60': (16, 64, 40, 20, 0, 3, 33),        # one tile, K = 60: a second chunk of 32 survivors
    'dense_k117': (32, 128, 100, 17, 0, 2, 65),     # 2 x 2 tiles, K = 117: three chunks
}


def dense(name):
    Hm, Wm, Np, nstuff, seed, cell, _ = DENSE[name]
    return dense_case(Hm, Wm, Np, nstuff, seed, cell)


K300_SEED = 0


def k300_case():
    """K = 300 > 256 (k_pan_argmax's `k += 256` second trip): 100 proposals x 3 classes, max_per_img = 280, 20 stuff rows, 9 x 40
    logits; 8 rows hold the 24 lowest selected thing scores, so entries 256.. of the selection win their rows' cells."""
    return partition_case(9, 40, 4, (36, 160), (33, 150), (33, 150), 100, 3, 20, K300_SEED, Kt=280, cell=2, low_rows=8)


# ---- threshold edges: one crisp frame, 24 x 80 (2 x 2 tiles, ragged), thing rows 0..8 in the order below, T = 2
Q = float(np.float32(0.25))
Q_BELOW = float(np.nextafter(np.float32(0.25), np.float32(0)))
EDGE_THINGS = [
    ({0: 0.90}, [(2, 3, 2, 21)]),          # 0 A: 19 px, the higher-scored neighbour of C
    ({1: 0.70}, [(2, 3, 17, 27)]),         # 1 C: 10 px, 4 under A -> 6 / 10
    ({0: 0.60}, [(5, 6, 2, 12)]),          # 2 D: 10 px, 5 under E -> 5 / 10
    ({1: 0.85}, [(5, 6, 7, 17)]),          # 3 E: 10 px
    ({0: Q}, [(8, 9, 60, 68)]),            # 4 F: score exactly 0.25f, 8 px across the tile border x = 64
    ({0: Q_BELOW}, [(8, 9, 70, 75)]),      # 5 G: the fp32 value below 0.25f, 5 px
    ({1: 0.50}, [(18, 19, 2, 7)]),         # 6 H: 5 px entirely under I
    ({0: 0.95}, [(17, 20, 0, 9)]),         # 7 I: 27 px
    ({1: 0.92}, [(20, 23, 66, 78, -1.0)]), # 8 X: logit -1 (prob 0.27) where every other kernel is at -30: 36 px, orig 0
]
EDGE_STUFF = [
    (0.01, [(0, 24, 0, 80), (20, 23, 66, 78, -30.0)]),      # 9 background: everywhere but X's hole; kept although 0.01 < 0.25
    (0.88, [(12, 16, 30, 70)]),                              # 10 S: 160 px
]


def edge_case(overlap_thr=0.6):
    return crisp_case(24, 80, EDGE_THINGS, EDGE_STUFF, overlap_thr=overlap_thr)


# entry order = selection order (things by score, then stuff by score):
#   0 I .95   1 X .92   2 A .90   3 E .85   4 C .70   5 D .60   6 H .50   7 F .25   8 G <.25   9 S .88   10 background .01
EDGE_AREA = [27, 36, 19, 10, 6, 5, 0, 8, 5, 160, 24 * 80 - 36 - (27 + 19 + 10 + 6 + 5 + 8 + 5 + 160)]
EDGE_ORIG = [27, 0, 19, 10, 10, 10, 5, 8, 5, 160, 24 * 80 - 36]
EDGE_SEG = [1, 0, 2, 4, 5, 0, 0, 6, 0, 3, 7]           # ids count accepted entries in score order across things and stuff
EDGE_SEG_F32_THR = [1, 0, 2, 4, 0, 0, 0, 5, 0, 3, 6]   # overlap_thr = float(float32(0.6)) > 6 / 10: C is rejected too


# ---- ties (crisp, 16 x 64: one tile; K >= 4)
def tie_same_row_case():
    """proposal 1 has bit-equal scores in both thing classes: its mask is selected twice"""
    return crisp_case(16, 64, [({1: 0.9}, [(1, 5, 1, 9)]), ({0: 0.7, 1: 0.7}, [(6, 10, 20, 40)]), ({0: 0.4}, [(12, 15, 50, 60)])],
                      [(0.3, [(0, 16, 0, 64)])])


def tie_stuff_planes_case():
    """stuff rows 1 and 2 (mask rows 3, 4) have bit-identical planes and bit-equal diagonal scores"""
    r = [(4, 12, 8, 40)]
    return crisp_case(16, 64, [({0: 0.9}, [(1, 3, 1, 9)]), ({1: 0.5}, [(13, 15, 50, 60)])], [(0.2, [(0, 16, 0, 64)]), (0.6, r), (0.6, r)])


def tie_scores_case():
    """equal scores on disjoint planes, in things and stuff: only the order columns are at stake"""
    return crisp_case(16, 64, [({1: 0.6}, [(1, 3, 1, 9)]), ({0: 0.6}, [(4, 6, 1, 9)]), ({0: 0.8}, [(7, 9, 1, 9)])],
                      [(0.6, [(10, 12, 1, 9)]), (0.8, [(13, 15, 1, 9)]), (0.6, [(1, 15, 30, 50)]), (0.1, [(0, 16, 0, 64)])])


def zero_scores_case():
    """every score exactly 0.0: all products are 0, entry 0 = (proposal 0, class 0) wins every pixel"""
    return crisp_case(16, 64, [({}, [(1, 5, 1, 9)]), ({}, [(6, 10, 20, 40)])], [(0.0, [(0, 16, 0, 64)]), (0.0, [(2, 4, 2, 4)])], Kt=3)


def few_kernels_case(K):
    """K = 1, 2, 3 selected kernels (fewer than one batch of four), the map cut into K vertical bands"""
    x = {1: [0, 64], 2: [0, 30, 64], 3: [0, 30, 47, 64]}[K]
    things = [({0: 0.9}, [(0, 16, x[0], x[1])]), ({1: 0.8}, [(0, 16, x[1], x[min(K, 2)])])][:min(K, 2)]
    return crisp_case(16, 64, things, [(0.5, [(0, 16, x[2], x[3])])] if K == 3 else [])


# ------------------------------------------------------------------------------------------------------------------------ registry
CASES = {**{n: (lambda n=n: sweep_case(n)) for n in SWEEP}, **{n: (lambda n=n: dense(n)) for n in DENSE}, 'k300': k300_case,
         'edges': edge_case, 'edges_f32_thr': lambda: edge_case(float(np.float32(0.6))),
         'tie_same_row': tie_same_row_case, 'tie_stuff_planes': tie_stuff_planes_case, 'tie_scores': tie_scores_case,
         'zero_scores': zero_scores_case, **{f'few_{K}': (lambda K=K: few_kernels_case(K)) for K in (1, 2, 3)}}
FLOORED = list(SWEEP) + list(DENSE) + ['k300', 'edges', 'edges_f32_thr']     # the cases whose margins must reach FLOOR
_CACHE = {}


def get(name):
    """(case, its joint_ref result), built once per process and shared: treat both as read-only"""
    if name not in _CACHE:
        case = CASES[name]()
        _CACHE[name] = (case, case_ref(case))
    return _CACHE[name]
