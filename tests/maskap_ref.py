"""COCO mask AP restated in plain loops over boolean NumPy masks: the yardstick of the device meter (include/vkn_maskap.h states the
rules).  pycocotools is not available, so this is a restatement of `COCOeval.evaluateImg`, `accumulate` and `summarize` for
iouType = 'segm', useCats = 1, written independently of video-k-net_amd/mask_ap_meter.py: images are dicts, the matching is one
function per (image, category, area range), and the accumulation walks Python lists.

One stated deviation from pycocotools: an intersection of 0 is IoU 0, with no division."""
import numpy as np

COCO_AREAS = ((0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10))
COCO_THRS = np.arange(0.5, 0.96, 0.05)
COCO_MAX_DETS = (100, 300, 1000)


def overlaps(dt, gt):
    """dt bool [K,H,W], gt bool [G,H,W] -> (inter int64 [K,G], area_dt int64 [K], area_gt int64 [G])"""
    dt, gt = np.asarray(dt, dtype=bool), np.asarray(gt, dtype=bool)
    K, G = dt.shape[0], gt.shape[0]
    inter = np.zeros((K, G), dtype=np.int64)
    for k in range(K):
        for g in range(G):
            inter[k, g] = int(np.count_nonzero(dt[k] & gt[g]))
    area_dt = np.array([int(np.count_nonzero(m)) for m in dt], dtype=np.int64).reshape(K)
    area_gt = np.array([int(np.count_nonzero(m)) for m in gt], dtype=np.int64).reshape(G)
    return inter, area_dt, area_gt


def iou_of(I, ad, ag, crowd):
    if I == 0:
        return 0.0
    U = ad if crowd else ad + ag - I
    return float(np.float64(I) / np.float64(U))


def evaluate_img(tables, scores, dt_labels, gt_labels, gt_crowd, gt_area, cat, rng, thrs, max_det):
    """One (image, category, area range).  -> dict(dt: detection indices in score order (the first max_det), matched / ignored:
    bool [T][len(dt)], gt_of: int [T][len(dt)] (input index or -1), npig)"""
    inter, area_dt, area_gt = tables
    lo, hi = rng
    scores = np.asarray(scores, dtype=np.float32)
    dts = [k for k in range(len(scores)) if int(dt_labels[k]) == cat]
    neg = np.array([-scores[k] for k in dts], dtype=np.float32)
    dts = [dts[i] for i in np.argsort(neg, kind='mergesort')][:max_det]
    gts = [g for g in range(len(gt_labels)) if int(gt_labels[g]) == cat]

    def ignore(g):
        a = float(gt_area[g]) if gt_area is not None else float(area_gt[g])
        return bool(gt_crowd[g]) or a < lo or a > hi
    gts = [g for g in gts if not ignore(g)] + [g for g in gts if ignore(g)]
    g_ig = [ignore(g) for g in gts]
    T = len(thrs)
    matched = [[False] * len(dts) for _ in range(T)]
    ignored = [[False] * len(dts) for _ in range(T)]
    gt_of = [[-1] * len(dts) for _ in range(T)]
    for ti, t in enumerate(thrs):
        taken = [False] * len(gts)
        for di, k in enumerate(dts):
            best, m = min(float(t), 1 - 1e-10), -1
            for gi, g in enumerate(gts):
                if taken[gi] and not gt_crowd[g]:
                    continue
                if m > -1 and not g_ig[m] and g_ig[gi]:
                    break
                v = iou_of(int(inter[k, g]), int(area_dt[k]), int(area_gt[g]), bool(gt_crowd[g]))
                if v < best:
                    continue
                best, m = v, gi
            if m > -1:
                taken[m] = True
                matched[ti][di], ignored[ti][di], gt_of[ti][di] = True, g_ig[m], gts[m]
            else:
                a = float(area_dt[k])
                ignored[ti][di] = a < lo or a > hi
    return dict(dt=dts, matched=matched, ignored=ignored, gt_of=gt_of, npig=sum(1 for x in g_ig if not x))


def image_tables(img):
    """the overlap tables of an image dict: from its masks, or `tables` given by hand"""
    return img['tables'] if 'tables' in img else overlaps(img['dt_masks'], img['gt_masks'])


def evaluate(images, num_classes, thrs=COCO_THRS, areas=COCO_AREAS, max_dets=COCO_MAX_DETS):
    """images: list of dicts(image_id, dt_masks | tables, dt_scores, dt_labels, gt_masks, gt_labels, gt_iscrowd, gt_area or None).
    -> dict(precision [T,101,C,A,M], recall [T,C,A,M], stats [12] or None, classwise [C], npig [C,A])"""
    T, A, M, R = len(thrs), len(areas), len(max_dets), 101
    rec_thrs = np.linspace(0.0, 1.0, R)
    precision, recall = -np.ones((T, R, num_classes, A, M)), -np.ones((T, num_classes, A, M))
    npig_all = np.zeros((num_classes, A), dtype=np.int64)
    images = sorted(images, key=lambda im: im['image_id'])
    tables = [image_tables(im) for im in images]
    for c in range(num_classes):
        for a, rng in enumerate(areas):
            per_img = []
            for im, tab in zip(images, tables):
                G = len(im['gt_labels'])
                crowd = im.get('gt_iscrowd')
                crowd = [0] * G if crowd is None else crowd
                per_img.append((im, evaluate_img(tab, im['dt_scores'], im['dt_labels'], im['gt_labels'], crowd, im.get('gt_area'), c, rng, thrs, max_dets[-1])))
            npig = sum(e['npig'] for _, e in per_img)
            npig_all[c, a] = npig
            if npig == 0:
                continue
            for m, max_det in enumerate(max_dets):
                sc, tm, ti = [], [[] for _ in range(T)], [[] for _ in range(T)]
                for im, e in per_img:
                    n = min(len(e['dt']), max_det)
                    sc += [np.float32(im['dt_scores'][k]) for k in e['dt'][:n]]
                    for t in range(T):
                        tm[t] += e['matched'][t][:n]
                        ti[t] += e['ignored'][t][:n]
                order = np.argsort(-np.array(sc, dtype=np.float32), kind='mergesort') if sc else []
                nd = len(sc)
                for t in range(T):
                    tp = fp = 0
                    rc, pr = [], []
                    for i in order:
                        if not ti[t][i]:
                            tp += 1 if tm[t][i] else 0
                            fp += 0 if tm[t][i] else 1
                        rc.append(float(tp) / npig)
                        pr.append(float(tp) / (float(fp) + float(tp) + np.spacing(1)))
                    recall[t, c, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = [0.0] * R
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side='left')):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, c, a, m] = q
    out = dict(precision=precision, recall=recall, npig=npig_all, stats=None, classwise=np.full((num_classes,), np.nan))
    for c in range(num_classes):
        p = precision[:, :, c, 0, -1]
        p = p[p > -1]
        if p.size:
            out['classwise'][c] = np.mean(p)
    if A == 4 and M == 3:
        def mean_of(s):
            s = s[s > -1]
            return float(np.mean(s)) if s.size else -1.0

        def ap(iou=None, a=0):
            s = precision if iou is None else precision[np.where(iou == np.asarray(thrs))[0]]
            return mean_of(s[:, :, :, a, M - 1])

        def ar(a=0, m=M - 1):
            return mean_of(recall[:, :, a, m])
        out['stats'] = [ap(), ap(0.5), ap(0.75), ap(a=1), ap(a=2), ap(a=3), ar(m=0), ar(m=1), ar(m=2), ar(a=1), ar(a=2), ar(a=3)]
    return out
