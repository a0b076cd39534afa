"""CPU references of the video detector's tracking tail (torch / NumPy), restating
knet/video/knet_quansi_dense_embed_fc_joint_train.py of the reference line by line.  The checkers of tests/test_gpu_track_tail.py and
the subject of tests/test_track_tail_refs.py; nothing here touches the product package.

Inputs are the C-ABI level data of one frame: `seg` int [Ho, Wo] (panoptic map), `info` int [K, 6] = {mask row, joint label, segment
id or 0, area, original area, score bits} as vkn_panoptic_joint_f32 writes it.
"""
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('_standin_unitrack_mask', os.path.join(ROOT, 'oracle', 'standins', 'unitrack', 'mask.py'))
_mask = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mask)
tensor_mask2box = _mask.tensor_mask2box            # unitrack/utils/mask.py:80-90 (the stand-in restates it)

KITTI_STEP_THINGS = [11, 13]                        # `kitti_step2cityscpaes`, :699


def segments_info(info, num_thing_classes):
    """info [K, 6] -> the reference's `segments_info` in segment-id order (knet/video/kernel_iter_head.py:880-899: things carry
    `category_id` = class and `score`; stuff `category_id` = 1-based stuff index)."""
    out = []
    for k in np.nonzero(info[:, 2] > 0)[0]:
        label, sid = int(info[k, 1]), int(info[k, 2])
        if label < num_thing_classes:
            out.append(dict(id=sid, isthing=True, category_id=label, instance_id=int(k), row=int(info[k, 0]),
                            score=float(info[k, 5:6].astype(np.int32).view(np.float32)[0])))
        else:
            out.append(dict(id=sid, isthing=False, category_id=label - num_thing_classes + 1))
    return sorted(out, key=lambda s: s['id'])


def things_for_tracking(seg, seg_infos):
    """`get_things_id_for_tracking`, :673-685 -> (segment ids, rows, labels, masks, scores) of the thing segments, in list order."""
    sids, rows, labels, masks, score = [], [], [], [], []
    for segment in seg_infos:
        if segment['isthing'] == True:  # noqa: E712  (as written)
            masks.append(seg == segment['id'])
            sids.append(segment['id'])
            rows.append(segment['row'])
            labels.append(segment['category_id'])
            score.append(segment['score'])
    return sids, rows, labels, masks, score


def semantic_thing(sem_logits, size, num_thing_classes, dtype=torch.float32):
    """:546-551 for one frame: sem_logits [Cs, hs, ws] -> (semantic_thing bool [Ho, Wo], top-two margin of the interpolated LOGITS
    [Ho, Wo] in `dtype`).  interpolate + sigmoid + argmax, as the reference writes it."""
    x = torch.as_tensor(sem_logits).to(dtype)[None]
    up = F.interpolate(x, tuple(size), mode='bilinear', align_corners=False)
    seg_out = up.sigmoid().argmax(1)[0]
    top2 = up[0].topk(2, dim=0).values
    return (seg_out < num_thing_classes).numpy(), (top2[0] - top2[1]).numpy()


def track_boxes(seg, info, num_thing_classes, thing=None):
    """:541-584 up to the tracker call: -> dict(det float32 [n, 5], labels int64 [n], rows int32 [n], segid int32 [n]) of the thing
    segments in segment order; `thing` = semantic_thing [Ho, Wo] (bool) or None for `semantic_filter=False` (:553)."""
    sids, rows, labels, masks, score = things_for_tracking(seg, segments_info(info, num_thing_classes))
    det = np.zeros((len(sids), 5), dtype=np.float32)
    if len(sids):
        m = torch.from_numpy(np.stack(masks)).float()
        m = m * (torch.from_numpy(np.asarray(thing)).float() if thing is not None else 1.)          # :567
        det[:, :4] = tensor_mask2box(m)                                                              # :583
        det[:, 4] = np.asarray(score, dtype=np.float32)                                              # :558
    return dict(det=det, labels=np.asarray(labels, dtype=np.int64), rows=np.asarray(rows, dtype=np.int32),
                segid=np.asarray(sids, dtype=np.int32))


def track_map(seg, info, num_thing_classes, ids):
    """:591-592 + `generate_track_id_maps` (:724-736): `ids` = what the tracker returned (any int sequence, possibly shorter than
    the number of thing segments, possibly empty)."""
    ids = np.asarray(ids, dtype=np.int64)
    final_id_maps = np.zeros(seg.shape)
    if len(ids) == 0:
        return final_id_maps.astype(np.int32)
    ids = ids + 1
    ids[ids == -1] = 0
    _, _, _, masks, _ = things_for_tracking(seg, segments_info(info, num_thing_classes))
    for i, id_ in enumerate(ids):
        if i >= len(masks):          # the reference would raise IndexError; the tracker never returns more rows than it was given
            break
        final_id_maps[masks[i]] = id_
    return final_id_maps.astype(np.int32)


def semantic_map(seg, info, num_thing_classes, num_stuff_classes, kitti_step):
    """`get_semantic_seg`, :698-722."""
    semantic_seg = np.zeros(seg.shape)
    for segment in segments_info(info, num_thing_classes):
        if segment['isthing'] == True:  # noqa: E712
            if kitti_step:
                cat_cur = KITTI_STEP_THINGS[segment['category_id']]
                semantic_seg[seg == segment['id']] = cat_cur
            else:
                semantic_seg[seg == segment['id']] = segment['category_id'] + num_stuff_classes
        else:
            if kitti_step:
                cat_cur = segment['category_id']
                cat_cur -= 1
                offset = 0
                for thing_id in KITTI_STEP_THINGS:
                    if cat_cur + offset >= thing_id:
                        offset += 1
                cat_cur += offset
                semantic_seg[seg == segment['id']] = cat_cur
            else:
                semantic_seg[seg == segment['id']] = segment['category_id'] - 1
    return semantic_seg.astype(np.int32)


# ---------------------------------------------------------------------------------------------------- shared inputs
def hand_frame(Ho, Wo, layout, num_thing_classes):
    """A hand-made frame: `layout` = [(joint label, (y0, y1, x0, x1), score)] in SEGMENT order (segment ids 1..); rectangles are
    half-open and later ones overwrite earlier ones.  -> (seg int32 [Ho, Wo], info int32 [K, 6]) with the info rows in REVERSE
    segment order plus one rejected entry, so that compaction by segment id is not the identity."""
    seg = np.zeros((Ho, Wo), dtype=np.int32)
    rows = []
    for i, (label, (y0, y1, x0, x1), score) in enumerate(layout):
        seg[y0:y1, x0:x1] = i + 1
        rows.append([10 + i, label, i + 1, 0, 0, int(np.float32(score).view(np.int32))])
    rows = rows[::-1] + [[99, 0, 0, 0, 0, int(np.float32(0.125).view(np.int32))]]
    info = np.asarray(rows, dtype=np.int32).reshape(-1, 6)
    for r in info:
        r[3] = r[4] = int((seg == r[2]).sum()) if r[2] > 0 else 0
    return seg, info


def dyadic_logits(Cs, hs, ws, seed, num_thing_classes):
    """Integer-valued semantic logits in [-8, 8]: with a power-of-two scale every bilinear weight and product is exact in fp32 (and
    the sum of four of them).  Three structured regions on top of the random cells:
      * the left third of the columns: thing channel 0 and the first stuff channel BOTH hold the cell's maximum — exact ties after
        the interpolation too, which the lowest channel (a thing) must win;
      * the top-right quarter: the last thing channel and the last stuff channel tie at the maximum in the same way;
      * the bottom-right quarter (rows >= hs // 2, columns >= ws // 2): one stuff channel at 8, everything else at -8 — a thing
        segment inside it is emptied by the filter."""
    rng = np.random.RandomState(seed)
    T = num_thing_classes
    x = rng.randint(-8, 9, size=(Cs, hs, ws)).astype(np.float32)
    top = x.max(0)
    w3 = ws // 3
    x[0, :, :w3] = top[:, :w3]
    x[T, :, :w3] = top[:, :w3]
    x[T - 1, :hs // 2, ws // 2:] = top[:hs // 2, ws // 2:]
    x[Cs - 1, :hs // 2, ws // 2:] = top[:hs // 2, ws // 2:]
    x[:, hs // 2:, ws // 2:] = -8.0
    x[T + 1, hs // 2:, ws // 2:] = 8.0
    return x


def float_logits(Cs, hs, ws, seed):
    rng = np.random.RandomState(seed)
    return (rng.randn(Cs, hs, ws) * 3.0).astype(np.float32)


CS, T_SEM = 5, 2                                      # channels of the semantic logits / thing classes of the filter cases
DYADIC_CASES = (((8, 16), (64, 128), 11), ((4, 9), (16, 36), 12))          # (hs, ws) -> (Ho, Wo), seed: power-of-two scales
NONDYADIC_CASES = (((5, 7), (37, 53), 21), ((6, 20), (48, 156), 22))
MARGIN, NEAR_TIE_CAP = 1e-4, 0.005                   # pixels decided by less than MARGIN (float64) are excluded; at most 0.5 % of the map
