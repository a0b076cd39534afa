"""`TrackTail` — what the video detector's `simple_test` does AFTER the head, on the device
(knet/video/knet_quansi_dense_embed_fc_joint_train.py:536-603): thing boxes under the semantic filter, the tracking embeddings of the
kept kernels, the quasi-dense association, and the two maps the detector returns.

    panoptic_joint -> [track_boxes -> gather rows -> track_head -> tracker (device count) -> track_maps]

Every step reads the previous one's device tensors; nothing is copied to the host and nothing is synchronised.  The class owns no
parameters: the embedding layers (`embed_fcs` / `fc_embed`), the track head and the tracker are the caller's.  The host form of the
first step, `KernelIterHead.things_for_tracking`, stays for callers that hold NumPy copies.
"""
import torch

from . import _lib, ops

KITTI_STEP_THINGS = (11, 13)      # `kitti_step2cityscpaes` (:699): the two KITTI-STEP thing classes in Cityscapes train ids


def sem_of_label(num_thing_classes, num_stuff_classes, kitti_step):
    """The semantic class of every JOINT label (< num_thing_classes: thing class; else num_thing_classes + stuff index), as
    `get_semantic_seg` assigns it (:698-722) to a segment whose `category_id` is the thing class / the 1-based stuff index
    (`KernelIterHead._segments_info`).  -> list of num_thing_classes + num_stuff_classes ints."""
    T, S = int(num_thing_classes), int(num_stuff_classes)
    if kitti_step and T > len(KITTI_STEP_THINGS):
        raise ValueError(f'kitti_step maps {len(KITTI_STEP_THINGS)} thing classes, not {T}')
    table = []
    for label in range(T + S):
        if label < T:
            table.append(KITTI_STEP_THINGS[label] if kitti_step else label + S)         # :704-708
        elif kitti_step:                                                                 # :711-719
            cat = label - T                                                              # category_id - 1
            offset = 0
            for thing_id in KITTI_STEP_THINGS:
                if cat + offset >= thing_id:
                    offset += 1
            table.append(cat + offset)
        else:
            table.append(label - T)                                                      # :721
    return table


class TrackTail:
    """Built from `(num_thing_classes, num_stuff_classes, semantic_filter, kitti_step, tracker, track_head)`: the detector's own
    attributes.  `tracker` is a `QuasiDenseEmbedTracker`, `track_head` a callable [n, C] -> [n, E] (`QuasiDenseMaskEmbedHeadGTMask`)."""

    def __init__(self, num_thing_classes, num_stuff_classes, semantic_filter=True, kitti_step=False, tracker=None, track_head=None):
        if tracker is None or track_head is None:
            raise ValueError('TrackTail needs the detector\'s tracker and track_head')
        self.num_thing_classes, self.num_stuff_classes = int(num_thing_classes), int(num_stuff_classes)
        self.semantic_filter, self.kitti_step = bool(semantic_filter), bool(kitti_step)
        self.tracker, self.track_head = tracker, track_head
        self.sem_of_label = sem_of_label(num_thing_classes, num_stuff_classes, kitti_step)
        self._tables = {}          # device -> the table as an int32 tensor (uploaded once per device)
        self.last = None           # the intermediates of the last call (device tensors): count, n_ids, labels, rows, segid

    def reset(self):
        """A new video (`init_tracker`, :505-506)."""
        self.tracker.reset()

    def _table(self, device):
        t = self._tables.get(device)
        if t is None:
            t = self._tables[device] = torch.tensor(self.sem_of_label, dtype=torch.int32).to(device)
        return t

    @torch.no_grad()
    def __call__(self, panoptic_seg, info, nseg, seg_preds, obj_feats, frame_id, embed=None):
        """panoptic_seg int32 [B,Ho,Wo], info int32 [B,K,6], nseg int32 [B]: `ops.panoptic_joint`'s outputs for B CONSECUTIVE frames of
        one video; seg_preds fp32 [B,Cs,hs,ws]: the kernel-init head's semantic logits (read with `semantic_filter`); obj_feats
        [B,N,C(,1,1)]: the head's object features, already embedded — or raw with `embed`, a callable for the detector's
        `embed_fcs` + `fc_embed` (:574-579); frame_id: the id of the first frame (frame b is frame_id + b).
        -> (semantic_map int32 [B,Ho,Wo], track_map int32 [B,Ho,Wo], det fp32 [B,K,5], ids int64 [B,max_dets]), device tensors:
        `det` rows are (xmin, ymin, xmax, ymax, score) of the thing segments in segment order (zero beyond `last['count']`), `ids`
        the tracker's ids of its returned rows (-2 beyond `last['n_ids']`).  A frame without things is not a tracker call (:569-573,
        :597-598): its track map is zero and the tracker state stays as it is."""
        if not (torch.is_tensor(panoptic_seg) and panoptic_seg.is_cuda and torch.is_tensor(obj_feats) and obj_feats.is_cuda):
            raise _lib.VknLibraryError('TrackTail: expected CUDA/HIP tensors — the MI355X path has no CPU fallback')
        if self.semantic_filter and seg_preds is None:
            raise ValueError('semantic_filter=True needs seg_preds')
        det, labels, rows, segid, count = ops.track_boxes(panoptic_seg, info, nseg, self.num_thing_classes,
                                                          sem_logits=seg_preds if self.semantic_filter else None)
        B, K = int(det.shape[0]), int(det.shape[1])
        feats = obj_feats.reshape(obj_feats.shape[0], obj_feats.shape[1], -1)
        if feats.shape[0] != B:
            raise ValueError('obj_feats [B,N,C] and panoptic_seg [B,Ho,Wo] disagree')
        if embed is not None:
            feats = embed(feats)
        D = self.tracker.max_dets
        n_max = min(K, D)          # rows handed to the tracker; it reads the first min(count, n_max) of them
        ids, n_ids = [], []
        for b in range(B):
            kept = feats[b].index_select(0, rows[b, :n_max].long())          # rows beyond count gather kernel 0 and are never read
            track_feats = self.track_head(kept)
            _, _, ids_b, cnt_b = self.tracker.match_padded(det[b, :n_max], labels[b, :n_max], track_feats, int(frame_id) + b,
                                                           count=count[b:b + 1])
            ids.append(ids_b)
            n_ids.append(cnt_b[:1])
        ids, n_ids = torch.stack(ids), torch.cat(n_ids)
        track_map, semantic_map = ops.track_maps(panoptic_seg, segid, count, ids, n_ids, info, self._table(det.device))
        ids = torch.where(torch.arange(D, device=ids.device)[None] < n_ids[:, None], ids, torch.full_like(ids, -2))
        self.last = dict(count=count, n_ids=n_ids, labels=labels, rows=rows, segid=segid)
        return semantic_map, track_map, det, ids
