"""`GtPrep` — the start of a training step on the device: `preprocess_gt_masks` and the `gt_match_indices` loop of `forward_train`
(knet/video/knet_quansi_dense_embed_fc_joint_train.py:152-223, :323-331; the image detector knet/det/knet.py has the same method).

    host masks (bytes) + semantic maps -> class presence + stuff labels     (vkn_gt_classes: a clear + 2 launches)
                                       -> ONE host read: the B stuff counts and class lists — they fix the tensor shapes downstream
                                       -> the fp32 bank [G_total, aH, aW] in `TailStep`'s row order (vkn_gt_bank_fill_f32: 1 launch)
    instance ids of the two frames     -> gt_match_indices + offsets        (vkn_gt_match_indices: 1 launch, no host read)

`F.interpolate(bilinear, align_corners=False)` to 1 / mask_assign_stride at an even integer stride is the mean of the 2 x 2 centre
pixels of every cell — exact for byte inputs, so the fused path and the torch composition below give the same bits.

Two deviations from the reference, on both paths: the input semantic map is NOT overwritten with the ignore label (the padding is a
predicate), and for an image without stuff `gt_sem_seg[b]` is an empty [0, aH, aW] view, not G_b rows of zeros (every consumer here
guards on `len(gt_sem_cls) > 0`)."""
import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, ops

DATASETS = ('generic', 'cityscapes', 'vipseg', 'kitti_step')


def label_of_class(dataset, num_thing_classes, num_stuff_classes, ignore_label=255, thing_label_in_seg=None):
    """The 256-entry table of the three `sem2ins_masks*` variants (knet/det/utils.py:8-93): the label of semantic class c, -1 = skip.
    generic: c + num_thing_classes - 1, skipping `thing_label_in_seg` (one label, default 0); cityscapes / vipseg: c + num_thing_classes,
    skipping the thing labels (default num_stuff_classes ... num_stuff_classes + num_thing_classes - 1); kitti_step:
    c - #{thing labels < c} + 2, skipping the thing labels (default 11, 13).  The ignore label is skipped in all of them."""
    if dataset not in DATASETS:
        raise ValueError(f'dataset must be one of {DATASETS}, got {dataset!r}')
    T, S = int(num_thing_classes), int(num_stuff_classes)
    if dataset == 'generic':
        things = (0 if thing_label_in_seg is None else int(thing_label_in_seg),)
        label = lambda c: c + T - 1                                          # noqa: E731
    elif dataset == 'kitti_step':
        things = (11, 13) if thing_label_in_seg is None else tuple(int(t) for t in thing_label_in_seg)
        label = lambda c: c - sum(1 for t in things if c > t) + 2            # noqa: E731  (the reference's label_shift=2)
    else:
        things = tuple(range(S, S + T)) if thing_label_in_seg is None else tuple(int(t) for t in thing_label_in_seg)
        label = lambda c: c + T                                              # noqa: E731
    table = [-1 if (c == ignore_label or c in things) else label(c) for c in range(256)]
    if any(v < -1 for v in table):
        raise ValueError('label_of_class: a listed class would get a negative label')
    return table


def _mask_bytes(gt_mask):
    """(array or tensor [G,H,W], is it a byte / bool one) of a `BitmapMasks` duck type (.masks, .height, .width) or a tensor"""
    m = gt_mask.masks if hasattr(gt_mask, 'masks') else gt_mask
    if isinstance(m, np.ndarray):
        if m.dtype == np.bool_:
            m = m.view(np.uint8)
        m = torch.from_numpy(np.ascontiguousarray(m))
    if not torch.is_tensor(m) or m.dim() != 3:
        raise TypeError('gt_masks entries must be [G,H,W] arrays / tensors or objects with .masks')
    return m, m.dtype in (torch.uint8, torch.bool)


class GtPrep:
    """`GtPrep(mask_assign_stride, num_thing_classes, num_stuff_classes, ignore_label=255, dataset='generic', thing_label_in_seg=None)`

    After `preprocess_gt_masks`: `bank` (the fp32 [G_total, aH, aW] every returned tensor is a view of), `n_sem`, `classes`,
    `thing_row0`, `sem_row0` (host lists; `classes`: per image the listed semantic classes, ascending), `status_word` (host int: VKN_STATUS_RANGE when an int64 map held a value outside [0, 255]; such pixels
    count as ignore) and `fused` (whether the device kernels ran).  After `match_indices`: `match`, `match_off`, `fused`."""

    def __init__(self, mask_assign_stride, num_thing_classes, num_stuff_classes, ignore_label=255, dataset='generic',
                 thing_label_in_seg=None):
        self.mask_assign_stride = int(mask_assign_stride)
        if self.mask_assign_stride != mask_assign_stride or self.mask_assign_stride < 1:
            raise ValueError('mask_assign_stride must be a positive integer')
        self.num_thing_classes, self.num_stuff_classes, self.ignore_label = int(num_thing_classes), int(num_stuff_classes), int(ignore_label)
        self.dataset = dataset
        self.label_of_class = label_of_class(dataset, num_thing_classes, num_stuff_classes, ignore_label, thing_label_in_seg)
        self.fused = None
        self.bank = self.match = self.match_off = None
        self.n_sem, self.classes, self.thing_row0, self.sem_row0, self.status_word = [], [], [], [], 0

    # ------------------------------------------------------------------------------------------------ preprocess_gt_masks
    def preprocess_gt_masks(self, img_metas, gt_masks, gt_labels, gt_semantic_seg):
        """img_metas: per image a dict with 'batch_input_shape' (the pad, read from the first) and 'img_shape'; gt_masks: per image a
        `BitmapMasks`-like object (.masks numpy uint8 [G,H,W], .height, .width) or a uint8 / bool tensor [G,H,W] on either side — host
        arrays are uploaded as BYTES; gt_labels: per image a tensor (its device is the target device); gt_semantic_seg [B,1,Hp,Wp]
        uint8 / int64, or None.  -> (gt_masks_tensor, gt_sem_cls, gt_sem_seg) as the reference: per image fp32 [G_b,aH,aW], int64
        [n_sem_b], fp32 [n_sem_b,aH,aW]; (masks, None, None) without a semantic map.
        The fused path makes ONE host read — the B stuff counts and class lists, a few hundred bytes: the one synchronisation of
        the call.  Outside the kernels' envelope (odd stride, sizes the stride does not divide, non-byte masks, CPU tensors) the
        torch composition runs instead, with the same values, and `fused` is False."""
        B = len(gt_masks)
        Hp, Wp = (int(v) for v in img_metas[0]['batch_input_shape'])
        s = self.mask_assign_stride
        valid = [(min(int(m['img_shape'][0]), Hp), min(int(m['img_shape'][1]), Wp)) for m in img_metas]
        masks, bytes_ok = zip(*(_mask_bytes(g) for g in gt_masks)) if B else ((), ())
        sem = gt_semantic_seg
        device = next((t.device for t in list(gt_labels or []) if torch.is_tensor(t)), None)
        if device is None:
            device = sem.device if torch.is_tensor(sem) else (masks[0].device if B else torch.device('cpu'))
        self.fused = (device.type == 'cuda' and all(bytes_ok) and ops.gt_prep_supported(B, Hp, Wp, s)
                      and all(m.shape[1] <= Hp and m.shape[2] <= Wp for m in masks)
                      and (sem is None or (torch.is_tensor(sem) and sem.dtype in (torch.uint8, torch.int64)
                                           and tuple(sem.shape) == (B, 1, Hp, Wp))))
        if not self.fused:
            return self._compose(device, masks, sem, valid, Hp, Wp)
        masks = [m.to(device) for m in masks]                                   # bytes (1 per pixel and instance), never fp32
        self.status_word = 0
        if sem is not None:
            sem3 = sem.to(device).reshape(B, Hp, Wp)
            _, classes, labels, _, raw = ops.gt_classes(sem3, valid, self.label_of_class)
            host = raw.cpu().numpy()                                            # THE host read of the call: status, counts, class lists
            self.status_word = int(host[:4].view(np.int32)[0])
            self.n_sem = [int(v) for v in host[4:4 + 4 * B].view(np.int32)]
            self.classes = [host[4 + 36 * B + 256 * b:][:n].tolist() for b, n in enumerate(self.n_sem)]
        else:
            sem3, classes, labels, self.n_sem, self.classes = None, None, None, [0] * B, [[] for _ in range(B)]
        rows = sum(int(m.shape[0]) for m in masks) + sum(self.n_sem)
        if rows * (Hp // s) * (Wp // s) * 4 >= 2 ** 31 or rows > 65535 - B:          # beyond vkn_gt_bank_fill_f32
            self.fused = False
            return self._compose(device, masks, sem, valid, Hp, Wp)
        self.bank, self.thing_row0, self.sem_row0 = ops.gt_bank_fill(masks, sem3, valid, self.n_sem, classes, s, (Hp, Wp), device=device)
        G = [int(m.shape[0]) for m in masks]
        out_masks = [self.bank[r:r + g] for r, g in zip(self.thing_row0, G)]
        if sem is None:
            return out_masks, None, None
        sem_seg = [self.bank[r:r + n] for r, n in zip(self.sem_row0, self.n_sem)]
        sem_cls = [labels[b, :n] for b, n in enumerate(self.n_sem)]
        return out_masks, sem_cls, sem_seg

    def _sem2ins(self, seg):
        """`sem2ins_masks*` through the table: seg [1,Hp,Wp] (ignore already filled in) -> (labels int64 [n], masks fp32 [n,Hp,Wp],
        the listed classes ascending, whether a value lay outside [0, 255]) — one `torch.unique` and its host read, as the reference"""
        values = [int(c) for c in torch.unique(seg).tolist()]
        listed = [c for c in values if 0 <= c <= 255 and self.label_of_class[c] >= 0]
        bad = any(c < 0 or c > 255 for c in values)
        if not listed:
            return seg.new_zeros((0,), dtype=torch.int64), seg.new_zeros((0,) + tuple(seg.shape[-2:]), dtype=torch.float32), listed, bad
        labels = torch.tensor([self.label_of_class[c] for c in listed], dtype=torch.int64, device=seg.device)
        return labels, torch.cat([seg == c for c in listed]).float(), listed, bad

    def _compose(self, device, masks, sem, valid, Hp, Wp):
        """The reference's op sequence in torch (pad, `sem2ins_masks*`, bilinear `F.interpolate`), on `device`."""
        s = self.mask_assign_stride
        aH, aW = Hp // s, Wp // s
        out_masks, sem_cls, sem_seg = [], [], []
        self.n_sem, self.classes, self.status_word = [], [], 0
        for i, m in enumerate(masks):
            t = m.to(device).to(torch.float32)
            if t.shape[2] != Wp or t.shape[1] != Hp:
                t = F.pad(t, (0, Wp - t.shape[2], 0, Hp - t.shape[1]), value=0)
            if sem is not None:
                seg = sem[i].to(device).clone()                                 # the reference fills the caller's tensor; this one does not
                seg[:, valid[i][0]:, :] = self.ignore_label
                seg[:, :, valid[i][1]:] = self.ignore_label
                labels, ins, listed, bad = self._sem2ins(seg)
                if bad:
                    self.status_word |= _lib.CONSTS['VKN_STATUS_RANGE']
                self.n_sem.append(len(listed))
                self.classes.append(listed)
                sem_seg.append(F.interpolate(ins[None], (aH, aW), mode='bilinear', align_corners=False)[0] if ins.shape[0]
                               else t.new_zeros((0, aH, aW)))
                sem_cls.append(labels)
            else:
                self.n_sem.append(0)
                self.classes.append([])
            out_masks.append(F.interpolate(t[None], (aH, aW), mode='bilinear', align_corners=False)[0] if t.shape[0]
                             else t.new_zeros((0, aH, aW)))
        self.bank, self.thing_row0, self.sem_row0 = None, [], []
        return (out_masks, sem_cls, sem_seg) if sem is not None else (out_masks, None, None)

    # ------------------------------------------------------------------------------------------------------ gt_match_indices
    def match_indices(self, gt_instance_ids, ref_gt_instance_ids):
        """Per image the int64 partner index of every key-frame instance in the reference frame: the FIRST position of its id among
        the image's reference ids, else -1 (:323-331).  -> a list of per-image tensors, views of `self.match` (with `self.match_off`,
        int64 [B+1]: the pair `vkn_track_loss_fwd_f32` takes).  CUDA inputs: one launch, nothing is copied to the host."""
        keys = [k.reshape(-1).to(torch.int64) for k in gt_instance_ids]
        refs = [r.reshape(-1).to(torch.int64) for r in ref_gt_instance_ids]
        B, lens = len(keys), [int(k.numel()) for k in keys]
        if B == 0 or B != len(refs):
            raise ValueError('match_indices: one key and one reference id tensor per image')
        self.fused = (all(t.is_cuda for t in keys + refs) and B <= ops.GT_MAX_IMAGES
                      and max(lens + [int(r.numel()) for r in refs]) <= ops.GT_MAX_IDS)
        if self.fused:
            self.match, self.match_off = ops.gt_match_indices(keys, refs)
        else:
            parts = []
            for k, r in zip(keys, refs):
                r = r.to(k.device)
                if r.numel() == 0 or k.numel() == 0:
                    parts.append(torch.full_like(k, -1))
                    continue
                eq = k[:, None] == r[None, :]
                parts.append(torch.where(eq.any(1), eq.to(torch.uint8).argmax(1), torch.full_like(k, -1)))
            self.match = torch.cat(parts)
            self.match_off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int64, device=self.match.device)
        starts = [0] + list(np.cumsum(lens))
        return [self.match[int(a):int(a) + n] for a, n in zip(starts, lens)]
