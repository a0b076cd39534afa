"""Float64 reference of the dense semantic loss of the kernel-initialisation head, and the fixtures' inputs (test infrastructure).

`paint` is the painting rule of include/vkn_seg_loss.h as a plain loop; `loss64` is `F.interpolate` + the loss in float64 with autograd
for the gradient; `compose32` is the fp32 torch composition the fused path replaces (knet/det/kernel_head.py:278-292, 404-426) — the
yardstick of the GPU tests.  References are computed once per (case, scale) and shared."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = ('focal_tiny', 'focal_cfg', 'ce_kitti', 'ce_vipseg', 'ce_s2', 'focal_s1', 'ce_s1')
CASE_FIELDS = ('focal', 'S', 'B', 'ncls', 'n_thing', 'h', 'w', 'C', 'nprop', 'seed')
PAINT = ('overlap', 'soft', 'no_stuff', 'no_pos', 'neither', 'sem_none', 'corners')
ALPHA, GAMMA = 0.25, 2.0          # the shipped focal loss (configs/det/_base_/models/knet_*: loss_seg)
# seeded shapes of the issue: (B, ncls, h, w, S)
EXTRA_SHAPES = ((1, 1, 1, 1, 1), (1, 255, 3, 5, 2), (1, 2, 2, 3, 4))


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(golden dict, case dict, ground truth of the case regenerated from the seeds: per image gt_masks, gt_labels, gt_sem_seg, gt_sem_cls)"""
    g = dict(np.load(os.path.join(GOLDEN, f'seg_tail_{name}.npz'), allow_pickle=False))
    p = dict(zip(CASE_FIELDS, (int(v) for v in g['case'])))
    tg = synth.train_targets(p['B'], p['n_thing'], p['ncls'] - p['n_thing'], p['S'] * p['h'], p['S'] * p['w'], p['seed'])
    return g, p, tg


@functools.lru_cache(maxsize=None)
def paint_fixture():
    g = dict(np.load(os.path.join(GOLDEN, 'seg_tail_paint.npz'), allow_pickle=False))
    assert tuple(sorted(PAINT)) == tuple(str(n) for n in g['names'])
    out = {}
    for n in PAINT:
        out[n] = dict(masks=g[f'{n}_masks'], labels=g[f'{n}_labels'], gt_inds=g[f'{n}_gt_inds'], sem=g.get(f'{n}_sem'),
                      sem_cls=g.get(f'{n}_sem_cls'), seg_targets=g[f'{n}_seg_targets'])
    return int(g['ncls']), out


def paint(ncls, shape, sem, sem_cls, masks, labels, gt_inds):
    """the rule, layer by layer: uint8 [H, W] (int64 where ncls itself does not fit a byte)"""
    t = np.full(shape, ncls, dtype=np.int64)
    if sem is not None and sem_cls is not None:
        for j in range(len(sem_cls)):
            t[sem[j] != 0] = int(sem_cls[j])
    for n in range(len(gt_inds)):
        if gt_inds[n] > 0:
            g = int(gt_inds[n]) - 1
            t[masks[g] != 0] = int(labels[g])
    return t.astype(np.uint8) if ncls <= 255 else t


def paint_case(name):
    """the fixture's map by the loop: uint8 [B, H, W]"""
    g, p, tg = fixture(name)
    shape = (p['S'] * p['h'], p['S'] * p['w'])
    return np.stack([paint(p['ncls'], shape, tg[b]['gt_sem_seg'], tg[b]['gt_sem_cls'], tg[b]['gt_masks'], tg[b]['gt_labels'],
                           g['assigned'][b]) for b in range(p['B'])])


def _loss(low, tgt, S, focal, ncls, alpha, gamma, loss_weight):
    """the composition in the dtype of `low` (torch ops only): up-scale, permute, loss"""
    seg = F.interpolate(low, scale_factor=S, mode='bilinear', align_corners=False) if S > 1 else low
    flat = seg.reshape(seg.shape[0], ncls, -1).permute(0, 2, 1).reshape(-1, ncls)
    t = tgt.reshape(-1).long()
    if focal:
        onehot = F.one_hot(t, num_classes=ncls + 1)[:, :ncls].to(flat.dtype)
        p = flat.sigmoid()
        pt = (1 - p) * onehot + p * (1 - onehot)
        fw = (alpha * onehot + (1 - alpha) * (1 - onehot)) * pt.pow(gamma)
        el = F.binary_cross_entropy_with_logits(flat, onehot, reduction='none') * fw
        return loss_weight * el.sum() / (t < ncls).sum().to(flat.dtype).clamp(min=1.0)
    return loss_weight * F.cross_entropy(flat, t, reduction='none', ignore_index=ncls).mean()


def _run(low, tgt, S, focal, ncls, alpha, gamma, loss_weight, g):
    low = low.detach().clone().requires_grad_(True)
    loss = _loss(low, tgt, S, focal, ncls, alpha, gamma, loss_weight)
    (loss * g).backward()
    return loss.detach(), low.grad.detach()


def loss64(low, tgt, S, focal, ncls, alpha=ALPHA, gamma=GAMMA, loss_weight=1.0, g=1.0):
    """(loss, g x d loss / d low) in float64 on the CPU; low fp32 / tgt uint8 numpy or tensors"""
    low = torch.as_tensor(np.asarray(low)).double()
    return _run(low, torch.as_tensor(np.asarray(tgt)), S, focal, ncls, alpha, gamma, loss_weight, g)


def compose32(low, tgt, S, focal, ncls, alpha=ALPHA, gamma=GAMMA, loss_weight=1.0, g=1.0):
    """the same composition in fp32 on the device of `low` (a tensor)"""
    return _run(low.float(), tgt, S, focal, ncls, alpha, gamma, loss_weight, g)


@functools.lru_cache(maxsize=None)
def fixture_ref(name, scale=1, g=1.0):
    """float64 (loss, grad) of a fixture's seg_preds x scale against its seg_targets"""
    gd, p, _ = fixture(name)
    return loss64(gd['seg_preds'] * np.float32(scale), gd['seg_targets'], p['S'], p['focal'], p['ncls'], loss_weight=float(gd['loss_weight']), g=g)


@functools.lru_cache(maxsize=None)
def extra_case(i, focal, scale):
    """seeded logits and targets of EXTRA_SHAPES[i] (every class and the ignore value occur where there is room) + their float64
    (loss, grad)"""
    B, ncls, h, w, S = EXTRA_SHAPES[i]
    low = synth.normalish((B, ncls, h, w), 4100 + i, 1.0) * np.float32(scale)
    u = synth.uniform((B, S * h, S * w), 4200 + i, 0.0, 1.0).astype(np.float64)
    tgt = np.minimum((u * (ncls + 1)).astype(np.int64), ncls).astype(np.uint8)
    return low, tgt, loss64(low, tgt, S, focal, ncls)
