#!/usr/bin/env python
"""A/B of the dense semantic loss of the kernel-initialisation head: `SegLossTail` (targets + loss + backward from the LOW-RES logits,
csrc/vkn_segloss.hip) against the torch composition `ConvKernelHead.forward_train` runs today (up-scale, paint, permuted copy, loss,
autograd backward), at the shapes of the shipped configs.  Needs the MI355X.

    python tools/seg_tail_ab.py [--rounds 40] [--iters 20] [--out profiles/seg_tail_ab.txt]

Both sides start from the same device inputs, in one process, and are timed ALTERNATELY: a round is `iters` steps of one side between
two device events, then the same of the other; reported are the median per step over the rounds and each side's spread (min .. max).
Next to the times stands the byte floor of the fused path: low read once + grad_low written once + the one-byte target map written
once and read twice + the painted layers read once, over the 6.3 TB/s the other floors of DESIGN.md §8 assume.  The two sides' losses and
gradients are compared at the timed sizes (a faster result that differs is not faster)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vkn_import  # noqa: E402

vkn = vkn_import.load()
DEV = torch.device('cuda:0')
RATE = 6.3e12
SHAPES = (   # name, loss, B, ncls, n_thing, h, w, S
    ('VIP-Seg video, CE, 124 cls, 90x160 low, S=4', 'ce', 2, 124, 58, 90, 160, 4),
    ('KITTI-STEP video, CE, 19 cls, 48x156 low, S=4', 'ce', 2, 19, 2, 48, 156, 4),
    ('Cityscapes image, focal, 19 cls, 128x256 low, S=2', 'focal', 2, 19, 8, 128, 256, 2),
)
NP, G, N_SEM = 100, 8, 10        # proposals, instances and present stuff classes per image


def inputs(B, ncls, n_thing, h, w, S, seed):
    rng = np.random.default_rng(seed)
    H, W = S * h, S * w
    low = torch.from_numpy(rng.standard_normal((B, ncls, h, w)).astype(np.float32) * 2).to(DEV)
    ys, xs = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    masks, labels, sem, cls, gt_inds, pos = [], [], [], [], [], []
    for _ in range(B):
        cy, cx = rng.uniform(0.1, 0.9, (G, 1, 1)) * H, rng.uniform(0.1, 0.9, (G, 1, 1)) * W
        ry, rx = rng.uniform(0.05, 0.25, (G, 1, 1)) * H, rng.uniform(0.05, 0.25, (G, 1, 1)) * W
        d = np.sqrt(((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2)
        masks.append(torch.from_numpy(np.clip((1.0 - d) * 4 + 0.5, 0, 1).astype(np.float32)).to(DEV))     # soft borders, as GtPrep's
        labels.append(torch.from_numpy(rng.integers(0, n_thing, G)).to(DEV))
        n = min(N_SEM, ncls - n_thing)
        bands = np.stack([((ys[0] >= j * H // n) & (ys[0] < (j + 1) * H // n)).astype(np.float32).repeat(W, axis=1) for j in range(n)])
        sem.append(torch.from_numpy(bands).to(DEV))
        cls.append(torch.from_numpy(np.sort(rng.choice(np.arange(n_thing, ncls), n, replace=False))).to(DEV))
        gi = np.zeros(NP, np.int64)
        rows = np.sort(rng.choice(NP, G, replace=False))
        gi[rows] = rng.permutation(G) + 1
        gt_inds.append(torch.from_numpy(gi).to(DEV))
        pos.append(torch.from_numpy(rows).to(DEV))           # known from shapes on the device-assignment path: no nonzero()
    return low, masks, labels, sem, cls, gt_inds, pos


def composed_step(loss_seg, ncls, S, low, masks, labels, sem, cls, gt_inds, pos):
    """today's branch of forward_train: up-scale; per image one masked arg-max over the stacked layers (`_image_targets`); the permuted
    copy and the loss (`ConvKernelHead.loss`); autograd backward to the low-res logits"""
    tgts = []
    for b in range(len(masks)):
        g = gt_inds[b][pos[b]] - 1
        stack = torch.cat([sem[b].bool(), masks[b][g].bool()])
        lab = torch.cat([cls[b].long(), labels[b][g].long()])
        order = torch.arange(stack.shape[0], device=DEV, dtype=torch.int32).view(-1, 1, 1)
        top = torch.where(stack, order, order.new_full((), -1)).amax(dim=0).long()
        tgts.append(torch.where(top >= 0, lab[top.clamp(min=0)], lab.new_full((), ncls)))
    loss = vkn.seg_tail.composed_loss(loss_seg, low, torch.stack(tgts, 0), ncls, S)
    return loss, torch.autograd.grad(loss, low)[0]


def fused_step(tail, low, masks, labels, sem, cls, gt_inds, pos):
    loss = tail.loss(low, tail.targets(masks, labels, sem, cls, gt_inds))
    return loss, torch.autograd.grad(loss, low)[0]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=40)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('seg_tail_ab.py measures on the MI355X: no GPU here, nothing measured')
    lines = [f'seg_tail_ab: {torch.cuda.get_device_name(0)}; per step = targets + loss + backward of B images; median of {args.rounds} '
             f'alternating rounds x {args.iters} steps (device events), spread = min .. max of the rounds; floor at {RATE / 1e12:.1f} TB/s',
             f'Np = {NP} proposals, G = {G} instances, up to {N_SEM} stuff layers per image']
    for name, kind, B, ncls, n_thing, h, w, S in SHAPES:
        loss_seg = (vkn.losses.FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0) if kind == 'focal'
                    else vkn.losses.CrossEntropyLoss(use_sigmoid=False, loss_weight=1.0))
        tail = vkn.SegLossTail(ncls, S, loss_seg)
        data = inputs(B, ncls, n_thing, h, w, S, seed=h * w)
        data[0].requires_grad_(True)
        A = lambda: fused_step(tail, *data)                          # noqa: E731
        C = lambda: composed_step(loss_seg, ncls, S, *data)          # noqa: E731
        (la, ga), (lc, gc) = A(), C()
        assert tail.fused
        torch.cuda.synchronize()
        dl = abs(float(la.detach()) - float(lc.detach())) / abs(float(lc.detach()))
        dg = float((ga - gc).abs().max()) / float(gc.abs().max())
        for _ in range(3):                                           # warm-up of both sides at this shape
            timed(A, args.iters), timed(C, args.iters)
        ta, tc = [], []
        for _ in range(args.rounds):
            ta.append(timed(A, args.iters))
            tc.append(timed(C, args.iters))
        n_layers = sum(int(s.shape[0]) for s in data[3]) + G * B
        H, W = S * h, S * w
        floor_bytes = 2 * B * ncls * h * w * 4 + 3 * B * H * W + n_layers * H * W * 4
        ma, mc = statistics.median(ta), statistics.median(tc)
        lines += [f'{name}, B = {B}',
                  f'  fused        {ma:9.1f} us  ({min(ta):.1f} .. {max(ta):.1f})',
                  f'  composition  {mc:9.1f} us  ({min(tc):.1f} .. {max(tc):.1f})    ratio composition / fused {mc / ma:.2f}',
                  f'  byte floor   {floor_bytes / RATE * 1e6:9.2f} us  ({floor_bytes / 1e6:.2f} MB; the up-scaled logits alone would be '
                  f'{B * ncls * H * W * 4 / 1e6:.1f} MB)    fused / floor {ma / (floor_bytes / RATE * 1e6):.0f}x',
                  f'  same result: loss differs by {dl:.1e} of its value, gradient by {dg:.1e} of its maximum']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
