#!/usr/bin/env python
"""Generate tests/golden/seg_tail_*.npz from the REFERENCE ITSELF (needs the reference checkout; CPU only; never imported by a test).

    VKN_REFERENCE=<reference checkout> python tools/gen_golden_seg_tail.py

The reference's files are loaded UNMODIFIED through the plumbing stand-ins of oracle/standins, by oracle/gen_golden.py's own import
lines; its helpers (`init_inputs`, `AttrDict`, the pass-through neck) are used as they are.  Per case the unmodified
`ConvKernelHead.forward_train` (knet/det/kernel_head.py:267-336) runs behind the pass-through neck as `run_rpn_train_case` runs it, on
hash-formula inputs (oracle/synth.py seeds: the tests regenerate the ground truth), and the fixture holds OUTPUTS only:

  seg_tail_<case>.npz   case = (focal?, S, B, ncls, n_thing, h, w, C, nprop, seed), loss_weight;
                        seg_preds fp32 [B, ncls, h, w]: the head's LOW-RES semantic logits;
                        seg_targets uint8 [B, S h, S w]: what `get_targets` returned (values <= ncls <= 255);
                        assigned int64 [B, nprop]: the assigner's gt_inds;  loss: `loss_rpn_seg` (fp32, and as float64 of that);
                        grad fp32 [B, ncls, h, w]: d loss_rpn_seg / d seg_preds from a backward of that loss alone.
  seg_tail_paint.npz    hand-made layer stacks through `_get_target_single` alone: inputs (masks, labels, pos_inds) and its seg_targets.
No up-scaled tensor is stored.  The same seeds give the same bytes: `np.savez_compressed` of arrays in a fixed order.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if not os.environ.get('VKN_REFERENCE'):
    raise SystemExit('set VKN_REFERENCE to the reference checkout')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import gen_golden as gg  # noqa: E402  (imports the reference's modules through the stand-ins)
from oracle import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')

# (loss, S, B, ncls, n_thing, h, w): the smallest shapes at which the kernels can still go wrong
CASES = {
    'focal_tiny': dict(focal=1, S=2, B=2, ncls=5, n_thing=2, h=8, w=16, C=64, nprop=12, seed=91),        # rpn_train_tiny's
    'focal_cfg': dict(focal=1, S=2, B=2, ncls=19, n_thing=2, h=16, w=32, C=256, nprop=100, seed=92),     # rpn_train_cfg's
    'ce_kitti': dict(focal=0, S=4, B=1, ncls=19, n_thing=2, h=12, w=39, C=64, nprop=12, seed=93),        # a quarter of 48 x 156; odd width
    'ce_vipseg': dict(focal=0, S=4, B=1, ncls=124, n_thing=58, h=6, w=10, C=64, nprop=12, seed=94),      # VIP-Seg's class count
    'ce_s2': dict(focal=0, S=2, B=2, ncls=5, n_thing=2, h=3, w=5, C=64, nprop=12, seed=95),
    'focal_s1': dict(focal=1, S=1, B=3, ncls=33, n_thing=8, h=5, w=7, C=64, nprop=12, seed=96),
    'ce_s1': dict(focal=0, S=1, B=1, ncls=2, n_thing=1, h=2, w=3, C=64, nprop=12, seed=97),
}
CASE_FIELDS = ('focal', 'S', 'B', 'ncls', 'n_thing', 'h', 'w', 'C', 'nprop', 'seed')


def build_head(p):
    loss_seg = (dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0) if p['focal']
                else dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
    cfg = dict(type='ConvKernelHead', num_proposals=p['nprop'], in_channels=p['C'], out_channels=p['C'], num_loc_convs=0,
               num_seg_convs=0, localization_fpn=dict(type='PassThroughNeck'), conv_kernel_size=1, semantic_fpn=True,
               num_classes=p['ncls'], use_binary=True, proposal_feats_with_obj=True, feat_downsample_stride=p['S'], feat_refine=False,
               num_thing_classes=p['n_thing'], num_stuff_classes=p['ncls'] - p['n_thing'], cat_stuff_mask=True,
               loss_rank=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.1), loss_seg=loss_seg,
               loss_mask=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
               loss_dice=dict(type='DiceLoss', loss_weight=4.0),
               train_cfg=gg.AttrDict(assigner=dict(type='MaskHungarianAssigner', cls_cost=dict(type='FocalLossCost', weight=2.0),
                                                   dice_cost=dict(type='DiceCost', weight=4.0, pred_act=True),
                                                   mask_cost=dict(type='MaskCost', weight=1.0, pred_act=True)),
                                     sampler=dict(type='MaskPseudoSampler'), pos_weight=1))
    head = gg.build_head(cfg)
    head.train()
    return head


def run_case(name, p):
    head = build_head(p)
    q = dict(C=p['C'], nprop=p['nprop'], ncls=p['ncls'], n_thing=p['n_thing'], H=p['h'], W=p['w'], B=p['B'], seed=p['seed'], sem=True)
    loc, sem, shapes = gg.init_inputs(q)
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == shapes
    head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_like(shapes, p['seed']).items()}, strict=True)
    loc, sem = torch.from_numpy(loc).requires_grad_(True), torch.from_numpy(sem).requires_grad_(True)
    tg = synth.train_targets(p['B'], p['n_thing'], p['ncls'] - p['n_thing'], p['S'] * p['h'], p['S'] * p['w'], p['seed'])
    gt_masks = [torch.from_numpy(t['gt_masks']) for t in tg]
    gt_labels = [torch.from_numpy(t['gt_labels']) for t in tg]
    gt_sem_seg = [torch.from_numpy(t['gt_sem_seg']) for t in tg]
    gt_sem_cls = [torch.from_numpy(t['gt_sem_cls']) for t in tg]
    seen = {}
    assign, decode, targets = head.assigner.assign, head._decode_init_proposals, head.get_targets

    def rec_assign(*a, **k):
        r = assign(*a, **k)
        seen.setdefault('assigned', []).append(r.gt_inds.clone())
        return r

    def rec_decode(*a, **k):
        out = decode(*a, **k)
        out[4].retain_grad()
        seen['seg_preds'] = out[4]
        return out

    def rec_targets(*a, **k):
        out = targets(*a, **k)
        seen['seg_targets'] = out[4].clone()
        return out
    head.assigner.assign, head._decode_init_proposals, head.get_targets = rec_assign, rec_decode, rec_targets
    losses = head.forward_train((loc, sem), [dict() for _ in range(p['B'])], gt_masks, gt_labels, gt_sem_seg=gt_sem_seg,
                                gt_sem_cls=gt_sem_cls)[0]
    loss = losses['loss_rpn_seg']
    loss.backward()                                            # of that loss alone
    seg_preds, tgt = seen['seg_preds'], seen['seg_targets']
    assert tuple(seg_preds.shape) == (p['B'], p['ncls'], p['h'], p['w']) and tuple(tgt.shape) == (p['B'], p['S'] * p['h'], p['S'] * p['w'])
    assert int(tgt.min()) >= 0 and int(tgt.max()) <= p['ncls'] <= 255
    out = dict(case=np.array([p[k] for k in CASE_FIELDS], dtype=np.int64), loss_weight=np.float64(head.loss_seg.loss_weight),
               seg_preds=seg_preds.detach().numpy(), seg_targets=tgt.numpy().astype(np.uint8),
               assigned=torch.stack(seen['assigned']).numpy(), loss=loss.detach().numpy().astype(np.float32),
               loss_f64=np.float64(float(loss.detach())), grad=seg_preds.grad.numpy())
    np.savez_compressed(os.path.join(GOLDEN, f'seg_tail_{name}.npz'), **out)
    print(f'{name}: loss_rpn_seg={float(loss.detach()):.6f}  positives={int((tgt < p["ncls"]).sum())}/{tgt.numel()}  '
          f'max|grad|={float(seg_preds.grad.abs().max()):.3e}')


def paint_cases():
    """Hand-made layer stacks (H x W = 6 x 9, ncls = 7): name -> (gt_masks [G,H,W], gt_labels [G], gt_inds [Np], sem [n,H,W] | None,
    sem_cls [n] | None)."""
    H, W = 6, 9
    z = lambda n: np.zeros((n, H, W), np.float32)                     # noqa: E731
    out = {}
    # an instance covers stuff, a later instance covers an earlier one; proposal order, not ground-truth order, decides
    m, s = z(3), z(2)
    s[0, :3], s[1, 3:] = 1, 1
    m[0, 1:4, 1:5], m[1, 2:5, 3:8], m[2, 0:2, 0:2] = 1, 1, 1
    out['overlap'] = (m, [0, 1, 1], [0, 2, 0, 1, 0, 3, 0, 0], s, [5, 6])
    # soft values: 0.25 covers as 1 does
    m, s = z(2), z(1)
    s[0, :, :4] = 0.25
    m[0, 2:4, 2:6], m[1, 3:6, 5:9] = 0.25, 0.5
    out['soft'] = (m, [1, 0], [1, 0, 0, 2], s, [4])
    # an image without stuff (empty lists), one without a positive, one with neither, and gt_sem_seg = None
    m = z(2)
    m[0, :2], m[1, 1:3, 4:] = 1, 1
    out['no_stuff'] = (m, [0, 1], [2, 1, 0], z(0), [])
    s = z(2)
    s[0, :, :5], s[1, 2:, 3:] = 1, 1
    out['no_pos'] = (m, [0, 1], [0, 0, 0], s, [2, 3])
    out['neither'] = (m, [0, 1], [0, 0, 0], z(0), [])
    out['sem_none'] = (m, [1, 0], [0, 2, 1], None, None)
    # a single covered pixel at position 0 and at the last position
    m = z(2)
    m[0, 0, 0], m[1, H - 1, W - 1] = 1, 1
    out['corners'] = (m, [0, 1], [1, 2], z(0), [])
    return out


def run_paint():
    head = build_head(dict(focal=1, S=1, B=1, ncls=7, n_thing=2, h=6, w=9, C=64, nprop=8, seed=1))
    cfg = gg.AttrDict(pos_weight=1)
    out = dict(names=np.array(sorted(paint_cases())), ncls=np.int64(7))
    for name, (masks, labels, gt_inds, sem, sem_cls) in paint_cases().items():
        masks, labels, gt_inds = torch.from_numpy(masks), torch.tensor(labels, dtype=torch.int64), torch.tensor(gt_inds, dtype=torch.int64)
        pos = torch.nonzero(gt_inds > 0, as_tuple=False).squeeze(-1)
        neg = torch.nonzero(gt_inds == 0, as_tuple=False).squeeze(-1)
        g = gt_inds[pos] - 1
        preds = torch.zeros((gt_inds.numel(),) + tuple(masks.shape[1:]))
        sem_t = None if sem is None else torch.from_numpy(sem)
        cls_t = None if sem_cls is None else torch.tensor(sem_cls, dtype=torch.int64)
        res = head._get_target_single(pos, neg, preds[pos], preds[neg], masks[g], labels[g], sem_t, cls_t, cfg)
        out[f'{name}_masks'], out[f'{name}_labels'], out[f'{name}_gt_inds'] = masks.numpy(), labels.numpy(), gt_inds.numpy()
        if sem is not None:
            out[f'{name}_sem'], out[f'{name}_sem_cls'] = sem, np.asarray(sem_cls, dtype=np.int64)
        out[f'{name}_seg_targets'] = res[4].numpy().astype(np.uint8)
        print('paint', name, np.bincount(res[4].numpy().ravel(), minlength=8).tolist())
    np.savez_compressed(os.path.join(GOLDEN, 'seg_tail_paint.npz'), **out)


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    torch.manual_seed(0)
    for name, p in CASES.items():
        run_case(name, p)
    run_paint()


if __name__ == '__main__':
    main()
