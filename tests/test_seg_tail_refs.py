"""CPU: the float64 reference of the dense semantic loss (tests/seg_tail_ref.py) against the fixtures taken from the reference's own
`ConvKernelHead.forward_train` (tools/gen_golden_seg_tail.py), and the painting rule against the head's masked arg-max."""
import numpy as np
import pytest
import torch

import seg_tail_ref as R

# fp32 rounding of the reference's own evaluation: its loss is a sum of N <= 1.4e5 fp32 terms, each a few ulp off, added by torch's
# pairwise reduction (error ~ log2(N) ulp at most): 32 ulp of the loss.  A gradient element is a sum of at most (2 S)^2 = 64 products
# of fp32 element derivatives (each a few ulp of the LARGEST derivative off, soft-max normalisation included): 64 ulp of the maximum.
LOSS_RTOL = 32 * 2.0 ** -24
GRAD_RTOL = 64 * 2.0 ** -24


@pytest.mark.parametrize('name', R.FIXTURES)
def test_float64_reference_meets_the_fixture(name):
    g, p, tg = R.fixture(name)
    assert g['seg_targets'].dtype == np.uint8 and g['seg_preds'].dtype == np.float32 and g['seg_preds'].shape == (p['B'], p['ncls'], p['h'], p['w'])
    assert np.array_equal(R.paint_case(name), g['seg_targets'])
    loss, grad = R.fixture_ref(name)
    assert float(g['loss']) == float(g['loss_f64'])
    err = abs(float(loss) - float(g['loss_f64']))
    gerr = float((grad - torch.from_numpy(g['grad']).double()).abs().max())
    gmax = float(grad.abs().max())
    print(f'{name}: loss rel err {err / abs(float(loss)):.2e} (bound {LOSS_RTOL:.2e}); grad err / max {gerr / gmax:.2e} (bound {GRAD_RTOL:.2e})')
    assert err <= LOSS_RTOL * abs(float(loss))
    assert gerr <= GRAD_RTOL * gmax


def test_fixture_table_is_the_issues():
    table = {n: tuple(R.fixture(n)[1][k] for k in ('focal', 'S', 'B', 'ncls', 'n_thing', 'h', 'w')) for n in R.FIXTURES}
    assert table == {'focal_tiny': (1, 2, 2, 5, 2, 8, 16), 'focal_cfg': (1, 2, 2, 19, 2, 16, 32), 'ce_kitti': (0, 4, 1, 19, 2, 12, 39),
                     'ce_vipseg': (0, 4, 1, 124, 58, 6, 10), 'ce_s2': (0, 2, 2, 5, 2, 3, 5), 'focal_s1': (1, 1, 3, 33, 8, 5, 7),
                     'ce_s1': (0, 1, 1, 2, 1, 2, 3)}
    for n in ('focal_tiny', 'focal_cfg'):          # the first two ARE the rpn_train goldens' cases: same assignments
        g = R.fixture(n)[0]
        ref = dict(np.load(f'{R.GOLDEN}/rpn_train_{n[6:]}.npz', allow_pickle=False))
        assert np.array_equal(g['assigned'], ref['assigned'])
        assert abs(float(g['loss_f64']) - float(ref['loss_vals'][list(ref['loss_keys']).index('loss_rpn_seg')])) == 0.0


@pytest.mark.parametrize('name', R.PAINT)
def test_paint_rule_is_the_reference_and_the_heads_masked_argmax(vkn, name):
    """the loop of include/vkn_seg_loss.h == the reference's `_get_target_single` (fixture) == this package's head and SegLossTail's
    torch fall-back (one masked arg-max each)"""
    from types import SimpleNamespace
    from importlib import import_module
    ncls, cases = R.paint_fixture()
    c = cases[name]
    H, W = c['masks'].shape[1:]
    want = c['seg_targets']
    assert np.array_equal(R.paint(ncls, (H, W), c['sem'], c['sem_cls'], c['masks'], c['labels'], c['gt_inds']), want)
    masks, labels, gt_inds = torch.from_numpy(c['masks']), torch.from_numpy(c['labels']), torch.from_numpy(c['gt_inds'])
    sem = None if c['sem'] is None else torch.from_numpy(c['sem'])
    cls = None if c['sem_cls'] is None else torch.from_numpy(c['sem_cls'])
    seg_tail = import_module('video_k_net_amd.seg_tail')
    got = seg_tail.paint_targets((H, W), ncls, torch.device('cpu'), sem, cls, masks, labels, gt_inds)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    pos = torch.nonzero(gt_inds > 0).squeeze(-1)
    head = SimpleNamespace(num_classes=ncls, _cfg=vkn.ConvKernelHead._cfg)
    one = vkn.ConvKernelHead._image_targets(head, gt_inds.numel(), (H, W), torch.float32, torch.device('cpu'), pos, masks[gt_inds[pos] - 1],
                                            labels[gt_inds[pos] - 1], sem, cls, dict(pos_weight=1))
    assert np.array_equal(one[4].numpy(), want)
    none = vkn.ConvKernelHead._image_targets(head, gt_inds.numel(), (H, W), torch.float32, torch.device('cpu'), pos, masks[gt_inds[pos] - 1],
                                             labels[gt_inds[pos] - 1], sem, cls, dict(pos_weight=1), with_seg=False)
    assert none[4] is None and all(torch.equal(a, b) for a, b in zip(one[:4], none[:4]))     # the other targets do not depend on it


def test_tail_accepts_the_shipped_losses_by_value(vkn):
    L = vkn.losses
    T = vkn.SegLossTail
    assert T(19, 2, L.FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0)).mode == vkn.ops.SEG_LOSS_FOCAL
    assert T(19, 4, L.CrossEntropyLoss(use_sigmoid=False, loss_weight=1.0)).mode == vkn.ops.SEG_LOSS_CE
    assert T(19, 4, L.CrossEntropyLoss(use_sigmoid=True)).mode is None
    assert T(19, 4, L.CrossEntropyLoss(use_sigmoid=False, class_weight=[1.0] * 19)).mode is None
    assert T(19, 4, L.FocalLoss(reduction='sum')).mode is None and T(19, 4, L.DiceLoss()).mode is None
    assert vkn.ConvKernelHead.fused_seg_loss is False
    sup = vkn.ops.seg_loss_supported
    assert sup(1, 124, 90, 160, 4) and sup(64, 255, 1, 1, 1) and not sup(1, 19, 8, 8, 3) and not sup(1, 256, 8, 8, 2) and not sup(65, 19, 8, 8, 2)
    assert not sup(1, 255, 2048, 1040, 2) and not sup(1, 0, 8, 8, 2)            # ncls h w 4 >= 2^31


def test_composition_fallback_on_the_cpu_equals_the_heads_loss(vkn):
    """Outside the kernels' reach (here: CPU tensors) `SegLossTail` IS today's composition: the reference's map, and its fp32 loss and
    gradient up to the rounding of two fp32 evaluations of the same expression (this CPU's and the fixture's)."""
    g, p, tg = R.fixture('ce_s2')
    tail = vkn.SegLossTail(p['ncls'], p['S'], vkn.losses.CrossEntropyLoss(use_sigmoid=False, loss_weight=1.0))
    t = lambda key: [torch.from_numpy(e[key]) for e in tg]          # noqa: E731
    tgt = tail.targets(t('gt_masks'), t('gt_labels'), t('gt_sem_seg'), t('gt_sem_cls'), [torch.from_numpy(a) for a in g['assigned']])
    assert tail.fused is False and tgt.dtype == torch.int64 and np.array_equal(tgt.numpy(), g['seg_targets'])
    low = torch.from_numpy(g['seg_preds']).requires_grad_(True)
    loss = tail.loss(low, tgt)
    loss.backward()
    assert tail.fused is False
    assert abs(float(loss.detach()) - float(g["loss"])) <= 2 * LOSS_RTOL * float(g['loss'])
    assert float((low.grad - torch.from_numpy(g['grad'])).abs().max()) <= 2 * GRAD_RTOL * float(np.abs(g['grad']).max())


def test_the_vis_head_keeps_its_own_path(vkn):
    assert vkn.ConvKernelHead._seg_tail_allowed is True and vkn.ConvKernelHeadVideo._seg_tail_allowed is False
    assert vkn.ConvKernelHeadVideo.fused_seg_loss is False
