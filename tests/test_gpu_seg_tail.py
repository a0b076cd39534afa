"""GPU: the dense semantic loss of the kernel-initialisation head from the low-res logits (include/vkn_seg_loss.h, csrc/vkn_segloss.hip)
through the C ABI (`ops.seg_targets` / `seg_loss_fwd` / `seg_loss_bwd`) and through `SegLossTail` / `ConvKernelHead.fused_seg_loss`.

Yardsticks: the painted map is exact; loss and gradient are held to the float64 reference of tests/seg_tail_ref.py within
4 x the error of the fp32 torch composition on the same device (the thing being replaced; 4 x allows another summation order), with a
floor of 2^-20 of the value (the composition may happen to land on the float64 value).  Largest errors measured on the MI355X (the
tests print theirs; docs/LAB_NOTEBOOK.md has the table): loss 3.9e-7 of the float64 value where its bound was 1.6e-6, gradient 1.6e-6 of
its maximum where its bound was 6.4e-6 (x 30 logits, equal to the composition's own error), no figure above 34 % of its bound.
"""
import numpy as np
import pytest
import torch

import seg_tail_ref as R
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FLOOR = 2.0 ** -20
SENTINEL = 0xAB


def _dev(a, dtype=None):
    t = torch.as_tensor(np.asarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _truth(tg, assigned):
    """device ground truth of a fixture: (gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_inds) lists"""
    t = lambda key: [_dev(e[key]) for e in tg]          # noqa: E731
    return t('gt_masks'), t('gt_labels'), t('gt_sem_seg'), t('gt_sem_cls'), [_dev(a) for a in assigned]


def _guarded_targets(vkn, masks, labels, sem, cls, gt_inds, ncls, H, W, shift=0):
    """`ops.seg_targets` into a map with a guard row of sentinel bytes before and after (and `shift` bytes in front: the store width
    follows the address) -> (map, dense_pos, guards untouched?)"""
    B = len(masks)
    buf = torch.full((shift + (B * H + 2) * W,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = buf[shift + W: shift + W + B * H * W].view(B, H, W)
    status = torch.zeros((1,), dtype=torch.int32, device=DEV)
    tgt, dense_pos = vkn.ops.seg_targets(masks, labels, sem, cls, gt_inds, ncls, (H, W), tgt=view, status=status)
    torch.cuda.synchronize()
    assert tgt.data_ptr() == view.data_ptr()
    clean = bool((buf[:shift + W] == SENTINEL).all()) and bool((buf[shift + W + B * H * W:] == SENTINEL).all())
    return tgt.cpu().numpy(), int(dense_pos), clean, int(status)


# ---------------------------------------------------------------------------------------------------------------------- targets
@pytest.mark.parametrize('name', R.FIXTURES)
def test_targets_equal_the_reference_map(vkn, name):
    g, p, tg = R.fixture(name)
    H, W = p['S'] * p['h'], p['S'] * p['w']
    masks, labels, sem, cls, gt_inds = _truth(tg, g['assigned'])
    want = g['seg_targets']
    for shift in (0, 1):
        got, dense_pos, clean, status = _guarded_targets(vkn, masks, labels, sem, cls, gt_inds, p['ncls'], H, W, shift)
        assert np.array_equal(got, want) and dense_pos == int((want < p['ncls']).sum()) and clean and status == 0, (name, shift)
    loss_seg = vkn.losses.FocalLoss() if p['focal'] else vkn.losses.CrossEntropyLoss(use_sigmoid=False)
    tail = vkn.SegLossTail(p['ncls'], p['S'], loss_seg)
    tgt = tail.targets(masks, labels, sem, cls, [type('A', (), dict(gt_inds=a))() for a in gt_inds])
    assert tail.fused and tgt.dtype == torch.uint8 and np.array_equal(tgt.cpu().numpy(), want)
    assert int(tgt._vkn_dense_pos) == int((want < p['ncls']).sum())


@pytest.mark.parametrize('name', R.PAINT)
def test_targets_hand_made_layers(vkn, name):
    """overlapping layers, soft values, no stuff, no positive, neither, gt_sem_seg=None, one covered pixel at position 0 and at the last"""
    ncls, cases = R.paint_fixture()
    c = cases[name]
    H, W = c['masks'].shape[1:]
    sem = None if c['sem'] is None else [_dev(c['sem'])]
    cls = None if c['sem_cls'] is None else [_dev(c['sem_cls'])]
    got, dense_pos, clean, status = _guarded_targets(vkn, [_dev(c['masks'])], [_dev(c['labels'])], sem, cls, [_dev(c['gt_inds'])], ncls, H, W)
    assert np.array_equal(got[0], c['seg_targets']) and dense_pos == int((c['seg_targets'] < ncls).sum()) and clean and status == 0
    if name == 'neither':
        assert bool((got == ncls).all()) and dense_pos == 0
    if name == 'corners':
        assert got[0, 0, 0] == 0 and got[0, -1, -1] == 1 and dense_pos == 2


def test_targets_more_layers_than_one_staging_chunk_and_views_of_one_bank(vkn):
    """300 proposals over 4 masks + 3 stuff layers (two LDS chunks); the masks are consecutive views of one bank, as GtPrep leaves them"""
    rng = np.random.default_rng(5)
    H, W, ncls = 9, 261, 11                                     # two column tiles, odd width
    bank = _dev((rng.random((7, H, W)) > 0.7).astype(np.float32) * 0.25)
    masks, sem = bank[:4], bank[4:]
    labels, cls = _dev(np.array([3, 0, 2, 1])), _dev(np.array([8, 9, 10]))
    gt_inds = np.zeros(300, np.int64)
    gt_inds[[2, 40, 255, 256, 299]] = [2, 4, 1, 3, 2]           # ground truth 1 is matched twice: the later row wins where both cover
    got, dense_pos, clean, status = _guarded_targets(vkn, [masks], [labels], [sem], [cls], [_dev(gt_inds)], ncls, H, W, shift=3)
    want = R.paint(ncls, (H, W), sem.cpu().numpy(), cls.cpu().numpy(), masks.cpu().numpy(), labels.cpu().numpy(), gt_inds)
    assert np.array_equal(got[0], want) and dense_pos == int((want < ncls).sum()) and clean and status == 0


def test_out_of_range_label_sets_the_status_bit_and_paints_ncls(vkn):
    ncls, H, W = 5, 4, 7
    m = np.zeros((2, H, W), np.float32)
    m[0, :2], m[1, 1:3, 2:5] = 1, 1
    for labels, gt_inds, want_bit in (([1, 5], [1, 2, 0], 1), ([1, -1], [1, 2, 0], 1), ([1, 2], [1, 3, 2], 1), ([1, 2], [1, 0, 2], 0)):
        got, dense_pos, clean, status = _guarded_targets(vkn, [_dev(m)], [_dev(np.array(labels))], None, None, [_dev(np.array(gt_inds))], ncls, H, W)
        safe = [l if 0 <= l < ncls else ncls for l in labels]
        inds = [k if k <= 2 else 0 for k in gt_inds]            # a gt_inds entry above G paints nothing
        want = R.paint(ncls, (H, W), None, None, m, safe, inds)
        assert np.array_equal(got[0], want) and clean and (status & 1) == want_bit and dense_pos == int((want < ncls).sum()), (labels, gt_inds)


# ----------------------------------------------------------------------------------------------------------- forward and backward
def _bound(comp_err, scale):
    return max(4.0 * comp_err, FLOOR * scale)


def _check(vkn, tag, low, tgt, S, focal, ncls, loss_weight=1.0):
    """forward + backward (g = 1 and g = 3) of one case against float64, bounds from the fp32 composition on the device; the backward
    writes into a NaN-filled buffer with one guard plane on each side.  Returns the errors relative to their bounds' scales."""
    mode = vkn.ops.SEG_LOSS_FOCAL if focal else vkn.ops.SEG_LOSS_CE
    low_d, tgt_d = _dev(low), _dev(tgt)
    B, _, h, w = low.shape
    dense_pos = (tgt_d < ncls).sum().to(torch.int32).reshape(1)
    loss, state = vkn.ops.seg_loss_fwd(low_d, tgt_d, dense_pos, mode, S, R.ALPHA, R.GAMMA, loss_weight)
    out = {}
    for g in (1.0, 3.0):
        ref_loss, ref_grad = R.loss64(low, tgt, S, focal, ncls, loss_weight=loss_weight, g=g)
        c_loss, c_grad = R.compose32(low_d, tgt_d, S, focal, ncls, loss_weight=loss_weight, g=g)
        if g == 1.0:
            err, cerr = abs(float(loss) - float(ref_loss)), abs(float(c_loss) - float(ref_loss))
            print(f'{tag}: loss {float(loss):.9g} f64 {float(ref_loss):.9g} err {err:.3e} composition {cerr:.3e} bound {_bound(cerr, abs(float(ref_loss))):.3e}')
            assert err <= _bound(cerr, abs(float(ref_loss))), (tag, err, cerr)
            out['loss'] = err / max(abs(float(ref_loss)), 1e-300)
        plane = ncls * h * w
        buf = torch.full(((B + 2) * plane,), float('nan'), device=DEV)
        view = buf[plane:(B + 1) * plane].view(B, ncls, h, w)
        got = vkn.ops.seg_loss_bwd(low_d, tgt_d, torch.full((1,), g, device=DEV), state, mode, S, R.ALPHA, R.GAMMA, grad_low=view)
        torch.cuda.synchronize()
        assert got.data_ptr() == view.data_ptr() and bool(torch.isfinite(view).all()), tag          # every element inside is written
        bits, nan = buf.view(torch.int32), torch.full((1,), float('nan')).view(torch.int32).item()
        assert bool((bits[:plane] == nan).all()) and bool((bits[(B + 1) * plane:] == nan).all()), tag   # outside: bitwise untouched
        e = (view.detach().cpu().double() - ref_grad).abs()
        ce = (c_grad.cpu().double() - ref_grad).abs()
        gmax = float(ref_grad.abs().max())
        border = torch.zeros((h, w), dtype=torch.bool)
        border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
        for part, sel in (('all', torch.ones_like(border)), ('border', border), ('inner', ~border)):
            if not bool(sel.any()):
                continue
            pe, pce = float(e[:, :, sel].max()), float(ce[:, :, sel].max())
            print(f'{tag}: g={g} grad[{part}] err {pe:.3e} composition {pce:.3e} bound {_bound(pce, gmax):.3e} max|grad| {gmax:.3e}')
            assert pe <= _bound(pce, gmax), (tag, g, part, pe, pce)
        out[f'grad{g:g}'] = float(e.max()) / max(gmax, 1e-300)
    return out


@pytest.mark.parametrize('scale', (1, 30))
@pytest.mark.parametrize('name', R.FIXTURES)
def test_loss_and_gradient_on_the_fixture_inputs(vkn, name, scale):
    g, p, _ = R.fixture(name)
    _check(vkn, f'{name} x{scale}', g['seg_preds'] * np.float32(scale), g['seg_targets'], p['S'], p['focal'], p['ncls'], float(g['loss_weight']))


@pytest.mark.parametrize('scale', (1, 30))
@pytest.mark.parametrize('focal', (1, 0))
@pytest.mark.parametrize('i', range(len(R.EXTRA_SHAPES)))
def test_loss_and_gradient_on_the_edge_shapes(vkn, i, focal, scale):
    """(B, ncls, h, w, S) = (1, 1, 1, 1, 1), (1, 255, 3, 5, 2), (1, 2, 2, 3, 4); x30 saturates the sigmoids and exercises the max subtraction"""
    low, tgt, _ = R.extra_case(i, focal, scale)
    B, ncls, h, w, S = R.EXTRA_SHAPES[i]
    _check(vkn, f'{R.EXTRA_SHAPES[i]} {"focal" if focal else "ce"} x{scale}', low, tgt, S, focal, ncls)


def test_more_than_one_workgroup_and_a_weighted_focal(vkn):
    """67 x 70 low-res at S = 2: two workgroup columns and many rows in both kernels, a partial last tile in each; loss_weight 0.5 and
    (in the class-split backward) 19 classes over four workgroups"""
    rng = np.random.default_rng(11)
    for focal, S, (h, w), ncls in ((1, 2, (67, 70), 19), (0, 4, (5, 130), 9), (0, 1, (9, 64), 3)):
        low = rng.standard_normal((2, ncls, h, w)).astype(np.float32) * 3
        tgt = rng.integers(0, ncls + 1, (2, S * h, S * w)).astype(np.uint8)
        _check(vkn, f'big focal={focal} S={S}', low, tgt, S, focal, ncls, loss_weight=0.5)


def test_an_all_ignored_image_has_an_exactly_zero_gradient(vkn):
    """CE: ignored pixels contribute exactly zero — image 1 of 2 is all `ncls`: its grad_low is +0.0 bitwise, and the loss is image 0's"""
    rng = np.random.default_rng(3)
    ncls, h, w, S = 7, 5, 9, 4
    low = rng.standard_normal((2, ncls, h, w)).astype(np.float32) * 4
    tgt = rng.integers(0, ncls, (2, S * h, S * w)).astype(np.uint8)
    tgt[1] = ncls
    loss, state = vkn.ops.seg_loss_fwd(_dev(low), _dev(tgt), None, vkn.ops.SEG_LOSS_CE, S)
    grad = vkn.ops.seg_loss_bwd(_dev(low), _dev(tgt), torch.full((1,), 3.0, device=DEV), state, vkn.ops.SEG_LOSS_CE, S)
    assert bool((grad[1].view(torch.int32) == 0).all()) and float(grad[0].abs().max()) > 0
    ref, _ = R.loss64(low, tgt, S, 0, ncls)
    assert abs(float(loss) - float(ref)) <= 4 * FLOOR * float(ref)


# ------------------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize('name', R.FIXTURES)
def test_tail_against_the_reference_loss_and_gradient(vkn, name):
    """`SegLossTail` from the step's ground truth and the reference's assignments: `loss_rpn_seg` within 1e-4 (the tolerance
    tests/test_gpu_train.py holds the rpn losses to), the gradient by that file's `_check_grad` rule; two calls give the same bits."""
    from test_gpu_train import _check_grad
    g, p, tg = R.fixture(name)
    masks, labels, sem, cls, gt_inds = _truth(tg, g['assigned'])
    loss_seg = (vkn.losses.FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0) if p['focal']
                else vkn.losses.CrossEntropyLoss(use_sigmoid=False, loss_weight=1.0))
    tail = vkn.SegLossTail(p['ncls'], p['S'], loss_seg)
    runs = []
    for _ in range(2):
        low = _dev(g['seg_preds']).requires_grad_(True)
        loss = tail.loss(low, tail.targets(masks, labels, sem, cls, gt_inds))
        assert tail.fused and loss.dim() == 0
        (loss * 1.0).backward()
        runs.append((loss.detach().clone(), low.grad.clone()))
    ref = float(g['loss_f64'])
    assert abs(float(runs[0][0]) - ref) < 1e-4 * max(1.0, abs(ref)) and abs(float(runs[0][0]) - ref) < 1e-4 * abs(ref), (float(runs[0][0]), ref)
    _check_grad(g, 'grad', runs[0][1])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))     # determinism


# -------------------------------------------------------------------------------------------------------------------------- wiring
def _rpn_head(vkn, p, fused, stride=2, loss_seg=None):
    from helpers import make_init_case
    loc, sem, iw, sw, sb = make_init_case(p)
    head = vkn.build_head(dict(
        type='ConvKernelHead', num_proposals=p['nprop'], in_channels=p['C'], out_channels=p['C'], num_loc_convs=0, num_seg_convs=0,
        localization_fpn=None, conv_kernel_size=1, semantic_fpn=True, num_classes=p['ncls'], use_binary=True,
        proposal_feats_with_obj=True, feat_downsample_stride=stride, feat_refine=False, num_thing_classes=p['n_thing'],
        num_stuff_classes=p['ncls'] - p['n_thing'], cat_stuff_mask=True,
        loss_rank=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.1),
        loss_seg=loss_seg or dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
        loss_mask=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0), loss_dice=dict(type='DiceLoss', loss_weight=4.0),
        train_cfg=dict(assigner=dict(type='MaskHungarianAssigner', cls_cost=dict(type='FocalLossCost', weight=2.0),
                                     dice_cost=dict(type='DiceCost', weight=4.0, pred_act=True),
                                     mask_cost=dict(type='MaskCost', weight=1.0, pred_act=True)),
                       sampler=dict(type='MaskPseudoSampler'), pos_weight=1)))
    head.load_state_dict({'init_kernels.weight': iw, 'conv_seg.weight': sw, 'conv_seg.bias': sb}, strict=True)
    head = head.to(DEV).train()
    head._upstream_feats = lambda img: img          # the pass-through neck of the golden
    if fused is not None:
        head.fused_seg_loss = fused
    return head, loc, sem


def _count_entries(vkn, monkeypatch):
    calls = dict(seg_targets=0, seg_loss_fwd=0, seg_loss_bwd=0)
    for k in calls:
        orig = getattr(vkn.ops, k)

        def counted(*a, _k=k, _orig=orig, **kw):
            calls[_k] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(vkn.ops, k, counted)
    return calls


@pytest.mark.parametrize('name', ['rpn_train_tiny', 'rpn_train_cfg'])
def test_conv_kernel_head_with_the_fused_seg_loss_vs_reference_golden(vkn, name, monkeypatch):
    """`ConvKernelHead.forward_train` as tests/test_gpu_train.py builds it, with `fused_seg_loss = True`, on the existing goldens: all
    losses within 1e-4, assignments bit-exact, grad_sem / grad_loc and every parameter's gradient by `_check_grad`; the three entry
    points run once each.  With the default (False) they are never reached."""
    from helpers import GOLDEN, INIT_FIELDS
    from test_gpu_train import _check_grad
    g = dict(np.load(f'{GOLDEN}/{name}.npz', allow_pickle=False))
    p = dict(zip(INIT_FIELDS, (int(v) for v in g['case'])))
    calls = _count_entries(vkn, monkeypatch)
    tg = synth.train_targets(p['B'], p['n_thing'], p['ncls'] - p['n_thing'], 2 * p['H'], 2 * p['W'], p['seed'])
    t = lambda key: [torch.from_numpy(e[key]).to(DEV) for e in tg]  # noqa: E731
    for fused in (None, True):
        head, loc, sem = _rpn_head(vkn, p, fused)
        assert head.fused_seg_loss is bool(fused)
        locd, semd = loc.to(DEV).requires_grad_(True), sem.to(DEV).requires_grad_(True)
        assigned = []
        orig = head.assigner.assign

        def rec(*args, _orig=orig, **kw):
            r = _orig(*args, **kw)
            assigned.append(r.gt_inds.clone())
            return r
        head.assigner.assign = rec
        losses, prop, x_feats, masks, cls = head.forward_train((locd, semd), [dict() for _ in range(p['B'])], t('gt_masks'), t('gt_labels'),
                                                               gt_sem_seg=t('gt_sem_seg'), gt_sem_cls=t('gt_sem_cls'))
        assert cls is None and sorted(losses) == list(g['loss_keys'])
        assert np.array_equal(torch.stack(assigned).cpu().numpy(), g['assigned']), 'Hungarian assignments must be bit-exact'
        for k, ref in zip(g['loss_keys'], g['loss_vals']):
            assert abs(float(losses[k]) - ref) < 1e-4 * max(1.0, abs(ref)), (k, float(losses[k]), ref)
        total = sum(v for k, v in losses.items() if 'loss' in k) + 1e-3 * (prop ** 2).mean() + 1e-3 * (masks ** 2).mean()
        assert abs(float(total) - float(g['total'])) < 1e-4 * abs(float(g['total']))
        total.backward()
        _check_grad(g, 'grad_loc', locd.grad)
        _check_grad(g, 'grad_sem', semd.grad)
        named = dict(head.named_parameters())
        assert sorted(named) == list(g['grad_keys'])
        for i, k in enumerate(g['grad_keys']):
            _check_grad(g, f'grad_{i}', named[str(k)].grad)
        if not fused:
            assert calls == dict(seg_targets=0, seg_loss_fwd=0, seg_loss_bwd=0), calls
        else:
            assert calls == dict(seg_targets=1, seg_loss_fwd=1, seg_loss_bwd=1), calls
            assert head._seg_tail().fused


@pytest.mark.parametrize('S,ncls', [(3, 5), (2, 256)])
def test_outside_the_envelope_the_composition_runs_with_the_same_values(vkn, S, ncls):
    """S = 3 and ncls = 256: `.fused` is False, the C entries return VKN_E_SHAPE, and the values are the composition's"""
    rng = np.random.default_rng(S * 1000 + ncls)
    h, w, B, n_thing = 3, 4, 2, 2
    H, W = S * h, S * w
    masks = [_dev((rng.random((3, H, W)) > 0.6).astype(np.float32)) for _ in range(B)]
    labels = [_dev(rng.integers(0, n_thing, 3)) for _ in range(B)]
    sem = [_dev((rng.random((2, H, W)) > 0.5).astype(np.float32)) for _ in range(B)]
    cls = [_dev(np.array([n_thing, ncls - 1])) for _ in range(B)]
    gt_inds = [_dev(np.array([0, 2, 0, 1, 3, 0])) for _ in range(B)]
    tail = vkn.SegLossTail(ncls, S, vkn.losses.CrossEntropyLoss(use_sigmoid=False, loss_weight=1.0))
    tgt = tail.targets(masks, labels, sem, cls, gt_inds)
    assert tail.fused is False and tgt.dtype == torch.int64
    want = np.stack([R.paint(ncls, (H, W), sem[b].cpu().numpy(), cls[b].cpu().numpy(), masks[b].cpu().numpy(), labels[b].cpu().numpy(),
                             gt_inds[b].cpu().numpy()).astype(np.int64) for b in range(B)])
    assert np.array_equal(tgt.cpu().numpy(), want)
    low_np = rng.standard_normal((B, ncls, h, w)).astype(np.float32)
    low = _dev(low_np).requires_grad_(True)
    loss = tail.loss(low, tgt)
    loss.backward()
    assert tail.fused is False
    c_loss, c_grad = R.compose32(_dev(low_np), tgt, S, 0, ncls)
    # the same torch ops on the same device: the forward bit for bit; torch's up-scaling adjoint adds with atomics, so a gradient
    # element is the same <= (2 S)^2 fp32 terms in another order
    assert torch.equal(loss.detach(), c_loss)
    assert float((low.grad - c_grad).abs().max()) <= FLOOR * float(c_grad.abs().max())
    L = vkn._lib.lib()
    d = lambda x: x.data_ptr()          # noqa: E731
    u8 = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    out, state = torch.zeros((1,), device=DEV), torch.zeros((4096,), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        assert L.vkn_seg_loss_fwd_f32(d(low), d(u8), None, 1, B, ncls, h, w, S, 0.0, 0.0, 1.0, d(out), d(state), None) == -2
        assert L.vkn_seg_loss_bwd_f32(d(low), d(u8), d(out), 1, B, ncls, h, w, S, 0.0, 0.0, d(state), d(low.grad), None) == -2
        assert L.vkn_seg_loss_state_bytes(1, B, h, w, S) == (0 if S == 3 else L.vkn_seg_loss_state_bytes(1, B, h, w, 2))
        if ncls == 256:
            imgs = (vkn._lib.VknSegImage * 1)(vkn._lib.VknSegImage(None, None, None, None, None, 0, 0, 0))
            assert L.vkn_seg_targets_u8(imgs, 1, H, W, ncls, d(u8), d(out), d(out), None) == -2


# --------------------------------------------------------------------------------------------------------- determinism and capture
@pytest.mark.parametrize('name', ['focal_cfg', 'ce_kitti'])
def test_two_calls_give_equal_bits_and_a_captured_graph_replays_them(vkn, name):
    """targets + forward + backward through `SegLossTail` / `SegLossFn`, captured once in `torch.cuda.graph` on a single stream (no
    forks) and replayed twice: the eager bits.  A host read or a data-dependent shape would fail the capture."""
    g, p, tg = R.fixture(name)
    masks, labels, sem, cls, gt_inds = _truth(tg, g['assigned'])
    low = _dev(g['seg_preds']).requires_grad_(True)
    loss_seg = vkn.losses.FocalLoss() if p['focal'] else vkn.losses.CrossEntropyLoss(use_sigmoid=False)
    tail = vkn.SegLossTail(p['ncls'], p['S'], loss_seg)

    def step():
        tgt = tail.targets(masks, labels, sem, cls, gt_inds)
        loss = tail.loss(low, tgt)
        return tgt, loss, torch.autograd.grad(loss, low)[0]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        eager = [tuple(t.detach().clone() for t in step()) for _ in range(2)]
    stream.synchronize()
    for a, b in zip(*eager):
        assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
    assert not bool(torch.isnan(eager[0][2]).any()) and tail.fused
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        static = [t.detach() for t in step()]
    for _ in range(2):
        for t in static:
            t.fill_(0) if t.dtype == torch.uint8 else t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager[0], static):
            assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
    vkn.ops.workspace_status(DEV)
