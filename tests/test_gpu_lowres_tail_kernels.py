"""GPU: the loss tail's two low-res kernels on ragged maps (odd heights / widths, one-row and one-column maps, both strides) and at the
frame shapes of the shipped configs (KITTI-STEP 48 x 156 at x4 and x2, Cityscapes 128 x 256 at x4 with two frames).
  forward:  vkn_mask_losses_fwd_lowres_f32   vs   vkn_upsample_bilinear_f32 + vkn_mask_losses_fwd_bank_f32     (kernel vs kernel)
  backward: vkn_mask_losses_bwd_lowres_f32   vs   vkn_mask_losses_bwd_bank_f32 + vkn_upsample_bilinear_bwd_f32 (kernel vs kernel)
  both      vs   an independent float64 reference (helpers.lowres_tail_reference: F.interpolate + mmdet's losses restated, autograd), so
                 that a mistake both kernel forms share (rank target rule, border clamp, normalisation) cannot pass
(knet/det/kernel_update_head.py:122-130 up-scaling, :279-349 loss_mask / loss_dice / loss_rank)"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _case(B, Ns, h, w, S, K, masks='pixels'):
    """low-res logits, target bank [K, S h, S w] and the row tables of K random positive rows (positive k = bank row k).  masks='pixels':
    every target pixel on with probability 0.4; 'rects': one rectangle per target (10-40 % of each side) — targets overlap and some
    pixels no positive row covers."""
    g = torch.Generator().manual_seed(100 * h + w)
    low = (torch.randn(B, Ns, h, w, generator=g) * 3).to(DEV)
    H, W = S * h, S * w
    if masks == 'pixels':
        bank = (torch.rand(K, H, W, generator=g) > 0.6).float().to(DEV)
    else:
        bank = torch.zeros(K, H, W)
        for k in range(K):
            mh, mw = (int(v) for v in (torch.rand(2, generator=g) * 0.3 + 0.1) * torch.tensor([H, W]) + 1)
            y0, x0 = int(torch.randint(0, H - mh + 1, (1,), generator=g)), int(torch.randint(0, W - mw + 1, (1,), generator=g))
            bank[k, y0:y0 + mh, x0:x0 + mw] = 1.0
        bank = bank.to(DEV)
    rowk = torch.full((B * Ns,), -1, dtype=torch.int32)
    tgt = torch.zeros(B * Ns, dtype=torch.int32)
    pos = torch.randperm(B * Ns, generator=g)[:K].sort()[0]
    if Ns == 256:
        pos[-1] = B * Ns - 1                      # the last row of a 256-row frame is positive: top = 255 is a real row index
        pos = pos.unique()
        K = int(pos.numel())
        bank = bank[:K].contiguous()
    rowk[pos] = torch.arange(K, dtype=torch.int32)
    tgt[pos] = torch.arange(K, dtype=torch.int32)
    return g, low, bank, rowk.to(DEV), tgt.to(DEV), pos.to(DEV), K


@pytest.mark.parametrize('B,Ns,h,w,S,K', [(2, 23, 7, 13, 4, 9), (3, 40, 5, 70, 2, 17), (1, 117, 1, 9, 4, 5), (2, 9, 11, 1, 2, 4), (1, 256, 6, 10, 4, 30)],
                         ids=['7x13x4', '5x70x2', 'one_row', 'one_col', 'ns256'])
def test_lowres_forward_and_backward_on_ragged_maps(vkn, B, Ns, h, w, S, K):
    L, ops = vkn._lib.lib(), vkn.ops
    g, low, bank, rowk, tgt, posd, K = _case(B, Ns, h, w, S, K)
    H, W = S * h, S * w
    P = H * W
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    scaled = ops.upsample_bilinear(low, S)
    # ---- forward
    nch, nbl, ncl = L.vkn_mask_losses_chunks(P), L.vkn_mask_losses_blocks(P), L.vkn_mask_losses_lowres_chunks(h, w)
    rp0, rk0 = torch.zeros(K, nch, 4, device=DEV), torch.zeros(B, nbl, device=DEV)
    lse0, top0 = torch.zeros(B, P, device=DEV), torch.zeros(B, P, dtype=torch.int32, device=DEV)
    rp1, rk1 = torch.zeros(K, ncl, 4, device=DEV), torch.zeros(B, ncl, device=DEV)
    lse1, top1 = torch.full((B, P), float('nan'), device=DEV), torch.full((B, P), -7, dtype=torch.int32, device=DEV)
    if P % 4 == 0:
        assert L.vkn_mask_losses_fwd_bank_f32(p(scaled), p(bank), p(tgt), p(posd), p(rowk), K, B, Ns, P, 1, p(rp0), p(lse0), p(top0), p(rk0), st) == 0
    assert L.vkn_mask_losses_fwd_lowres_f32(p(low), p(bank), p(tgt), p(rowk), K, B, Ns, h, w, S, 1, p(rp1), p(lse1), p(top1), p(rk1), st) == 0
    torch.cuda.synchronize()
    if P % 4 == 0:
        a, b_ = rp0.double().sum(1), rp1.double().sum(1)
        assert float(((a - b_).abs() / a.abs().clamp(min=1.0)).max()) < 2e-6
        assert torch.equal(top0, top1) and float((lse0 - lse1).abs().max()) < 2e-5        # (every pixel was written: no NaN / -7 left)
        assert abs(float(rk0.double().sum()) - float(rk1.double().sum())) < 2e-6 * max(1.0, abs(float(rk0.double().sum())))
    else:      # (the up-scaled form needs P % 4 == 0: compare with torch)
        z = scaled.double().reshape(B, Ns, P)
        assert float((torch.logsumexp(z, 1).float() - lse1).abs().max()) < 2e-5
    # ---- backward
    a_, bc = (torch.rand(K, generator=g) * 50).to(DEV), (torch.rand(K, generator=g) * 50 + 60).to(DEV)
    one = torch.ones(1, device=DEV)
    out_lr = torch.full_like(low, float('nan'))
    assert L.vkn_mask_losses_bwd_lowres_f32(p(low), p(bank), p(tgt), p(rowk), p(a_), p(bc), p(one), p(one), p(one), 1.0, 4.0, 0.1, K, p(lse1),
                                            p(top1), B, Ns, h, w, S, 1, p(out_lr), st) == 0
    if P % 4 == 0:
        gs = torch.empty_like(scaled)
        assert L.vkn_mask_losses_bwd_bank_f32(p(scaled), p(bank), p(tgt), p(rowk), p(a_), p(bc), p(one), p(one), p(one), 1.0, 4.0, 0.1, K, p(lse1),
                                              p(top1), B, Ns, P, 1, p(gs), st) == 0
        ref = ops.upsample_bilinear_bwd(gs, S)
        torch.cuda.synchronize()
        assert float((out_lr - ref).abs().max()) < 2e-6 * float(ref.abs().max())
    else:
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out_lr).all())


def test_lowres_forward_logsumexp_survives_a_huge_spread(vkn):
    """k_ml_fwd_lr sums exp(z - Mb) against ONE reference point per block (the maximum of the block's taps over all rows); logits spread
    over +-600 underflow that sum at pixels far from the maximal tap — those blocks are redone with the online form: the lse must still be
    torch's logsumexp of the up-scaled logits, with no inf / NaN."""
    L, ops = vkn._lib.lib(), vkn.ops
    B, Ns, h, w, S, K = 2, 31, 9, 20, 4, 3
    g = torch.Generator().manual_seed(9)
    low = (torch.randn(B, Ns, h, w, generator=g) * 200).to(DEV)
    H, W = S * h, S * w
    P = H * W
    bank = (torch.rand(K, H, W, generator=g) > 0.5).float().to(DEV)
    rowk = torch.full((B * Ns,), -1, dtype=torch.int32)
    tgt = torch.zeros(B * Ns, dtype=torch.int32)
    rowk[[3, 17, 40]] = torch.arange(K, dtype=torch.int32)
    tgt[[3, 17, 40]] = torch.arange(K, dtype=torch.int32)
    rowk, tgt = rowk.to(DEV), tgt.to(DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ncl = L.vkn_mask_losses_lowres_chunks(h, w)
    rp, rk = torch.zeros(K, ncl, 4, device=DEV), torch.zeros(B, ncl, device=DEV)
    lse, top = torch.full((B, P), float('nan'), device=DEV), torch.full((B, P), -7, dtype=torch.int32, device=DEV)
    assert L.vkn_mask_losses_fwd_lowres_f32(p(low), p(bank), p(tgt), p(rowk), K, B, Ns, h, w, S, 1, p(rp), p(lse), p(top), p(rk), st) == 0
    torch.cuda.synchronize()
    want = torch.logsumexp(ops.upsample_bilinear(low, S).double().reshape(B, Ns, P), 1)
    assert bool(torch.isfinite(lse).all())
    assert float((lse.double() - want).abs().max()) < 1e-4 * float(want.abs().max())
    spread = (ops.upsample_bilinear(low, S).reshape(B, Ns, P).amax(1) - low.reshape(B, Ns, -1).amax((1, 2), keepdim=False)[:, None]).min()
    assert float(spread) < -100.0          # (some pixel's best row really lies far below the map's largest tap: the case exists in this input)


W_LOSS, G_UP = (1.0, 4.0, 0.1), (0.7, 1.3, 0.9)      # loss weights (w_mask, w_dice, w_rank) and upstream gradients (g_mask, g_dice, g_rank)
F64_CASES = [(2, 23, 7, 13, 4, 9, 'pixels'), (3, 40, 5, 70, 2, 17, 'pixels'), (1, 117, 1, 9, 4, 5, 'pixels'), (2, 9, 11, 1, 2, 4, 'pixels'),
             (1, 256, 6, 10, 4, 30, 'pixels'), (1, 117, 48, 156, 4, 30, 'rects'), (2, 117, 48, 156, 2, 40, 'rects'),
             (2, 117, 128, 256, 4, 60, 'rects')]


@pytest.mark.parametrize('B,Ns,h,w,S,K,masks', F64_CASES,
                         ids=['7x13x4', '5x70x2', 'one_row', 'one_col', 'ns256', 'kitti_48x156x4', 'kitti_48x156x2_b2', 'cfg3_128x256x4_b2'])
def test_lowres_tail_vs_float64_reference(vkn, B, Ns, h, w, S, K, masks):
    """Both low-res kernels against helpers.lowres_tail_reference (float64, autograd).  Forward: the per-row sums (BCE, a, b, c), the
    logsumexp, the rank target (exact) and the rank sum.  Backward (fed the reference's dice a / b + c, lse and rank target, so it is
    checked on its own): grad_low against autograd's d/d low of g_mask w_mask loss_mask + g_dice w_dice loss_dice + g_rank w_rank loss_rank."""
    from helpers import lowres_tail_reference, record_margins
    L = vkn._lib.lib()
    _, low, bank, rowk, tgt, _, K = _case(B, Ns, h, w, S, K, masks)
    P = S * h * S * w
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ncl = L.vkn_mask_losses_lowres_chunks(h, w)
    rp, rk = torch.zeros(K, ncl, 4, device=DEV), torch.zeros(B, ncl, device=DEV)
    lse, top = torch.full((B, P), float('nan'), device=DEV), torch.full((B, P), -7, dtype=torch.int32, device=DEV)
    assert L.vkn_mask_losses_fwd_lowres_f32(p(low), p(bank), p(tgt), p(rowk), K, B, Ns, h, w, S, 1, p(rp), p(lse), p(top), p(rk), st) == 0
    ref = lowres_tail_reference(low, bank, tgt, rowk, S, W_LOSS, G_UP)
    torch.cuda.synchronize()
    if masks == 'rects':      # (the case exists: overlapping targets, and pixels no positive row covers)
        assert bool((ref['top'] == -1).any()) and float(bank.sum()) > float((bank.sum(0) > 0).sum())
    # ---- forward
    e_rows = float(((rp.double().sum(1) - ref['rows']).abs() / ref['rows'].abs().clamp(min=1.0)).max())
    e_lse = float((lse.double() - ref['lse']).abs().max())
    e_rank = abs(float(rk.double().sum()) - ref['rank_sum']) / max(1.0, abs(ref['rank_sum']))
    # ---- backward, on the reference's forward quantities
    gs = [torch.full((1,), v, device=DEV) for v in G_UP]
    a_, bc = ref['dice_a'].float().contiguous(), ref['dice_bc'].float().contiguous()
    lse_r, top_r = ref['lse'].float().contiguous(), ref['top'].contiguous()
    grad = torch.full_like(low, float('nan'))
    assert L.vkn_mask_losses_bwd_lowres_f32(p(low), p(bank), p(tgt), p(rowk), p(a_), p(bc), p(gs[0]), p(gs[1]), p(gs[2]), W_LOSS[0], W_LOSS[1],
                                            W_LOSS[2], K, p(lse_r), p(top_r), B, Ns, h, w, S, 1, p(grad), st) == 0
    torch.cuda.synchronize()
    e_grad = float((grad.double() - ref['grad']).abs().max()) / float(ref['grad'].abs().max())
    record_margins(f'lowres_tail_f64[{B}x{Ns}x{h}x{w}x{S}]', dict(rows=e_rows, lse=e_lse, rank=e_rank, grad=e_grad))
    assert torch.equal(top, ref['top'])
    # fp32 budget: every sum is a fixed-order fp32 reduction of up to 2^19 terms, the lse a log of a sum of Ns exponentials.  Measured on
    # the MI355X, largest over the eight cases: rows 1.2e-7, lse 2.4e-6 (absolute, |lse| ~ 10), rank 6.2e-8, grad 2.0e-7 (of max |grad|)
    assert e_rows < 2.5e-7 and e_lse < 5e-6 and e_rank < 1.5e-7
    assert e_grad < 4e-7


def test_lowres_backward_refuses_more_than_256_rows(vkn):
    """Ns = 300 (> 256: the backward holds the rank target as one byte per pixel): VKN_E_SHAPE with real, correctly sized buffers, before
    anything is launched (the output stays untouched); and the forward's alignment rule (8 bytes) for bank / lse / top"""
    L = vkn._lib.lib()
    B, Ns, h, w, S, K = 1, 300, 6, 10, 4, 7
    _, low, bank, rowk, tgt, _, K = _case(B, Ns, h, w, S, K, 'rects')
    P = S * h * S * w
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    a_, bc = torch.ones(K, device=DEV), torch.full((K,), 3.0, device=DEV)
    one = torch.ones(1, device=DEV)
    lse, top = torch.zeros(B, P, device=DEV), torch.full((B, P), -1, dtype=torch.int32, device=DEV)
    grad = torch.full_like(low, float('nan'))
    args = lambda bk, ls, tp: (p(low), p(bk), p(tgt), p(rowk), p(a_), p(bc), p(one), p(one), p(one), 1.0, 4.0, 0.1, K, p(ls), p(tp), B)  # noqa: E731
    assert L.vkn_mask_losses_bwd_lowres_f32(*args(bank, lse, top), Ns, h, w, S, 1, p(grad), st) == -2          # VKN_E_SHAPE
    # (the same buffers as a 250-row problem pass the shape gate; offset by 4 bytes they fail the alignment gate: VKN_E_ALIGN.  Each offset
    #  view lies in a buffer one element longer, so that it is full-length: in bounds even if the gate were missing)
    def shifted(t):
        big = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        big[1:] = t.reshape(-1)
        return big[1:]
    assert L.vkn_mask_losses_bwd_lowres_f32(*args(shifted(bank), lse, top), 250, h, w, S, 1, p(grad), st) == -5
    assert L.vkn_mask_losses_bwd_lowres_f32(*args(bank, shifted(lse), top), 250, h, w, S, 1, p(grad), st) == -5
    assert L.vkn_mask_losses_bwd_lowres_f32(*args(bank, lse, shifted(top)), 250, h, w, S, 1, p(grad), st) == -5
    torch.cuda.synchronize()
    assert bool(torch.isnan(grad).all())


def test_stage_tail_beyond_256_rows_takes_the_upscaled_gradient(vkn):
    """`TailStep.stage_losses` with low-res logits of Ns = 300 rows: the low-res kernels do not take that shape, so the losses come from
    the up-scaled values and the gradient through the upsample's adjoint — the float64 reference's losses and gradient w.r.t. the
    low-res logits (before: the low-res backward ran anyway and read a wrong rank target)."""
    from importlib import import_module
    from types import SimpleNamespace

    from helpers import lowres_tail_reference
    tt = import_module('video_k_net_amd.train_tail')
    B, Ns, h, w, S, G = 1, 300, 6, 10, 4, 9
    _, low, bank, _, _, _, _ = _case(B, Ns, h, w, S, G, 'rects')
    rows = torch.tensor([3, 40, 41, 100, 180, 255, 256, 270, 299], dtype=torch.int32, device=DEV)     # positive rows: past 255 too
    cols = torch.tensor([4, 0, 8, 2, 7, 1, 3, 6, 5], dtype=torch.int32, device=DEV)                   # their targets
    labels = torch.zeros(G, dtype=torch.int64, device=DEV)
    step = tt.TailStep(torch.device(DEV), [bank], [labels], None, None)
    lossmod = SimpleNamespace
    head = SimpleNamespace(num_stuff_classes=0, num_thing_classes=1, num_classes=1,
                           loss_cls=lossmod(loss_weight=2.0, alpha=0.25, gamma=2.0), loss_mask=lossmod(loss_weight=W_LOSS[0]),
                           loss_dice=lossmod(loss_weight=W_LOSS[1], eps=1e-3), loss_rank=lossmod(loss_weight=W_LOSS[2]))
    cls_score = torch.randn(B, Ns, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    lowg = low.clone().requires_grad_(True)
    scaled = vkn.ops.upsample_bilinear(low, S)
    out = step.stage_losses(head, dict(pos_weight=1.0), [SimpleNamespace(_pairs32=(rows, cols))], cls_score, scaled, lowres=lowg, stride=S)
    (G_UP[0] * out['loss_mask'] + G_UP[1] * out['loss_dice'] + G_UP[2] * out['loss_rank']).backward()
    rowk = torch.full((B * Ns,), -1, dtype=torch.int32, device=DEV)
    tgt = torch.zeros(B * Ns, dtype=torch.int32, device=DEV)
    rowk[rows.long()] = torch.arange(G, dtype=torch.int32, device=DEV)
    tgt[rows.long()] = cols
    ref = lowres_tail_reference(low, bank, tgt, rowk, S, W_LOSS, G_UP)
    for name, i in (('loss_mask', 0), ('loss_dice', 1), ('loss_rank', 2)):
        assert abs(float(out[name]) - W_LOSS[i] * ref['losses'][i]) < 1e-5 * max(1.0, abs(W_LOSS[i] * ref['losses'][i])), name
    assert float((lowg.grad.double() - ref['grad']).abs().max()) < 1e-5 * float(ref['grad'].abs().max())
