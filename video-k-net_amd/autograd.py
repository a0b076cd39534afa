"""Differentiable wrappers of the two x-streaming HIP ops (training, BASELINE cfg3; SURVEY.md §8(a) footnote).

The binarised mask carries no gradient (`.float()` of a bool, knet/det/kernel_update_head.py:191-192), so
  * gather  xraw = M x^T           is differentiable w.r.t. x only:   dx  = M^T dxraw            (decode-shaped)
  * decode  Z = K x + kb           w.r.t. both operands:              dK  = dZ x^T, dkb = sum dZ (gather-shaped, real operand)
                                                                      dx  = K^T dZ              (decode-shaped)
i.e. the backward passes are the SAME two kernel shapes with transposed operands: `vkn_mask_decode_f32` with the roles of
channels and kernels swapped, and `vkn_mask_gather_real_f32`.  Gradient operands are scaled by a power of two into the f16
hi/lo split's range first (exact in fp32) and the result is scaled back.  Dynamic range: ONE power-of-two scale per tensor puts
max|g| at ~2^10; an element more than ~2^34 below the tensor's maximum falls under the smallest f16 subnormal of the low half
(2^-24) and contributes zero — irrelevant for loss gradients (their spread inside one tensor is far smaller) but it is a limit.
"""
import math

import torch

from . import ops


def _pow2_scale(t, target=1024.0):
    """Power of two s (device scalar tensor) with max|t| * s in [target / 2, target) (2^10-ish for an all-zero tensor: harmless).
    One reduction pass (`max |t|` as the infinity norm, no |t| temporary) and three scalar ops; nothing touches the host."""
    t = t.detach()
    if t.numel() == 0:
        return torch.ones((), dtype=torch.float32, device=t.device)
    # (measured: vector_norm(inf) takes 34 us whatever the size — right for the 61 MB logit gradients, 6x slower than abs + amax on
    #  the [B, N, C] kernel gradients)
    m = torch.linalg.vector_norm(t, ord=float('inf')) if t.numel() > (1 << 22) else t.abs().amax()
    e = torch.frexp(m)[1]                                              # m = mantissa * 2^e, mantissa in [0.5, 1)
    return torch.ldexp(torch.ones_like(m), (int(math.floor(math.log2(target))) - e).clamp_(-100, 100))


def _scaled_rows(t, s, mult=32):
    """t [B, R, ...] * s with the rows zero-padded to a multiple of `mult`: one pass over t (no concatenation)."""
    r = t.shape[1]
    rp = (r + mult - 1) // mult * mult
    out = torch.empty((t.shape[0], rp) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
    torch.mul(t, s, out=out[:, :r])
    if rp != r:
        out[:, r:].zero_()
    return out


def _pad_last(t, n):
    """[..., m] -> [..., n] zero-padded (n >= m), contiguous."""
    if t.shape[-1] == n:
        return t.contiguous()
    out = t.new_zeros(tuple(t.shape[:-1]) + (n,))
    out[..., :t.shape[-1]] = t
    return out


def _decode_unscaled(x, kernels, inv):
    """decode(x, kernels) * inv with the multiplication inside the decode kernel where it applies (MFMA kernel: even H*W), else behind it."""
    if (x.shape[-1] * x.shape[-2]) % 2 == 0:
        return ops.mask_decode(x, kernels, out_scale=inv)
    return ops.mask_decode(x, kernels).mul_(inv)


class _XHub:
    """Collects the feature map's gradient contributions of ONE backward pass (see `x_hub`).  A pass that never reaches the hub's
    node — `torch.autograd.grad(loss, head_params, retain_graph=True)`, `backward(inputs=...)`, an exception between a consumer and the
    hub — must not leave its parts behind for the next pass over the same graph to add again: the first part parked in a pass queues
    an end-of-backward callback on the engine that drops whatever the hub's node did not take."""

    def __init__(self):
        self.parts = []
        self.task = None          # the engine's id of the backward pass the parked parts belong to
        self._cb_queued = False

    def _enter(self):
        """parts of another pass (one that raised before its end-of-backward callbacks ran) are dropped on first touch"""
        task = torch._C._current_graph_task_id()
        if task != self.task:
            self.parts, self.task, self._cb_queued = [], task, False

    def park(self, dx):
        self._enter()
        if not self._cb_queued:
            self._cb_queued = True
            torch.autograd.Variable._execution_engine.queue_callback(self._end_of_backward)
        self.parts.append(dx)

    def take(self):
        self._enter()
        parts, self.parts = self.parts, []
        return parts

    def _end_of_backward(self):
        self._cb_queued = False
        self.parts, self.task = [], None


class XHubFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, hub):
        ctx.hub = hub
        ctx.set_materialize_grads(False)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        parts = ctx.hub.take()
        if g is not None:
            parts.append(g)
        return (ops.sum_tensors(parts) if parts else None), None


def x_hub(x):
    """An alias of the feature map x whose gradient is summed in ONE pass.  x feeds six differentiable ops per training step (a gather
    and a decode per stage); autograd would add their [B, C, H, W] gradients pair by pair — five passes of two reads and one write
    (430 us of a 6.5 ms step at 4 frames).  `mask_gather` / `mask_decode` recognise the alias (its `_vkn_hub`), park their dx in the
    hub and hand autograd nothing; the hub's node — which the engine runs after every consumer, being their common ancestor — adds
    all parts once (vkn_sum_n_f32) and passes the sum on to x.  Anything else that consumes the alias gets ordinary autograd (its
    gradient arrives at the hub as `g` and joins the parts)."""
    hub = _XHub()
    xh = XHubFn.apply(x, hub)
    xh._vkn_hub = hub
    return xh


class MaskGatherFn(torch.autograd.Function):
    """(xraw, cnt) = gather(x, bit(mask_logits)); backward: dx = bit^T dxraw."""

    @staticmethod
    def forward(ctx, x, mask_logits, hard_mask_thr, hub=None):
        xraw, cnt = ops.mask_gather(x, mask_logits, hard_mask_thr)       # (fp16 / bf16 x: the half-storage kernel, VKN_FLAG_X_F16 / _BF16)
        ctx.hub = hub
        ctx.need_dx = x.requires_grad
        ctx.x_dtype = x.dtype
        if ctx.need_dx:
            # backward needs nothing but bit(z >= thr) as the decode kernel's feature rows.  With H*W % 64 == 0 they are written HERE,
            # once, as the fp16 {0, 1} rows that kernel reads (rows padded to its 32-row contraction step; exact, low half zero, so
            # they travel as a half-storage map): no bool tensor, no conversion pass in backward.  Else: one byte per logit.
            B, N, H, W = mask_logits.shape
            ctx.n = N
            if (H * W) % 64 == 0 and mask_logits.dtype == torch.float32:
                ctx.save_for_backward(ops.threshold_rows_f16(mask_logits, hard_mask_thr))
            else:
                ctx.save_for_backward(mask_logits >= ops.thr_logit(hard_mask_thr))
        ctx.mark_non_differentiable(cnt)
        return xraw, cnt

    @staticmethod
    def backward(ctx, dxraw, _dcnt):
        if not ctx.need_dx:
            return None, None, None, None
        (rows,) = ctx.saved_tensors
        N = ctx.n
        Np = (N + 31) // 32 * 32
        if rows.dtype == torch.bool:                                    # [B, N, H, W] bool: the general path
            B, _, H, W = rows.shape
            bits, rows = rows, torch.empty((B, Np, H, W), dtype=torch.float32, device=rows.device)
            rows[:, :N] = bits
            if Np != N:
                rows[:, N:].zero_()
        # dx = bit^T dxraw: the decode kernel with the bit rows as its feature map and the (power-of-two scaled, transposed, padded)
        # gradient as its kernels — scale, transpose and pad in one launch each (vkn_pow2_scale_f32, vkn_transpose_pad_f32); the
        # 1 / s is applied inside the decode kernel.  Half-storage x: the gradient leaves in x's storage type (autograd's
        # contract), rounded once from the fp32 result
        s8 = ops.pow2_scale(dxraw)
        kt = ops.transpose_pad(dxraw, ops.scale_of(s8), Np)             # [B, C, Np]
        dx = _decode_unscaled(rows, kt, ops.inv_of(s8))
        dx = dx if ctx.x_dtype == torch.float32 else dx.to(ctx.x_dtype)
        if ctx.hub is not None:           # (x_hub: the contribution is summed with the others in one pass)
            ctx.hub.park(dx)
            dx = None
        return dx, None, None, None


class SoftMaskGatherFn(torch.autograd.Function):
    """xraw = w x^T with the SOFT weights w = [z >= thr] sigmoid(z) (`use_binary=False`, knet/det/kernel_head.py:243-249): differentiable
    w.r.t. x and — unlike the binarised gather — w.r.t. the mask logits z.  Forward: the real-operand gather kernel; backward: two
    decode-shaped launches, dx = w^T dxraw and dz = [z >= thr] sigmoid'(z) (dxraw x)."""

    @staticmethod
    def forward(ctx, x, mask_logits, hard_mask_thr):
        on = mask_logits >= ops.thr_logit(hard_mask_thr)
        w = torch.sigmoid(mask_logits) * on
        xraw, _ = ops.mask_gather_real(x, w)
        ctx.save_for_backward(x, mask_logits)
        ctx.thr = hard_mask_thr
        return xraw

    @staticmethod
    def backward(ctx, dxraw):
        x, z = ctx.saved_tensors
        B, N, H, W = z.shape
        sg = torch.sigmoid(z)
        on = z >= ops.thr_logit(ctx.thr)
        s = _pow2_scale(dxraw)
        inv = 1.0 / s
        dxs = (dxraw * s).contiguous()                                    # [B, N, C]
        dx = dz = None
        if ctx.needs_input_grad[0]:
            Np = (N + 31) // 32 * 32
            rows = torch.zeros((B, Np, H, W), dtype=torch.float32, device=z.device)
            rows[:, :N] = sg * on
            dx = _decode_unscaled(rows, _pad_last(dxs.transpose(1, 2), Np), inv)           # [B, C, H, W]
        if ctx.needs_input_grad[1]:
            dz = _decode_unscaled(x, dxs, inv) * (sg * (1.0 - sg)) * on                    # [B, N, H, W]
        return dx, dz, None


class MaskDecodeFn(torch.autograd.Function):
    """Z = decode(x, K, kb); backward: dK = dZ x^T, dkb = sum_p dZ, dx = K^T dZ."""

    @staticmethod
    def forward(ctx, x, kernels, bias, hub=None):
        out = ops.mask_decode(x, kernels, bias)
        ctx.save_for_backward(x, kernels)
        ctx.has_bias = bias is not None
        ctx.hub = hub
        return out

    @staticmethod
    def backward(ctx, dz):
        x, kernels = ctx.saved_tensors
        dz = dz.contiguous()
        s8 = ops.pow2_scale(dz)                                           # one launch (vkn_pow2_scale_f32)
        sc, inv = ops.scale_of(s8), ops.inv_of(s8)
        need_k = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        N = dz.shape[1]
        dk = dkb = dx = None
        xdt = x.dtype
        if need_k and xdt != torch.float32:
            # half-storage x: dK = dZ x^T runs on the real-operand gather kernel, which reads fp32 features — x widened once (exact);
            # the FORWARD passes are the half-storage kernels (bit-identical to the fp32 ones on the rounded x)
            x = x.float()
        # dzs = dz * s with the rows zero-padded to the 32-row contraction step: one pass (vkn_scale_pad_rows_f32)
        dzs = ops.scale_pad_rows(dz, sc)
        if ctx.needs_input_grad[0]:
            # dx[b, c, p] = sum_n K[b, n, c] dz[b, n, p]: the decode kernel with dzs as its feature map and K^T (padded) as its kernels
            kT = ops.transpose_pad(kernels.reshape(kernels.shape[0], N, -1), None, dzs.shape[1])
            dx = _decode_unscaled(dzs, kT, inv)
            if xdt != torch.float32:
                dx = dx.to(xdt)
        if need_k:
            # the padded rows are zero, so the gather may run over them too; 1 / s and the slice in one launch
            dk, dkb = ops.unscale_rows(*ops.mask_gather_real(x, dzs), inv, N)
        if ctx.hub is not None and dx is not None:
            ctx.hub.park(dx)
            dx = None
        return dx, dk if ctx.needs_input_grad[1] else None, dkb if (ctx.has_bias and ctx.needs_input_grad[2]) else None, None


def mask_gather(x, mask_logits, hard_mask_thr=0.5):
    return MaskGatherFn.apply(x, mask_logits, hard_mask_thr, getattr(x, '_vkn_hub', None))


def mask_decode(x, kernels, bias=None):
    return MaskDecodeFn.apply(x, kernels, bias, getattr(x, '_vkn_hub', None))


def mask_gather_soft(x, mask_logits, hard_mask_thr=0.5):
    return SoftMaskGatherFn.apply(x, mask_logits, hard_mask_thr)


class MaskLossesFn(torch.autograd.Function):
    """(loss_mask, loss_dice, loss_rank | 0) of one training stage from the up-scaled mask logits: two HIP passes forward, one
    backward that writes the gradient of all three into one tensor (csrc/vkn_loss.hip).  Values: those of CrossEntropyLoss(
    use_sigmoid=True), DiceLoss(use_sigmoid, activate) and CrossEntropyLoss over the kernel axis with the masked-max rank target
    (`KernelUpdateHead.loss`); the mask targets carry no gradient."""

    @staticmethod
    def forward(ctx, mask_pred, mask_targets, pos_rows, B, w_mask, w_dice, dice_eps, w_rank):
        R, P = mask_pred.shape[0] * mask_pred.shape[1], mask_pred.shape[2] * mask_pred.shape[3]
        pred = mask_pred.reshape(R, P)
        target = mask_targets.reshape(R, P)
        K = int(pos_rows.shape[0])
        dev = pred.device
        rowk = torch.full((R,), -1, dtype=torch.int32, device=dev)
        rowk[pos_rows] = torch.arange(K, dtype=torch.int32, device=dev)
        with_rank = w_rank is not None
        stats, lse, top, rank_sum = ops.mask_losses_fwd(pred, target, pos_rows, rowk, B, with_rank)
        bce, a, b, c = stats.unbind(1)
        bc = (b + dice_eps) + (c + dice_eps)
        loss_mask = w_mask * (bce.sum() / (K * P))
        loss_dice = w_dice * (1.0 - (2.0 * a) / bc).mean()
        loss_rank = (w_rank * (rank_sum / (B * P))) if with_rank else pred.new_zeros(())
        ctx.save_for_backward(pred, target, rowk, a, bc, lse if with_rank else pred.new_empty(0), top if with_rank else rowk.new_empty(0))
        ctx.meta = (B, K, P, w_mask, w_dice, w_rank, tuple(mask_pred.shape))
        return loss_mask, loss_dice, loss_rank

    @staticmethod
    def backward(ctx, g_mask, g_dice, g_rank):
        pred, target, rowk, a, bc, lse, top = ctx.saved_tensors
        B, K, P, w_mask, w_dice, w_rank, shape = ctx.meta
        with_rank = w_rank is not None
        gd = g_dice * (w_dice / K)
        rowcoef = torch.stack([gd * (-2.0 / bc), gd * (4.0 * a / (bc * bc))], dim=1).contiguous()
        coef = torch.stack([g_mask * (w_mask / (K * P)), (g_rank * (w_rank / (B * P))) if with_rank else g_mask * 0.0]).float().contiguous()
        grad = ops.mask_losses_bwd(pred, target, rowk, rowcoef.float(), coef, lse, top, B, with_rank)
        return grad.reshape(shape), None, None, None, None, None, None, None


def mask_losses(mask_pred, mask_targets, pos_rows, w_mask, w_dice, dice_eps, w_rank=None):
    """mask_pred [B, Ns, H, W] logits, mask_targets [B*Ns, H, W], pos_rows int64 [K > 0] ascending -> (loss_mask, loss_dice, loss_rank)."""
    return MaskLossesFn.apply(mask_pred.contiguous(), mask_targets.contiguous(), pos_rows, mask_pred.shape[0], w_mask, w_dice, dice_eps, w_rank)


class TrackLossFn(torch.autograd.Function):
    """(loss_track, loss_track_aux) of the quasi-dense embed head from the embeddings of ALL rows and the assigner's `gt_inds`: one
    HIP launch sequence forward, one backward (csrc/vkn_trackloss.hip) — no gather, no `nonzero`, no host synchronisation.  The upstream
    gradients travel as one device [2] tensor; `key_gt`, `ref_gt`, `match`, `match_off` carry no gradient."""

    @staticmethod
    def forward(ctx, key_embeds, ref_embeds, key_gt, ref_gt, match, match_off, cfg):
        key_embeds, ref_embeds = key_embeds.contiguous(), ref_embeds.contiguous()
        losses, _, _, state = ops.track_loss_fwd(cfg, key_embeds, ref_embeds, key_gt, ref_gt, match, match_off)
        ctx.save_for_backward(key_embeds, ref_embeds, state)
        ctx.cfg = cfg
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_track, g_aux):
        key_embeds, ref_embeds, state = ctx.saved_tensors
        gout = torch.stack([g_track.reshape(()), g_aux.reshape(())]).float()
        d_key, d_ref = ops.track_loss_bwd(ctx.cfg, key_embeds, ref_embeds, state, gout)
        return d_key, d_ref, None, None, None, None, None


def track_loss(key_embeds, ref_embeds, key_gt, ref_gt, match, match_off, cfg):
    """key_embeds, ref_embeds [B,N,E]; key_gt, ref_gt int64 [B,N]; match int64 [n], match_off int64 [B+1]; cfg `ops.track_loss_cfg`
    -> (loss_track, loss_track_aux) 0-d tensors (include/vkn_track_train.h)."""
    return TrackLossFn.apply(key_embeds, ref_embeds, key_gt, ref_gt, match, match_off, cfg)


class UpsampleBilinearFn(torch.autograd.Function):
    """`F.interpolate(x, scale_factor=S, mode='bilinear', align_corners=False)` on the HIP kernels, forward and adjoint."""

    @staticmethod
    def forward(ctx, masks, scale):
        ctx.scale = int(scale)
        return ops.upsample_bilinear(masks, ctx.scale)

    @staticmethod
    def backward(ctx, grad_out):
        return ops.upsample_bilinear_bwd(grad_out.contiguous(), ctx.scale), None


def upsample_bilinear(masks, scale):
    return UpsampleBilinearFn.apply(masks, scale)


class FocalLossFn(torch.autograd.Function):
    """`loss_weight * sum(focal(z, labels) * row_weight) / avg_factor` with the element losses and their derivative from ONE HIP
    pass (vkn_focal_loss_f32) instead of ~20 element-wise launches forward and ~30 backward."""

    @staticmethod
    def forward(ctx, logits, labels, row_weight, scale, alpha, gamma):
        total, grad = ops.focal_loss_fwd(logits, labels, row_weight, alpha, gamma)
        ctx.save_for_backward(grad, scale)
        return total * scale

    @staticmethod
    def backward(ctx, g):
        grad, scale = ctx.saved_tensors
        return grad * (g * scale), None, None, None, None, None


def focal_loss(logits, labels, row_weight, loss_weight, avg_factor, alpha, gamma):
    """mmdet `FocalLoss(use_sigmoid=True, reduction='mean')` with an `avg_factor`: sum / avg_factor * loss_weight.  `avg_factor` may be
    a device tensor (no synchronisation)."""
    if torch.is_tensor(avg_factor):
        scale = (loss_weight / avg_factor.detach().to(device=logits.device, dtype=torch.float32)).reshape(())
    else:
        scale = torch.full((), float(loss_weight) / float(avg_factor), dtype=torch.float32, device=logits.device)
    return FocalLossFn.apply(logits, labels, row_weight, scale, alpha, gamma)


class LazyUpsampleFn(torch.autograd.Function):
    """`values` ARE upsample_bilinear(x, stride) (computed without a graph); backward = the upsample's adjoint.  Lets a consumer that
    differentiates w.r.t. x itself (the low-res loss tail) use the values while any other consumer of the returned tensor still
    back-propagates to x."""

    @staticmethod
    def forward(ctx, x, values, stride):
        ctx.stride = stride
        ctx.set_materialize_grads(False)
        return values.view_as(values)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        return ops.upsample_bilinear_bwd(g.contiguous(), ctx.stride), None, None


def lazy_upsample(x, values, stride):
    out = LazyUpsampleFn.apply(x, values, stride)
    out._vkn_lowres = x          # (kernel_iter_head._train_stages: these values belong to exactly this low-res tensor)
    return out


class SegLossFn(torch.autograd.Function):
    """`loss_rpn_seg` of the kernel-initialisation head from the LOW-RES semantic logits and the one-byte target map (include/
    vkn_seg_loss.h): two launches forward, one backward (csrc/vkn_segloss.hip); neither the up-scaled logits nor their gradient exist.
    The upstream gradient travels as a device scalar, nothing reads the host: capturable.  `tgt` and `dense_pos` carry no gradient."""

    @staticmethod
    def forward(ctx, low, tgt, dense_pos, mode, stride, alpha, gamma, loss_weight):
        low = low.contiguous()
        loss, state = ops.seg_loss_fwd(low, tgt, dense_pos, mode, stride, alpha, gamma, loss_weight)
        ctx.save_for_backward(low, tgt, state)
        ctx.args = (mode, stride, alpha, gamma)
        return loss

    @staticmethod
    def backward(ctx, g):
        low, tgt, state = ctx.saved_tensors
        mode, stride, alpha, gamma = ctx.args
        return ops.seg_loss_bwd(low, tgt, g.reshape(1).float(), state, mode, stride, alpha, gamma), None, None, None, None, None, None, None


def seg_loss(low, tgt, dense_pos, mode, stride, alpha=0.25, gamma=2.0, loss_weight=1.0):
    """low fp32 [B,ncls,h,w]; tgt uint8 [B,S h,S w] and dense_pos int32 [1] of `ops.seg_targets`; mode `ops.SEG_LOSS_FOCAL` / `_CE`
    -> the loss as a 0-d tensor."""
    return SegLossFn.apply(low, tgt, dense_pos, mode, stride, alpha, gamma, loss_weight)


class ConvGNReLUFn(torch.autograd.Function):
    """One mmcv `ConvModule`, y = ReLU(GN(conv(x))) with a k x k conv (k = weight.shape[-1], padding k // 2, no bias), forward and
    backward on the library's kernels (include/vkn_fpn_train.h) from a materialised fp32 input.  Forward: `vkn_conv_gn_f32` in its
    raw-input mode, then the GroupNorm + ReLU pass; x, the raw conv output and its statistics are saved.  Backward: the GroupNorm +
    ReLU backward, the weight gradient, and — only when x needs one — the input gradient.  A non-finite gradient is reported through
    `ops.workspace_status`."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, groups, stride):
        x = x.contiguous()
        Cout, _, k, _ = weight.shape
        r, stats = ops.conv_gn(x, ops.conv_prepare(weight), Cout, k, stride, groups)
        ctx.save_for_backward(x, weight, gamma, beta, r, stats)
        ctx.stride = stride
        ctx.ws_cache = ops.workspace_cache()      # the backward reports into the status word of the thread that ran the forward
        return ops.gn_relu_apply(r, stats, gamma, beta)

    @staticmethod
    def backward(ctx, dy):
        x, weight, gamma, beta, r, stats = ctx.saved_tensors
        k, stride = weight.shape[-1], ctx.stride
        with ops.adopt_workspace(ctx.ws_cache):
            dr, dgamma, dbeta = ops.gn_relu_bwd(dy.contiguous(), r, stats, gamma, beta)
            dw = ops.conv_wgrad(dr, x, k, stride) if ctx.needs_input_grad[1] else None
            dx = None
            if ctx.needs_input_grad[0]:
                image_t = ops.conv_prepare(weight.detach().flip(2, 3).transpose(0, 1).contiguous())
                dx = ops.conv_dgrad(dr, image_t, x.shape[1], x.shape[2], x.shape[3], k, stride)
        return dx, dw, dgamma if ctx.needs_input_grad[2] else None, dbeta if ctx.needs_input_grad[3] else None, None, None


def conv_gn_relu(x, weight, gamma, beta, groups, stride=1):
    return ConvGNReLUFn.apply(x, weight, gamma, beta, groups, stride)


class MSDASampleFn(torch.autograd.Function):
    """The sampling core of multi-scale deformable attention, forward (`vkn_msda_sample_f32`, include/vkn_msda.h) and backward
    (`vkn_msda_sample_bwd_f32`, include/vkn_msda_train.h) on the library's kernels.  The RAW offsets and logits go in: the softmax and
    its backward are inside the kernels.  Only the operands are saved; the backward recomputes the forward's points.  No float atomics:
    two backward passes give the same bits.  `ref` and the shapes get no gradient.  A non-finite gradient is reported through
    `ops.workspace_status`."""

    @staticmethod
    def forward(ctx, value, offsets, logits, ref, spatial_shapes, num_heads, num_points):
        value = value.contiguous()
        ctx.save_for_backward(value, offsets, logits, ref)
        ctx.cfg = (tuple((int(h), int(w)) for h, w in spatial_shapes), int(num_heads), int(num_points))
        ctx.ws_cache = ops.workspace_cache()      # the backward reports into the status word of the thread that ran the forward
        return ops.msda_sample(value, ctx.cfg[0], offsets, logits, ref, ctx.cfg[1], ctx.cfg[2])

    @staticmethod
    def backward(ctx, dout):
        value, offsets, logits, ref = ctx.saved_tensors
        shapes, M, P = ctx.cfg
        with ops.adopt_workspace(ctx.ws_cache):
            dvalue, doff, dlogits = ops.msda_sample_bwd(value, shapes, offsets, logits, ref, dout.contiguous(), M, P)
        need = ctx.needs_input_grad
        return dvalue if need[0] else None, doff if need[1] else None, dlogits if need[2] else None, None, None, None, None


def msda_sample(value, spatial_shapes, offsets, logits, ref, num_heads, num_points):
    """value [B, S, M D]; offsets [B Q, 2 M L P] and logits [B Q, M L P], the raw outputs of the `sampling_offsets` /
    `attention_weights` Linears (column ranges of one GEMM output are taken as they are); ref [Q, L, 2] -> [B, Q, M D], differentiable
    in value, offsets and logits."""
    return MSDASampleFn.apply(value, offsets, logits, ref, spatial_shapes, num_heads, num_points)


class SwinWindowAttnFn(torch.autograd.Function):
    """The (shifted-)window attention core of a Swin block, forward (`vkn_swin_window_attn_f32`, include/vkn_swin.h) and backward
    (`vkn_wattn_bwd_f32`, include/vkn_wattn_train.h) on the library's kernels.  Only the operands are saved: the backward recomputes
    scores and softmax, so no [B nW, heads, N, N] tensor outlives the forward.  No float atomics: two backward passes give the same bits.
    The gradient of `qkv_bias` is the part through pad tokens only; the part through real tokens reaches the bias through `qkv`."""

    @staticmethod
    def forward(ctx, qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale):
        qkv = qkv.contiguous()
        ctx.save_for_backward(qkv, qkv_bias, bias_table)
        ctx.cfg = (int(H), int(W), int(heads), int(window), int(shift), float(scale))
        return ops.swin_window_attention(qkv, qkv_bias, bias_table, *ctx.cfg)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        qkv, qkv_bias, bias_table = ctx.saved_tensors
        dqkv, dbias, dtable = ops.swin_window_attention_bwd(qkv, qkv_bias, bias_table, dout.contiguous(), *ctx.cfg)
        need = ctx.needs_input_grad
        return (dqkv if need[0] else None, dbias if qkv_bias is not None and need[1] else None, dtable if need[2] else None,
                None, None, None, None, None, None)


def swin_window_attention(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale):
    """qkv [B, H W, 3 heads 32], the rows of the `qkv` Linear on the tokens as they lie; qkv_bias [3 heads 32] or None; bias_table
    [(2 window - 1)^2, heads] -> [B, H W, heads 32], differentiable in all three."""
    return SwinWindowAttnFn.apply(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale)
