/* vkn_fpn_train.h — C ABI of libvkn.so, a training part: the backward of ONE localization-FPN block, mmcv's
 * `ConvModule(Cin, Cout, k, stride, padding = k / 2, norm_cfg = GN(groups), act_cfg = ReLU)`, y = ReLU(GN(conv(x)))
 * (knet/det/semantic_fpn_wrapper.py:83-146), whose forward is vkn_conv_gn_f32 of vkn.h.
 *
 * Conventions and error codes are those of vkn.h: `extern "C"`, DEVICE pointers into caller-owned contiguous fp32 memory, 16-byte
 * aligned, nothing allocated inside, work enqueued asynchronously on `stream`, no host synchronisation, 0 = VKN_OK.  Every entry
 * refuses before any launch, in this order: NULL pointers / counts <= 0 -> VKN_E_ARG, a shape outside the envelope -> VKN_E_SHAPE,
 * a workspace that is NULL or smaller than its `*_workspace_bytes` -> VKN_E_WORKSPACE, a misaligned pointer -> VKN_E_ALIGN.
 * A workspace starts with the 256-byte status header of vkn.h (vkn_workspace_status reads and clears it); the entries only OR into it.
 * No float atomics: every sum has a fixed order, two runs on the same inputs are bitwise equal.
 *
 * Envelope (the forward block's): Cin, Cout (C) multiples of 32 and <= 512, groups divides Cout, H, W >= 1, k = 3 with stride 1 or 2
 * (padding 1) or k = 1 with stride 1, Ho = ceil(H / stride), B * C * H * W * 4 < 2^31 for every tensor.
 *
 * Operand range of the two MFMA entries (vkn_conv_wgrad_f32, vkn_conv_dgrad_f32): the two-term f16 split of vkn.h, but NO operand is
 * staged unscaled.  Gradient maps are routinely 1e-4 .. 1e-7, where an unscaled split has no bits left (absolute resolution 2^-24):
 * each call measures max |v| of `dr` (and of `x` in the weight gradient) and stages v * 2^e with max |v| 2^e in [2^14, 2^15); the
 * epilogue multiplies by the inverse powers (exact).  The resolution is therefore 2^-22 relative for operands within about 2^-17 of
 * the tensor's largest magnitude and 2^-39 of that magnitude below.  A non-finite staged value ORs VKN_STATUS_RANGE into the status
 * word, and so does a non-finite `dy` in vkn_gn_relu_bwd_f32: the outputs are then garbage, never a silent result. */
#ifndef VKN_FPN_TRAIN_H
#define VKN_FPN_TRAIN_H
#include "vkn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_FPN_BWD_RUN_PX 2048       /* pixels of one (frame, channel) that one workgroup of the GroupNorm backward sums */
#define VKN_FPN_WGRAD_MAX_SPLITS 64   /* the most partial [Cout][Cin k^2] tiles the weight gradient splits its pixel runs into */
#define VKN_FPN_WGRAD_TARGET_WGS 256  /* splits = clamp(TARGET_WGS / ((Cin / 32) ceil(Cout / 128)), 1, min(MAX_SPLITS, runs)) */

/* ---- y = relu(gamma (r - mean) rstd + beta): the block's output from the RAW conv output r [B][C][H][W] and the
 *      stats [B][groups][2] = (mean, rstd) that vkn_conv_gn_f32 wrote (out, out_stats); gamma, beta [C].  y [B][C][H][W], may be r.
 *      One launch, no workspace. */
int vkn_gn_relu_apply_f32(const float* r, const float* stats, const float* gamma, const float* beta, int groups, float* y, int B, int C,
                          int H, int W, void* stream);

/* ---- backward of that: from dy [B][C][H][W] (the gradient of y), r, stats, gamma, beta
 *        xhat = (r - mean) rstd,  mask = gamma xhat + beta > 0 (recomputed, the forward's own expression),  dz = dy mask,
 *        dgamma[c] = sum_{b, p} dz xhat,  dbeta[c] = sum_{b, p} dz,  g = dz gamma,
 *        dr = rstd (g - mean_grp(g) - xhat mean_grp(g xhat)),  the means over the (frame, group)'s C / groups * H * W elements.
 *      dr [B][C][H][W] (may be dy), dgamma, dbeta [C].  Three launches: fp32 sums per (frame, channel, run of VKN_FPN_BWD_RUN_PX pixels)
 *      reduced per workgroup in fp64; a fixed-order fp64 merge into the group means, dgamma and dbeta; the elementwise pass. */
size_t vkn_gn_relu_bwd_workspace_bytes(int B, int C, int H, int W, int groups);
int vkn_gn_relu_bwd_f32(const float* dy, const float* r, const float* stats, const float* gamma, const float* beta, int groups, float* dr,
                        float* dgamma, float* dbeta, int B, int C, int H, int W, void* ws, size_t ws_bytes, void* stream);

/* ---- weight gradient dw[co][ci][ky][kx] = sum_{b, y, x} dr[b][co][y][x] x[b][ci][y s + ky - p][x s + kx - p] (zero outside x),
 *      dr [B][Cout][Ho][Wo], x [B][Cin][H][W] (the conv's input as the forward saw it: with the positional map added, if any),
 *      dw [Cout][Cin][k][k].  A GEMM over B Ho Wo on MFMA: the 64-pixel runs of the output rows are dealt to `splits` workgroups per
 *      (32 input channels, 128 output channels), each writing a partial tile; a second launch adds the partials in split order in fp64.
 *      Five launches (two per operand's power of two, the GEMM, the sum). */
size_t vkn_conv_wgrad_workspace_bytes(int B, int Cin, int H, int W, int Cout, int ksize, int stride);
int vkn_conv_wgrad_f32(const float* dr, const float* x, float* dw, int B, int Cin, int H, int W, int Cout, int ksize, int stride, void* ws,
                       size_t ws_bytes, void* stream);

/* ---- input gradient dx[b][ci][iy][ix] = sum_{co, ky, kx} dr[b][co][(iy + p - ky) / s][(ix + p - kx) / s] w[co][ci][ky][kx] over
 *      the taps whose two quotients are whole and inside dr: a gather per input pixel, no atomics.  With stride 2 a workgroup takes
 *      64 input pixels of ONE column parity of a row, so the taps that reach them are the same for all of its lanes.
 *      wimg_t: the vkn_conv_prepare_f32 image of the FLIPPED, CHANNEL-TRANSPOSED weight wt[ci][co][ky][kx] = w[co][ci][k-1-ky][k-1-kx]
 *      (vkn_conv_weight_bytes(Cin, Cout, k) bytes), which makes it the forward's A operand.  dx [B][Cin][H][W], every element written.
 *      Three launches. */
size_t vkn_conv_dgrad_workspace_bytes(int B, int Cout, int H, int W, int stride);
int vkn_conv_dgrad_f32(const float* dr, const void* wimg_t, float* dx, int B, int Cin, int H, int W, int Cout, int ksize, int stride,
                       void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_FPN_TRAIN_H */
