/* vkn_msda_train.h — C ABI of libvkn.so, a neck training part: the backward of the sampling core of multi-scale deformable
 * attention, whose forward is vkn_msda_sample_f32 of vkn_msda.h.
 *
 * Conventions and error codes are those of vkn.h: `extern "C"`, DEVICE pointers into caller-owned fp32 memory (the one HOST array is
 * marked), 16-byte aligned, nothing allocated inside, work enqueued asynchronously on `stream`, no host synchronisation, 0 = VKN_OK.
 * The entry refuses before any launch, in this order: NULL pointers / counts <= 0 / a row stride shorter than its row / an empty
 * level -> VKN_E_ARG, a shape outside the envelope -> VKN_E_SHAPE, a workspace that is NULL or smaller than
 * vkn_msda_bwd_workspace_bytes -> VKN_E_WORKSPACE, a misaligned pointer -> VKN_E_ALIGN.  The workspace starts with the 256-byte status
 * header of vkn.h (vkn_workspace_status reads and clears it); the entry only ORs into it.
 * No float atomics: every float sum has a fixed order and the one scatter is an INTEGER sum, so two runs on the same inputs are
 * bitwise equal.
 *
 * Nothing of the forward is saved.  The softmax weights w_i (max-subtracted, i over the L P points of one (b, q, m)), the pixel
 * coordinates, the test y > -1 && x > -1 && y < H_l && x < W_l, the four clamped corners and the bilinear fractions
 * lw = x - floor(x), hw = 1 - lw, lh = y - floor(y), hh = 1 - lh are recomputed by the forward's own code.  With v1 .. v4 the values
 * at the corners (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1) (zero for a corner outside the level), s_i[d] the bilinear
 * sample and G_i = sum_d dout[d] s_i[d]:
 *     dlogits[b,q,m,i]       = w_i (G_i - sum_j w_j G_j)                                  (exactly 0 when L P = 1)
 *     doff[b,q,m,l,p,x]      = w_i sum_d dout[d] (hh (v2 - v1) + lh (v4 - v3))            (d x / d off_x = 1)
 *     doff[b,q,m,l,p,y]      = w_i sum_d dout[d] (hw (v3 - v1) + lw (v4 - v2))
 *     dvalue[b, start_l + y W_l + x, m, d] += dout[d] w_i (corner weight)                 for every corner inside the level
 * A point that fails the four comparisons gets doff = exactly 0 and adds nothing to dvalue (mmcv's backward; F.grid_sample's with all
 * corners outside).  dlogits and doff are gathers: the sums over d run across the lanes of one (b, q, m) in a fixed butterfly order.
 * There is no gradient for `ref`.
 *
 * dvalue is a scatter, built as a FIXED-POINT integer accumulation.  A first pass measures max |dout| and derives, on the device,
 * the largest power of two 2^e with max |dout| 2^e Q P < 2^62: |contribution| <= max |dout| (a softmax weight and a corner weight
 * are both <= 1), and a cell receives at most Q P of them (one per point of its level; the four corners of a point are distinct
 * cells).  Each contribution c is rounded ONCE, llrint(c 2^e), and added with a 64-bit integer atomic into an int64 [B][S][M][D]
 * accumulator in the workspace, which the entry zeroes itself on the stream; a last pass writes dvalue = (float)acc 2^-e.  With
 * Q P <= 2^24 every contribution keeps at least 37 bits below the largest |dout|.  A non-finite dout, or a non-finite contribution
 * (from a NaN logit, say), ORs VKN_STATUS_RANGE into the status word and is never converted to an integer.
 *
 * Safety: as in the forward, the four comparisons come before any float -> int conversion and before any address is formed; a point
 * that fails them forms no address.  No input VALUE (NaN, +-inf, 1e30 offsets) can produce an access outside `value` or the accumulator.
 *
 * Envelope: the forward's (vkn_msda.h), the same 2^31-byte limit for doff and dlogits with their row strides,
 * Q P <= VKN_MSDA_BWD_MAX_QP, and an accumulator of fewer than 2^31 elements (B S M D < 2^31: implied by the forward's limit). */
#ifndef VKN_MSDA_TRAIN_H
#define VKN_MSDA_TRAIN_H
#include "vkn_msda.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_MSDA_BWD_MAX_QP 16777216      /* 2^24: the most contributions one cell of dvalue may receive */
#define VKN_MSDA_BWD_WS_HEAD 1536         /* bytes of the workspace before the accumulator: status header, the power of two, max partials */

/* VKN_MSDA_BWD_WS_HEAD + 8 B S M D rounded up to 256 bytes; 0 outside the envelope.  shapes: HOST array of L pairs (H_l, W_l). */
size_t vkn_msda_bwd_workspace_bytes(const int* shapes, int B, int Q, int M, int D, int L, int P);

/* value, off, ld_off, logits, ld_logits, ref, shapes: the forward's operands, as vkn_msda.h states them;
 * dout    [B][Q][M D], the gradient of the forward's output;
 * dvalue  [B][S][M][D];
 * doff    row (b, q) at doff + (b Q + q) ld_doff, [M][L][P][2];
 * dlogits row (b, q) at dlogits + (b Q + q) ld_dlogits, [M][L P].  ld_doff >= 2 M L P and ld_dlogits >= M L P are row strides in
 *         floats: both gradients may land in ONE [B Q][3 M L P] buffer, the mirror of the forward's one GEMM output.
 * Every element of the three outputs is written (of a strided output: every element of its rows' 2 M L P / M L P columns); nothing
 * outside them is.  Five launches and one memset. */
int vkn_msda_sample_bwd_f32(const float* value, const float* off, int ld_off, const float* logits, int ld_logits, const float* ref,
                            const int* shapes, const float* dout, float* dvalue, float* doff, int ld_doff, float* dlogits,
                            int ld_dlogits, int B, int Q, int M, int D, int L, int P, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_MSDA_TRAIN_H */
