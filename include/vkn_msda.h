/* vkn_msda.h — C ABI of libvkn.so, a neck part: the sampling core of multi-scale deformable attention, the one op of
 * `MSDeformAttnPixelDecoder` (knet/det/msdeformattn_decoder.py) that is neither a dense conv nor a GEMM.
 *
 * Conventions and error codes are those of vkn.h: `extern "C"`, DEVICE pointers into caller-owned fp32 memory (the one HOST array is
 * marked), 16-byte aligned, nothing allocated inside, work enqueued asynchronously on `stream`, no host synchronisation, 0 = VKN_OK.
 * The entry refuses before any launch, in this order: NULL pointers / counts <= 0 / a row stride shorter than its row -> VKN_E_ARG,
 * a shape outside the envelope -> VKN_E_SHAPE, a misaligned pointer -> VKN_E_ALIGN.  No workspace, no atomics: every sum has a fixed
 * order, two runs on the same inputs are bitwise equal.
 *
 * For every batch item b, query q, head m and channel d
 *     w[l,p]   = softmax over the L P raw logits of (b, q, m), max-subtracted
 *     loc[l,p] = ref[q,l,:] + off[b,q,m,l,p,:] / (W_l, H_l)                  (x, y; normalised)
 *     x = loc.x W_l - 0.5,  y = loc.y H_l - 0.5                              (align_corners = False)
 *     sample   = bilinear(value[b, start_l + ., m, :], y, x), zero outside the level
 *     out[b,q,m D + d] = sum_{l,p} w[l,p] sample[d]                          (summed in (l, p) order, divided by the softmax sum last)
 * A point contributes only if y > -1 && x > -1 && y < H_l && x < W_l, and each of its four corners only if it lies inside the level:
 * mmcv's `ms_deform_attn` rule, = F.grid_sample(bilinear, padding_mode='zeros', align_corners=False) on 2 loc - 1.
 *
 * Safety: the four comparisons come before any float -> int conversion and before any address is formed; a point that fails them
 * (a NaN, an infinity, 1e30) reads nothing and adds nothing.  No input VALUE can produce an out-of-range load.
 *
 * Envelope: D in {16, 32, 64}, M D a multiple of 32 and <= 256, 1 <= L <= VKN_MSDA_MAX_LEVELS, 1 <= P <= VKN_MSDA_MAX_POINTS,
 * B S M D 4 < 2^31 with S = sum_l H_l W_l, and the same limit for out, off and logits with their row strides. */
#ifndef VKN_MSDA_H
#define VKN_MSDA_H
#include "vkn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_MSDA_MAX_LEVELS 4
#define VKN_MSDA_MAX_POINTS 8
#define VKN_MSDA_MAX_CHANNELS 256     /* M D */

/* value  [B][S][M][D], the levels concatenated in the order of `shapes`;
 * off    row (b, q) at off + (b Q + q) ld_off, [M][L][P][2] (x, y) in pixels of the level: the raw output of `sampling_offsets`;
 * logits row (b, q) at logits + (b Q + q) ld_logits, [M][L P]: the raw output of `attention_weights`.  ld_off >= 2 M L P and
 *        ld_logits >= M L P are row strides in floats: both may point into ONE [B Q][3 M L P] GEMM output;
 * ref    [Q][L][2] (x, y) normalised reference points, shared by the batch;
 * shapes HOST array of L pairs (H_l, W_l), read before the call returns;
 * out    [B][Q][M D], every element written.  One launch. */
int vkn_msda_sample_f32(const float* value, const float* off, int ld_off, const float* logits, int ld_logits, const float* ref,
                        const int* shapes, float* out, int B, int Q, int M, int D, int L, int P, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_MSDA_H */
