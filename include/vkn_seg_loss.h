/* vkn_seg_loss.h — C ABI of libvkn.so, an extension part: the dense semantic loss of the kernel-initialisation head, computed from the
 * LOW-RES semantic logits.
 *
 * Conventions, error codes and the status word are those of vkn.h: `extern "C"`, DEVICE pointers into caller-owned contiguous memory
 * (the one HOST array is marked), nothing allocated inside, work enqueued asynchronously on `stream`, no host synchronisation,
 * 0 = VKN_OK.  Every entry refuses before any launch, in this order: NULL pointers / negative counts -> VKN_E_ARG, a shape outside the
 * envelope -> VKN_E_SHAPE, a misaligned pointer -> VKN_E_ALIGN, a host pointer where device memory is expected -> VKN_E_ARG (last: it
 * is the only check that asks the runtime).
 *
 * What it replaces: `loss_rpn_seg` of `ConvKernelHead.forward_train` / `.loss` (knet/det/kernel_head.py:278-292, 404-426) with the
 * `seg_targets` of `_get_target_single` (:446-462).  There the semantic logits [B, ncls, h, w] are up-scaled by
 * `feat_downsample_stride` (F.interpolate, bilinear, align_corners=False), permuted into a contiguous [B S h S w, ncls] copy and handed
 * to the loss; here the up-scaled logits exist in registers only.
 *
 * The arithmetic: up-scaled pixel d of a row reads the source (d + 0.5) / S - 0.5, clamped at the borders.  For an even S the S x S
 * block of pixels that starts at S i + S / 2 lies between the low-res rows i, i + 1 (columns alike) with the weights (a + 0.5) / S,
 * a = 0 .. S - 1: compile-time constants, exact in fp32.  S = 1 is the identity.
 */
#ifndef VKN_SEG_LOSS_H
#define VKN_SEG_LOSS_H
#include "vkn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_SEG_LOSS_FOCAL 0    /* mmdet's sigmoid focal loss, avg_factor = max(dense_pos, 1)  (:404-418) */
#define VKN_SEG_LOSS_CE 1       /* soft-max cross entropy, ignore_index = ncls, mean over ALL pixels  (:420-426) */
#define VKN_SEG_MAX_IMAGES 64   /* images per call */
#define VKN_SEG_MAX_CLASSES 255 /* semantic classes: the target map is one byte per pixel and `ncls` itself means background / ignore */
#define VKN_SEG_MAX_ROWS 65535  /* proposals (Np) and ground-truth instances (G) per image */

/* One image of the batch (a HOST array of these, as VknGtImage is used).
 *   masks    fp32 [G][H][W]: the instance masks at the up-scaled size; a pixel is covered where the value != 0; may be NULL when G == 0;
 *   sem      fp32 [n_sem][H][W]: the stuff masks, same rule; NULL (or n_sem == 0): the image has no stuff layer;
 *   labels   int64 [G]: the label of every instance;        sem_cls int64 [n_sem]: the label of every stuff mask;
 *   gt_inds  int64 [Np]: the assigner's `gt_inds` (0 = unmatched, k = ground truth k - 1); may be NULL when Np == 0. */
typedef struct VknSegImage {
    const float* masks;
    const float* sem;
    const int64_t* labels;
    const int64_t* sem_cls;
    const int64_t* gt_inds;
    int G, n_sem, Np;
} VknSegImage;
size_t vkn_sizeof_seg_image(void);

/* ---- the painted target map (a clear + 1 launch): `seg_targets` of `_get_target_single` (knet/det/kernel_head.py:446-462), per pixel:
 *      t = ncls; for j = 0 .. n_sem - 1: sem[j][p] != 0 -> t = sem_cls[j]; then for n = 0 .. Np - 1 with gt_inds[n] > 0, g = gt_inds[n] - 1:
 *      masks[g][p] != 0 -> t = labels[g].  The last layer that covers a pixel wins (the kernel walks the layers from the last one down
 *      and stops at the first that covers).  `pos_inds` of MaskPseudoSampler are the non-zero positions of gt_inds, ascending: no
 *      `nonzero`, no gather, no host read.
 *      in : imgs HOST [B]; H, W: the up-scaled size; ncls;
 *      out: tgt uint8 [B][H][W]; dense_pos int32 [1] = #{t < ncls} over the batch (cleared by the call; integer atomics, one per
 *           workgroup: exact in any order);
 *           status: VKN_STATUS_RANGE is ORed into it when a label of a painted layer lies outside [0, ncls) — that layer paints ncls —
 *           or when a gt_inds entry exceeds G — that row paints nothing, nothing is read out of bounds.
 *      Envelope: 1 <= B <= VKN_SEG_MAX_IMAGES, 1 <= ncls <= VKN_SEG_MAX_CLASSES, 1 <= H <= 262140, 1 <= W, H W < 2^31,
 *      0 <= G, Np <= VKN_SEG_MAX_ROWS, 0 <= n_sem <= VKN_SEG_MAX_ROWS; dense_pos, status 4-byte, the mask pointers 4-byte aligned. */
int vkn_seg_targets_u8(const VknSegImage* imgs, int B, int H, int W, int ncls, unsigned char* tgt, int* dense_pos, int* status,
                       void* stream);

/* ---- bytes of the state buffer that vkn_seg_loss_fwd_f32 fills for vkn_seg_loss_bwd_f32 (0 outside the envelope): the scale of the
 *      loss, the fp64 partial sums of the workgroups, and in CE mode the soft-max statistics (max, log-sum) of every up-scaled pixel. */
size_t vkn_seg_loss_state_bytes(int mode, int B, int h, int w, int S);

/* ---- the loss (2 launches): `loss_rpn_seg` (knet/det/kernel_head.py:278-292, 404-426) from low [B][ncls][h][w] fp32, tgt uint8
 *      [B][S h][S w] and, in focal mode, dense_pos int32 [1] (both as vkn_seg_targets_u8 leaves them).
 *      VKN_SEG_LOSS_FOCAL: loss_weight / max(dense_pos, 1) x the sum over all pixels and classes of py_sigmoid_focal_loss with the
 *        one-hot target [t == c] (a pixel with t == ncls is all-negative and counts);
 *      VKN_SEG_LOSS_CE: loss_weight / (B S h S w) x the sum over the pixels with t < ncls of logsumexp_c z_c - z_t (max subtracted);
 *        alpha, gamma and dense_pos are not read.
 *      A thread owns one S x S block; per workgroup one fp64 partial sum, added by one finishing workgroup in a fixed order: two calls
 *      give the same bits.  out: loss fp32 [1]; state: vkn_seg_loss_state_bytes(...) bytes, 16-byte aligned.
 *      Envelope: mode one of the two, S in {1, 2, 4}, 1 <= ncls <= VKN_SEG_MAX_CLASSES, 1 <= B <= VKN_SEG_MAX_IMAGES, 1 <= h, w,
 *      ncls h w 4 < 2^31, h <= 196605 (the backward's grid); low, loss, dense_pos 4-byte aligned. */
int vkn_seg_loss_fwd_f32(const float* low, const unsigned char* tgt, const int* dense_pos, int mode, int B, int ncls, int h, int w, int S,
                         float alpha, float gamma, float loss_weight, float* loss, void* state, void* stream);

/* ---- its backward (1 launch): grad_low [B][ncls][h][w] = gout[0] x d loss / d low, gout fp32 [1] on the device.  The adjoint of the
 *      up-scaling applied to the element derivatives (focal: as vkn_focal_loss_f32; CE: soft-max - one-hot, zero on ignored pixels), in
 *      gather form: every element of grad_low is written exactly once, in a fixed order of additions, without atomics; the up-scaled
 *      gradient is never written (the reference's autograd writes and reads it: knet/det/kernel_head.py:278-292 backwards).
 *      `state` is what the forward left for the same low, tgt and arguments.  Envelope: the forward's. */
int vkn_seg_loss_bwd_f32(const float* low, const unsigned char* tgt, const float* gout, int mode, int B, int ncls, int h, int w, int S,
                         float alpha, float gamma, const void* state, float* grad_low, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_SEG_LOSS_H */
