/* vkn_instmask.h — C ABI of libvkn.so, an instance-result part: instance masks as BITS straight from the head's mask logits (the fused
 * rescale), and the entries of the run-length encoder (vkn_rle.h) and of the mask-overlap meter (vkn_maskap.h) that take such bits.
 *
 * Conventions and error codes are those of vkn.h and vkn_rle.h: `extern "C"`, DEVICE pointers into caller-owned contiguous memory, nothing
 * allocated inside, work enqueued asynchronously on `stream`, no host synchronisation (capturable), 0 = VKN_OK.  Every entry refuses before
 * any launch, in this order: NULL pointers / negative counts -> VKN_E_ARG, a shape outside the envelope -> VKN_E_SHAPE, a `ws_bytes` that
 * is not the size query's value -> VKN_E_WORKSPACE, a misaligned pointer -> VKN_E_ALIGN, a host pointer where device memory is expected ->
 * VKN_E_ARG (last: it is the only check that asks the runtime).
 *
 * What it replaces: `KernelUpdateHead.rescale_masks` followed by `> mask_thr` (knet/det/kernel_update_head.py:443-466), which forms K
 * full-resolution fp32 maps three times over, and the pack pass that turned those maps into bits for the two consumers.  Per mask k:
 *
 *   p = interp( interp( sigmoid( interp_up(logits[rows[k]]) ), size = (Hb, Wb) )[:h, :w], size = (Ho, Wo) )      bit = p > thr
 *
 * `interp` is bilinear, align_corners = False, in fp32 with ATen's coefficients (source = scale * (dst + 0.5) - 0.5 clamped at 0, scale =
 * 1 / up for interp_up and in / out for the two `size =` calls) and ATen's evaluation order: x then y, each as v0 * w0 + v1 * w1 — the
 * rules of vkn_panoptic_joint_f32, from the same two device functions.  interp_up exists for up > 1 only; with up = 1 the logits are the
 * head's scaled_mask_preds, as in the reference.  Every level is evaluated, one that keeps its size too (its second weight is 0: a finite
 * value passes unchanged, a NaN tap spreads, as v0 * 1 + NaN * 0 does).  The comparison is ONE fp32 comparison, torch's `>`: equal to thr
 * gives 0, NaN gives 0.  fp32 rounding differs from torch's own kernels in the last bits of p, so a pixel whose exact p lies within 1e-4 of
 * thr may come out either way; it comes out the same way on every call.
 *
 * Not built: polygon output, a threshold per mask, logits in f16.
 */
#ifndef VKN_INSTMASK_H
#define VKN_INSTMASK_H
#include "vkn.h"
#include "vkn_rle.h"
#include "vkn_maskap.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_INSTMASK_MAX_K 1024         /* masks of one call */
#define VKN_INSTMASK_MAX_SCALED_W 4096  /* Wm * up */
#define VKN_INSTMASK_TILE_ROWS 16       /* output rows of one strip of 64 columns that a workgroup resamples at a time */
#define VKN_INSTMASK_BATCH 4            /* masks that a workgroup walks with one set of coefficient tables */
#define VKN_INSTMASK_LDS_BYTES 65536    /* what the footprints of one tile and its coefficient tables may take */
#define VKN_INSTMASK_WS_BYTES 16        /* the workspace: one status word (uint32) and padding */
/* bits of the workspace's status word: zeroed by the call, then OR-ed in.  Nothing reads it back; the caller may. */
#define VKN_INSTMASK_STATUS_ROW_RANGE 1u    /* an entry of `rows` outside [0, N): its mask has no bit set */
#define VKN_INSTMASK_STATUS_FOOTPRINT 2u    /* a tile's footprint exceeded the staged region (a defect): the tile has no bit set */

/* The geometry of one image.
 *   up        factor of interp_up: 1 (logits are the scaled mask predictions), 2 or 4 (logits are the head's own, stride 8);
 *   Hm, Wm    rows and columns of one logits map;
 *   Hb, Wb    batch_input_shape;   h, w: img_shape, a crop of it (h <= Hb, w <= Wb);   Ho, Wo: ori_shape, the size of the masks. */
typedef struct VknInstMaskCfg {
    int up, Hm, Wm, Hb, Wb, h, w, Ho, Wo, reserved;
} VknInstMaskCfg;
size_t vkn_sizeof_inst_mask_cfg(void);
size_t vkn_sizeof_instmask_cfg(void);    /* the same value under the part's own name */

/* ---- bytes of the workspace of one call: VKN_INSTMASK_WS_BYTES; 0 outside the envelope: up in {1, 2, 4}, every extent >= 1, h <= Hb,
 *      w <= Wb, Wm * up <= VKN_INSTMASK_MAX_SCALED_W, 1 <= K <= VKN_INSTMASK_MAX_K, K * ceil(Wo / 64) * Ho < 2^28, and the footprint of
 *      one 64 x VKN_INSTMASK_TILE_ROWS output tile through every level, with its coefficient tables, within VKN_INSTMASK_LDS_BYTES (an
 *      extreme down-scaling does not fit). */
size_t vkn_instance_bits_workspace_bytes(const VknInstMaskCfg* cfg, int K);

/* ---- logits float [N][Hm][Wm]; rows int32 [K] (device) or NULL = the first K rows (then K <= N); any order, duplicates allowed.
 *      bits: 64-bit words [K][ceil(Wo / 64)][Ho], the layout that vkn_bits_rle_encode and vkn_bits_mask_overlap read: bit c of word
 *      [k][s][y] is pixel (y, 64 * s + c) of mask k; the bits behind Wo are zero.  Every word is written.  One fill of the status word and
 *      one launch; no atomics on the result, nothing read back: two calls on the same input write the same bits.
 *      Outside the envelope of the size query: VKN_E_SHAPE, nothing written.  logits, bits, ws 16-byte aligned, rows 4-byte aligned. */
int vkn_instance_bits_f32(const VknInstMaskCfg* cfg, const float* logits, int N, const int* rows, int K, float thr, long long* bits, void* ws,
                          size_t ws_bytes, void* stream);

/* ---- the run-length encoder on bits: vkn_rle_encode_u8 (vkn_rle.h) without its pack pass, seven launches.  bits [K][ceil(W / 64)][H] as
 *      above (the bits behind W zero); everything else, outputs included, as vkn_rle_encode_u8 on the masks that the bits spell.
 *      The workspace is that encoder's without its largest part.  Envelope: that of vkn_rle_workspace_bytes. */
size_t vkn_bits_rle_workspace_bytes(int K, int H, int W);
int vkn_bits_rle_encode(const long long* bits, int K, int H, int W, int* records, unsigned* runs, int cap_runs, unsigned char* bytes,
                        int cap_bytes, unsigned* status, void* ws, size_t ws_bytes, void* stream);

/* ---- the mask overlap with the detections as bits: vkn_mask_overlap_u8 (vkn_maskap.h) without the detections' pack pass; only the
 *      ground truths (uint8 [G][H][W]) are packed, into the workspace: up16(8 * G * ceil(W / 64) * H) bytes, 0 outside the envelope of
 *      vkn_mask_overlap_workspace_bytes AND for G = 0 (then `ws` may be NULL).  Two launches at most.  Everything else as
 *      vkn_mask_overlap_u8 on the masks that the bits spell. */
size_t vkn_bits_mask_overlap_workspace_bytes(int K, int G, int H, int W);
int vkn_bits_mask_overlap(const long long* dt_bits, const unsigned char* gt, int K, int G, int H, int W, long long* inter, long long* area_dt,
                          long long* area_gt, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_INSTMASK_H */
