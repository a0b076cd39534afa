/* vkn_rle.h — C ABI of libvkn.so, a result part: COCO run-length encoding (RLE) of instance masks on the device.
 *
 * Conventions and error codes are those of vkn.h: `extern "C"`, DEVICE pointers into caller-owned contiguous memory, nothing allocated
 * inside, work enqueued asynchronously on `stream`, no host synchronisation (capturable), 0 = VKN_OK.  Every entry refuses before any
 * launch, in this order: NULL pointers / negative counts -> VKN_E_ARG, a shape outside the envelope -> VKN_E_SHAPE, a `ws_bytes` that is
 * not vkn_rle_workspace_bytes(K, H, W) -> VKN_E_WORKSPACE, a misaligned pointer -> VKN_E_ALIGN, a host pointer where device memory is
 * expected -> VKN_E_ARG (last: it is the only check that asks the runtime).
 *
 * What it replaces: `encode_mask_results` in the reference's test loops (external/test.py:55-70, tools_vis/apis/test.py:36,80, and
 * behind mmtrack/transform.py:outs2results for YouTube-VIS), which runs pycocotools' encoder mask by mask on the host over the K
 * full-resolution boolean arrays that `segm2result` copied there.  pycocotools is not part of the reference tree
 * (external/ext/mask.py:3 only imports it; its comment at external/ext/mask.py:10-15 documents the format with two examples), so the
 * format is RESTATED here:
 *
 *   Run list.  For one mask [H][W], walk the pixels in COLUMN-MAJOR order, p = x * H + y, starting from "previous value" 0.  `counts` is
 *   the list of run lengths of alternating values, starting with the zeros: counts[0] = 0 when pixel (0,0) is set.  The last run is always
 *   emitted, sum(counts) = H * W, and nruns = 1 + the number of positions p with v[p] != v[p-1] (taking v[-1] = 0).
 *
 *   String.  For run i: x = counts[i]; if i > 2, x -= counts[i-2] (a signed 64-bit value).  Then loop: c = x & 31; x >>= 5 (arithmetic);
 *   more = (c & 16) ? (x != -1) : (x != 0); if more, c |= 32; emit the byte c + 48; stop when `more` is false.  At most 7 bytes per run
 *   for H * W < 2^31.
 *
 *   area = the number of set pixels; bbox = [x0, y0, x1 - x0 + 1, y1 - y0 + 1] over the set pixels, [0, 0, 0, 0] for an empty mask.
 *
 * The rescale of the low-resolution logits (two bilinear resamplings with a crop between them) is vkn_instmask.h's: it writes the masks
 * as bits, and its vkn_bits_rle_encode is this encoder on such bits, without the pack pass.
 * Not built: polygon or uncompressed input, decoding, merging and IoU on RLEs.
 */
#ifndef VKN_RLE_H
#define VKN_RLE_H
#include "vkn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_RLE_STRIP_COLS 64      /* columns of one mask that a workgroup owns: one 64-bit word per row of the strip */
#define VKN_RLE_MAX_K 1024         /* masks of one call */
#define VKN_RLE_MAX_RUN_BYTES 7    /* bytes of one run in the string, for H * W < 2^31 */
#define VKN_RLE_LAUNCHES 8         /* kernel launches of one encode call */
/* the per-mask record: VKN_RLE_RECORD_INTS int32, all written by every call */
#define VKN_RLE_RECORD_INTS 9
#define VKN_RLE_REC_NRUNS 0        /* TRUE number of runs of the mask, whatever the capacity */
#define VKN_RLE_REC_RUN_OFF 1      /* its first run in the run pool: the sum of nruns of the masks before it */
#define VKN_RLE_REC_NBYTES 2       /* TRUE number of bytes of its string */
#define VKN_RLE_REC_BYTE_OFF 3     /* its first byte in the byte pool: the sum of nbytes of the masks before it */
#define VKN_RLE_REC_AREA 4
#define VKN_RLE_REC_BBOX 5         /* x0, y0, width, height */
/* bits of the status word: OR-ed in by the call, cleared by the caller */
#define VKN_RLE_STATUS_FULL_RUNS 1u    /* the runs of the call exceed cap_runs: nothing was written at or beyond the capacity */
#define VKN_RLE_STATUS_FULL_BYTES 2u   /* the bytes of the call exceed cap_bytes: likewise */
#define VKN_RLE_STATUS_FULL (VKN_RLE_STATUS_FULL_RUNS | VKN_RLE_STATUS_FULL_BYTES)

/* ---- bytes of the workspace of one call; 0 outside the envelope: 1 <= K <= VKN_RLE_MAX_K, H, W >= 1, H * W < 2^31,
 *      K * H * W < 2^31 (the size serves both element types; the f32 entry narrows the last condition to K * H * W * 4 < 2^31).
 *      Its largest part is the masks as bits, one 64-bit word per row of a strip: 8 * K * ceil(W / 64) * H bytes. */
size_t vkn_rle_workspace_bytes(int K, int H, int W);

/* ---- masks uint8 [K][H][W], nonzero = set (8 launches).  Outputs:
 *        records  int32 [K][VKN_RLE_RECORD_INTS], the layout above;
 *        runs     uint32 [cap_runs]: the run pool.  Mask k's counts are runs[run_off .. run_off + nruns);
 *        bytes    uint8 [cap_bytes]: the byte pool.  Mask k's string is bytes[byte_off .. byte_off + nbytes);
 *        status   one uint32, see VKN_RLE_STATUS_*.
 *      The masks share the pools; the offsets are prefix sums in mask order, so the used part of a pool is one contiguous prefix.  When
 *      the call's total exceeds a capacity its FULL bit is set, nothing is written at or beyond the capacity (what lies below it is
 *      written as usual), and the records still hold the TRUE nruns and nbytes and the offsets that follow from them: a second call with
 *      pools of the reported totals fits exactly.  Sizes and offsets are 32-bit: exact while the call's runs and bytes each stay below
 *      2^31 (a call has at most K * H * W + K runs).  Only integer arithmetic; two calls on the same input write the same bytes.
 *      Envelope: that of the size query (K * H * W * sizeof(element) < 2^31); rows contiguous, ANY W (the kernel reads aligned 16-byte pieces and keeps
 *      the bytes of its rows); cap_runs, cap_bytes >= 0.  masks, records, runs, bytes, ws 16-byte aligned, status 4-byte aligned. */
int vkn_rle_encode_u8(const unsigned char* masks, int K, int H, int W, int* records, unsigned* runs, int cap_runs, unsigned char* bytes,
                      int cap_bytes, unsigned* status, void* ws, size_t ws_bytes, void* stream);

/* ---- logits float [K][H][W]: a pixel is set iff v > thr, ONE fp32 comparison (equal to thr: 0, NaN: 0, +inf: 1).  Everything else as
 *      vkn_rle_encode_u8 on the bytes `logits > thr`, bit for bit. */
int vkn_rle_encode_f32(const float* logits, float thr, int K, int H, int W, int* records, unsigned* runs, int cap_runs, unsigned char* bytes,
                       int cap_bytes, unsigned* status, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_RLE_H */
