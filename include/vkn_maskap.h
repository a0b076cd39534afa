/* vkn_maskap.h — C ABI of libvkn.so, an instance metric part: COCO mask AP ('segm') from device masks.
 *
 * Conventions and error codes are those of vkn.h: `extern "C"`, DEVICE pointers into caller-owned contiguous memory (the one HOST array is
 * marked), nothing allocated inside, work enqueued asynchronously on `stream`, no host synchronisation (capturable), 0 = VKN_OK.  Every
 * entry refuses before any launch, in this order: NULL pointers / negative counts -> VKN_E_ARG, a configuration or shape outside the
 * envelope -> VKN_E_SHAPE, a `ws_bytes` / `state_bytes` that is not the size query's answer -> VKN_E_WORKSPACE, a misaligned pointer ->
 * VKN_E_ALIGN, a host pointer where device memory is expected -> VKN_E_ARG (last: it is the only check that asks the runtime).
 *
 * What it replaces: `COCOeval(cocoGt, cocoDt, 'segm')` with its `evaluate()` behind the reference's `evaluate(metric=['segm'])`
 * (external/cityscape_panoptic.py:453-568, the same text in external/cityscapes_vps.py; maxDets and iouThrs are set at :356-357 and
 * :475-479).  pycocotools is not part of the reference tree, so the rules of `COCOeval.evaluateImg` are RESTATED at vkn_mask_ap_match
 * below; `accumulate` and `summarize` are float64 and stay on the host (mask_ap_meter.py).  Two parts:
 *   overlap  K detections against G ground truths at full resolution -> exact integer tables (intersections and areas);
 *   match    the tables, scores and labels of one image -> one record per detection in a log in the device state.
 *
 * Not built: bbox IoU, `useCats = 0`, a YouTube-VIS scorer on top of the tube tables (the overlap call ADDS, so calling it once per frame
 * yields them), IoU on RLE strings.
 */
#ifndef VKN_MASKAP_H
#define VKN_MASKAP_H
#include "vkn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_MASKAP_MAX_MASKS 1024     /* detections, and ground truths, of one call */
#define VKN_MASKAP_MAX_CLASSES 256
#define VKN_MASKAP_MAX_THRS 16        /* IoU thresholds: one bit each in a record's words */
#define VKN_MASKAP_MAX_AREAS 4        /* area ranges */
#define VKN_MASKAP_ROW_RUN 32         /* rows of one strip of 64 columns that an overlap workgroup owns */
#define VKN_MASKAP_DT_TILE 64         /* detections of an overlap workgroup: one lane each */
#define VKN_MASKAP_GT_TILE 8          /* ground truths whose counts a lane keeps in registers at a time */
#define VKN_MASKAP_GT_CHUNK 64        /* ground truths whose words of a run are staged in LDS at a time */
#define VKN_MASKAP_HEADER_BYTES 256   /* the state's header: uint32 status, uint32 count (records appended so far, TRUE), the rest zero */
/* the record of one detection: VKN_MASKAP_RECORD_INTS int32 */
#define VKN_MASKAP_RECORD_INTS 12
#define VKN_MASKAP_REC_IMAGE 0        /* the image sequence number of the call */
#define VKN_MASKAP_REC_LABEL 1
#define VKN_MASKAP_REC_SCORE 2        /* the bits of the fp32 score */
#define VKN_MASKAP_REC_RANK 3         /* rank within its category in the image by descending score, -1 beyond max_det (or label out of range) */
#define VKN_MASKAP_REC_WORDS 4        /* per area range a: [4 + 2a] bit t = matched at threshold t, [5 + 2a] bit t = ignored at threshold t */
/* bits of the state's status word, sticky until vkn_mask_ap_reset */
#define VKN_MASKAP_STATUS_FULL 1u         /* more records than cap_records: nothing was written at or beyond the capacity, count stays true */
#define VKN_MASKAP_STATUS_LABEL_RANGE 2u  /* a detection's or a ground truth's label outside [0, num_classes): it takes part in no category */
#define VKN_MASKAP_STATUS_SCORE_NAN 4u    /* a NaN score: ordered behind every number (as NumPy's argsort does) */

/* ---- overlap: bytes of the workspace of one call, the two sides as bits, one 64-bit word per row of a strip of 64 columns;
 *      0 outside the envelope AND for K = G = 0 (then there is nothing to do and `ws` may be NULL).
 *      Envelope: 0 <= K, G <= VKN_MASKAP_MAX_MASKS, H, W >= 1, H * W < 2^31, max(K, G) * H * W < 2^31 (the size serves both element types;
 *      the f32 entry narrows it to K * H * W * 4 < 2^31).  Bytes: up16(8 * K * ceil(W / 64) * H) + up16(8 * G * ceil(W / 64) * H). */
size_t vkn_mask_overlap_workspace_bytes(int K, int G, int H, int W);

/* ---- dt uint8 [K][H][W], gt uint8 [G][H][W]: nonzero = set.  The call ADDS into three int64 tables, which the caller zeroes:
 *        inter[K][G]  += pixels set in both detection k and ground truth g;   area_dt[K] += set pixels of k;   area_gt[G] += set pixels of g.
 *      Calling it once per frame of a video with the same rows and columns therefore yields tube overlaps.  K = 0 and G = 0 are valid
 *      (images without detections or without annotations): the pointers of an empty side (its masks, its area table, and `inter` when
 *      K * G = 0) may be NULL, and the call then does nothing beyond the other side's areas.  Three launches at most (two packs, one
 *      overlap); all sums are 64-bit INTEGER atomics, so the result does not depend on the order of arrival: the same input gives the same bits.
 *      Envelope: that of the size query; rows contiguous, ANY W.  dt, gt, the tables and ws 16-byte aligned. */
int vkn_mask_overlap_u8(const unsigned char* dt, const unsigned char* gt, int K, int G, int H, int W, long long* inter, long long* area_dt,
                        long long* area_gt, void* ws, size_t ws_bytes, void* stream);

/* ---- dt float [K][H][W]: a pixel is set iff v > thr, ONE fp32 comparison (equal to thr: 0, NaN: 0, +inf: 1), the rule of
 *      vkn_rle_encode_f32.  Everything else as vkn_mask_overlap_u8 on the bytes `dt > thr`, bit for bit. */
int vkn_mask_overlap_f32(const float* dt, float thr, const unsigned char* gt, int K, int G, int H, int W, long long* inter, long long* area_dt,
                         long long* area_gt, void* ws, size_t ws_bytes, void* stream);

/* The configuration of a meter.
 *   iou_thrs[T]            IoU thresholds (COCO: 0.5, 0.55 .. 0.95), 1 <= T <= VKN_MASKAP_MAX_THRS;
 *   area_lo[A], area_hi[A] area ranges [lo, hi], both ends inside (COCO: all, small, medium, large), 1 <= A <= VKN_MASKAP_MAX_AREAS;
 *   num_classes            1 .. VKN_MASKAP_MAX_CLASSES;   max_det: the largest of maxDets, 1 .. VKN_MASKAP_MAX_MASKS;
 *   cap_records            records of the log, 1 .. 2^24.
 * Entries of the arrays beyond T and A are not read. */
typedef struct VknMaskApCfg {
    double iou_thrs[VKN_MASKAP_MAX_THRS];
    double area_lo[VKN_MASKAP_MAX_AREAS], area_hi[VKN_MASKAP_MAX_AREAS];
    int num_classes, T, A, max_det, cap_records, reserved;
} VknMaskApCfg;
size_t vkn_sizeof_mask_ap_cfg(void);

/* ---- bytes of one state; 0 outside the envelope.  Three parts, each 16-byte aligned:
 *      [0] header (VKN_MASKAP_HEADER_BYTES): uint32 status, uint32 count, the rest zero;
 *      [1] int64 npig[num_classes][A]: ground truths that are not ignored, summed over the calls so far;
 *      [2] int32 log[cap_records][VKN_MASKAP_RECORD_INTS]: the first min(count, cap_records) records are valid, in the order of the
 *          calls and, inside a call, in the detections' input order. */
size_t vkn_mask_ap_state_bytes(const VknMaskApCfg* cfg);

/* ---- byte offsets of the three parts.  offsets3: HOST array of 3. */
int vkn_mask_ap_state_layout(const VknMaskApCfg* cfg, size_t* offsets3);

/* ---- an empty state (1 fill): all `state_bytes` bytes are written, with zero. */
int vkn_mask_ap_reset(const VknMaskApCfg* cfg, void* state, size_t state_bytes, void* stream);

/* ---- one image: `COCOeval.evaluateImg` for every (category, area range) at maxDet = max_det, from the tables of the overlap call
 *      (inter int64 [K][G], area_dt int64 [K], area_gt int64 [G]: pixel counts), scores f32 [K], dt_labels i32 [K], gt_labels i32 [G],
 *      gt_crowd u8 [G] (nonzero = crowd), gt_area f64 [G] or NULL (COCO takes a ground truth's area from the annotation; NULL: the pixel
 *      count).  The rules, per category c and area range [lo, hi]:
 *        detections of c are ordered by descending score, stable in input order (argsort(-score, kind='mergesort'): NaN last); the
 *          first max_det are kept, `rank` is the position in that order;
 *        a ground truth of c is IGNORED iff it is crowd or its area is < lo or > hi; ground truths are ordered non-ignored first, stable;
 *        iou = (double) I / (double) U, U = area_dt for a crowd ground truth and area_dt + area_gt - I otherwise; I = 0 gives iou 0 with
 *          no division (a stated deviation from pycocotools for an empty detection against a crowd region);
 *        per threshold t the detections are taken in order: best = min(t, 1 - 1e-10), m = none; walk the ordered ground truths: skip one
 *          already matched at t unless it is crowd; stop at the first ignored one once m is a non-ignored match; skip one with
 *          iou < best; otherwise best = iou, m = it (an equal IoU moves the match to the later ground truth);
 *        a matched detection takes its ground truth's ignore flag; an unmatched detection whose own area (pixel count) is < lo or > hi
 *          is ignored.
 *      Comparisons are fp64 on values that are exact integers before the one division.  The call appends exactly K records (layout
 *      above) and adds the non-ignored ground truths into npig.  match_gt: NULL, or int32 [A][T][K] that is written whole: the matched
 *      ground truth's input index per detection in input order, -1 for none.  Status bits: VKN_MASKAP_STATUS_*.  Three launches.
 *      K = 0 and G = 0 are valid; the pointers of an empty side, and inter when K * G = 0, may be NULL.
 *      Envelope: the cfg's, 0 <= K, G <= VKN_MASKAP_MAX_MASKS.  state and the tables 16-byte aligned, gt_area 8-byte, scores, labels and
 *      match_gt 4-byte aligned. */
int vkn_mask_ap_match(const VknMaskApCfg* cfg, void* state, size_t state_bytes, const long long* inter, const long long* area_dt,
                      const long long* area_gt, const float* scores, const int* dt_labels, const int* gt_labels, const unsigned char* gt_crowd,
                      const double* gt_area, int K, int G, int image_seq, int* match_gt, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_MASKAP_H */
