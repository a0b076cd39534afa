/* vkn_stq.h — C ABI of libvkn.so, a metric part: the Segmentation and Tracking Quality (STQ) meter on the device.
 *
 * Conventions and error codes are those of vkn.h: `extern "C"`, DEVICE pointers into caller-owned contiguous memory (the one HOST array is
 * marked), nothing allocated inside, work enqueued asynchronously on `stream`, no host synchronisation, 0 = VKN_OK.  Every entry refuses
 * before any launch, in this order: NULL pointers / negative counts -> VKN_E_ARG, a configuration or shape outside the envelope ->
 * VKN_E_SHAPE, a `state_bytes` that is not vkn_stq_state_bytes(cfg) -> VKN_E_WORKSPACE, a misaligned pointer -> VKN_E_ALIGN, a host
 * pointer where device memory is expected -> VKN_E_ARG (last: it is the only check that asks the runtime).
 *
 * What it replaces: `STQuality.update_state` (tools/utils/STQ.py:106-188) behind the masking and packing of the evaluation scripts
 * (tools/eval_dstq_step.py:47-50, eval_dstq.py, eval_dstq_vipseg.py): two full-resolution maps copied to the host per frame, four
 * np.unique sorts and a dict loop.  Here the four tables the reference accumulates — confusion matrix, ground-truth tube areas,
 * prediction tube areas, intersection areas — are integer counts kept in ONE caller-owned state per sequence; they equal the reference's
 * bit for bit.  The few dozen float64 operations of `STQuality.result()` (:190-283) stay on the host, once per evaluation.
 */
#ifndef VKN_STQ_H
#define VKN_STQ_H
#include "vkn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_STQ_SPAN_PX 2048       /* pixels of one frame that a workgroup takes at a time */
#define VKN_STQ_MAX_GRID 512       /* workgroups of one update (two per compute unit of the MI355X): beyond, a workgroup walks several spans */
#define VKN_STQ_LDS_SLOTS 2048     /* slots of the workgroup's table in LDS (key 8 bytes + count 4 bytes each) */
#define VKN_STQ_HEADER_BYTES 256   /* the state's header: uint32 status, uint32 frames, the rest zero */
#define VKN_STQ_MAX_CLASSES 255
#define VKN_STQ_MIN_CAP 16         /* table capacities: powers of two in [16, 2^20] */
#define VKN_STQ_MAX_CAP 1048576
/* bits of the state's status word, sticky until vkn_stq_reset */
#define VKN_STQ_STATUS_ID_RANGE 1u     /* an instance id outside [0, 2^label_bit_shift): the pixel was skipped */
#define VKN_STQ_STATUS_CLASS_RANGE 2u  /* a class outside [0, n) after the ignore mapping: the pixel was skipped */
#define VKN_STQ_STATUS_FULL_GT 4u      /* the ground-truth tube table was full: a count was dropped */
#define VKN_STQ_STATUS_FULL_PRED 8u    /* the prediction tube table was full */
#define VKN_STQ_STATUS_FULL_PAIR 16u   /* the intersection table was full */
#define VKN_STQ_STATUS_FULL (VKN_STQ_STATUS_FULL_GT | VKN_STQ_STATUS_FULL_PRED | VKN_STQ_STATUS_FULL_PAIR)

/* The reference's constructor arguments (STQ.py:62-100) and the capacities of the three tables.
 *   offset            the reference's `offset`: an intersection is keyed y_true * offset + y_pred;
 *   drop_ignored_gt   1: a pixel whose gt class is `ignore_label` does not exist (the evaluation scripts' `valid_mask_seg`);
 *                     0: `STQuality` on unmasked maps;
 *   cap_gt / cap_pred / cap_pair   slots of the three tables.
 * Envelope: 1 <= num_classes <= 255, 1 <= label_bit_shift <= 30, offset >= num_classes << label_bit_shift (the reference's ValueError),
 * ((num_classes + 1) << label_bit_shift) * offset < 2^62, capacities powers of two in [VKN_STQ_MIN_CAP, VKN_STQ_MAX_CAP]. */
typedef struct VknStqCfg {
    long long offset;
    int num_classes, ignore_label, label_bit_shift, drop_ignored_gt, cap_gt, cap_pred, cap_pair;
} VknStqCfg;
size_t vkn_sizeof_stq_cfg(void);

/* ---- bytes of one state (one sequence); 0 outside the envelope.  Layout, every part 16-byte aligned:
 *      [0] header (VKN_STQ_HEADER_BYTES): uint32 status, uint32 frames (+= B per update, on the device);
 *      [1] int64 confusion[n][n], rows = ground truth, n = num_classes + 1 if ignore_label >= num_classes, else num_classes (STQ.py:81-87);
 *      [2..7] three open-addressing tables, structure of arrays: int64 keys[cap] (empty = -1), int64 counts[cap], for gt, pred, pair.
 *      The slot a key lands in is not part of the contract; the set of (key, count) is. */
size_t vkn_stq_state_bytes(const VknStqCfg* cfg);

/* ---- byte offsets of the eight parts: header, confusion, gt keys, gt counts, pred keys, pred counts, pair keys, pair counts.
 *      offsets8: HOST array of 8. */
int vkn_stq_state_layout(const VknStqCfg* cfg, size_t* offsets8);

/* ---- an empty state (1 fill launch): header and counts 0, keys -1.  All `state_bytes` bytes are written. */
int vkn_stq_reset(const VknStqCfg* cfg, void* state, size_t state_bytes, void* stream);

/* ---- B frames of ONE sequence (1 launch): gt_sem, gt_ins, pred_sem, pred_ins int32 [B][HW]; is_thing uint8 [n], read for classes
 *      below num_classes only (the mapped ignore class is never a thing).  Per pixel, as STQ.py:119-188 behind eval_dstq_step.py:47-50:
 *        drop_ignored_gt and gt_sem == ignore_label: the pixel does not exist;
 *        yt = ((int64)gt_sem << shift) + gt_ins, yp alike;  sl = gt_sem, sp = pred_sem, each num_classes where it equals ignore_label and
 *        ignore_label > num_classes (`>`, while n was chosen with `>=`: STQ.py:127 against :81);
 *        confusion[sl][sp] += 1;  lm = is_thing[sl], pm = is_thing[sp];  crowd = lm and gt_ins == 0 clears both;
 *        pm: pred[yp] += 1;  lm: gt[yt] += 1;  both: pair[yt * offset + yp] += 1.
 *      What the reference cannot take (an IndexError, or a class silently changed) is flagged in the status word and the pixel skipped:
 *      an instance id outside [0, 2^shift) -> VKN_STQ_STATUS_ID_RANGE, a class outside [0, n) after the mapping ->
 *      VKN_STQ_STATUS_CLASS_RANGE.  A full table -> its VKN_STQ_STATUS_FULL_* bit; that count is dropped, nothing else is disturbed, the
 *      probe sequence ends after `cap` slots.  All sums are integer atomics: the result does not depend on the order of arrival.
 *      Envelope: the cfg's, 1 <= B, 1 <= HW, B * HW * 4 < 2^31.  state 16-byte aligned, the maps 4-byte aligned (HW is arbitrary, frame b
 *      starts at b * HW: the kernel peels to its 16-byte loads per span). */
int vkn_stq_update_i32(const VknStqCfg* cfg, void* state, size_t state_bytes, const unsigned char* is_thing, const int* gt_sem,
                       const int* gt_ins, const int* pred_sem, const int* pred_ins, int B, int HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_STQ_H */
