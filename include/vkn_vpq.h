/* vkn_vpq.h — C ABI of libvkn.so, a windowed metric part: video panoptic quality (VPQ) on the device.
 *
 * Conventions and error codes are those of vkn.h: `extern "C"`, DEVICE pointers into caller-owned contiguous memory (the one HOST array is
 * marked), nothing allocated inside, work enqueued asynchronously on `stream`, no host synchronisation, 0 = VKN_OK.  Every entry refuses
 * before any launch, in this order: NULL pointers / negative counts -> VKN_E_ARG, a configuration or shape outside the envelope ->
 * VKN_E_SHAPE, a `state_bytes` that is not vkn_vpq_state_bytes(cfg) -> VKN_E_WORKSPACE, a misaligned pointer -> VKN_E_ALIGN, a host
 * pointer where device memory is expected -> VKN_E_ARG (last: it is the only check that asks the runtime).
 *
 * What it replaces: `vpq_eval` (tools/eval_dvpq_step.py:21-97, the same text in tools/eval_dvpq_vipseg.py:310-386) behind `eval()`
 * (eval_dvpq_step.py:100-141) / `read_to_eval()` (eval_dvpq_vipseg.py:389-409), which concatenate the k frames of a window side by side
 * (eval_dvpq_step.py:106-107, :138) and run three np.unique sorts over all their pixels (eval_dvpq_step.py:33-47), once per window and
 * once more per window length.  A window's areas are the sums of its frames' areas, so here every frame is counted ONCE into its own
 * tables, and every window of every length follows from those tables without touching a pixel.  tp, fn, fp are integer counts; for the
 * float64 sum of IoUs (eval_dvpq_step.py:74-77) the device records the two integers of every true positive and the host divides and
 * adds them in the scripts' order.  The last lines (eval_dvpq_step.py:207-222, eval_dvpq_vipseg.py:469-485) stay on the host.
 *
 * Two deliberate departures from the scripts:
 *   (a) eval_dvpq_step.py:111-113 hands `vpq_eval` int32 ground truth, so `_ign_id * offset` at eval_dvpq_step.py:56 wraps in 32 bits
 *       (NumPy warns of the overflow) and the ignored overlap reads an unrelated key.  The meter computes every key in 64 bits, as
 *       eval_dvpq_vipseg.py does with its int64 ground truth (eval_dvpq_vipseg.py:399).
 *   (b) eval_dvpq_vipseg.py:441 sets `k = min(k, len_seq)`, which shortens k for a short sequence AND for every sequence after it.  That is
 *       not reproduced: a sequence shorter than k contributes no window of that k (eval_dvpq_step.py:187).
 */
#ifndef VKN_VPQ_H
#define VKN_VPQ_H
#include "vkn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_VPQ_MAX_KS 4           /* window lengths of one meter */
#define VKN_VPQ_MAX_K 8            /* the longest window, in frames */
#define VKN_VPQ_GROUP 8            /* frames of one call that share a launch of each kind */
#define VKN_VPQ_SPAN_PX 2048       /* pixels of one frame that a workgroup takes at a time */
#define VKN_VPQ_MAX_GRID 512       /* workgroups of one count launch: beyond, a workgroup walks several spans of its frame */
#define VKN_VPQ_LDS_SLOTS 2048     /* slots of the counting workgroup's table in LDS (key 8 bytes + count 4 bytes each) */
#define VKN_VPQ_HEADER_BYTES 256   /* the state's header: uint32 status, uint32 frames, uint32 log_used, the rest zero */
#define VKN_VPQ_MAX_CAT 255
#define VKN_VPQ_MIN_CAP 16         /* capacities: powers of two in [16, 2^20] */
#define VKN_VPQ_MAX_CAP 1048576
/* bits of the state's status word, sticky until vkn_vpq_reset */
#define VKN_VPQ_STATUS_ID_RANGE 1u     /* an instance id outside [0, 2^label_bit_shift): the pixel was skipped */
#define VKN_VPQ_STATUS_CLASS_RANGE 2u  /* a prediction class outside [0, num_cat), or a gt class that is neither in it nor ign_id: skipped */
#define VKN_VPQ_STATUS_FULL_GT 4u      /* a frame's or a window's table of gt segments was full: a count was dropped */
#define VKN_VPQ_STATUS_FULL_PRED 8u    /* ... of predicted segments */
#define VKN_VPQ_STATUS_FULL_PAIR 16u   /* ... of intersections */
#define VKN_VPQ_STATUS_FULL_LOG 32u    /* the log of true positives was full: a record was dropped */
#define VKN_VPQ_STATUS_FULL (VKN_VPQ_STATUS_FULL_GT | VKN_VPQ_STATUS_FULL_PRED | VKN_VPQ_STATUS_FULL_PAIR | VKN_VPQ_STATUS_FULL_LOG)

/* The constants of `vpq_eval` (eval_dvpq_step.py:23-26, eval_dvpq_vipseg.py:312-315), the window lengths and the capacities.
 *   offset            the scripts' 2^30: an intersection is keyed gt_id * offset + pred_id (eval_dvpq_step.py:46);
 *   num_cat           bins: classes + 1 (20 for STEP, 125 for VIP-Seg);
 *   ign_id            255;  label_bit_shift: max_ins = 2^shift, 16 in both scripts;
 *   nk, ks            window lengths (`--eval_frames`, eval_dvpq_step.py:14; eval_dvpq_vipseg.py:494), strictly ascending;
 *   cap_gt / cap_pred / cap_pair   slots of the three tables of ONE frame and of ONE window;  cap_log: records of the TP log.
 * Envelope: 1 <= num_cat <= 255, num_cat <= ign_id <= 255, 1 <= label_bit_shift <= 30, offset >= num_cat << shift (every prediction id
 * is below offset), ((ign_id + 1) << shift) * offset < 2^62, 1 <= nk <= VKN_VPQ_MAX_KS, 1 <= ks[i] <= VKN_VPQ_MAX_K ascending,
 * capacities powers of two in [VKN_VPQ_MIN_CAP, VKN_VPQ_MAX_CAP].  ks beyond nk are not read. */
typedef struct VknVpqCfg {
    long long offset;
    int num_cat, ign_id, label_bit_shift;
    int nk, ks[VKN_VPQ_MAX_KS];
    int cap_gt, cap_pred, cap_pair, cap_log;
} VknVpqCfg;
size_t vkn_sizeof_vpq_cfg(void);

/* ---- bytes of one state (one sequence); 0 outside the envelope.  Four parts, each 16-byte aligned:
 *      [0] header (VKN_VPQ_HEADER_BYTES): uint32 status, uint32 frames (+= B per update, on the device), uint32 log_used, the rest zero;
 *      [1] int64 acc[nk][3][num_cat]: tp, fn, fp per class (eval_dvpq_step.py:76, :87, :95) summed over every window of length ks[i] so far;
 *      [2] int64 log[cap_log][4]: one record per true positive (eval_dvpq_step.py:75-77): (k_index << 48) | window_ordinal (the index of
 *          the window's first frame), the pair key gt_id * offset + pred_id, int_area, union.  The first log_used records are valid; the
 *          slot a record lands in is not part of the contract, the set of records is;
 *      [3] private: the ring of per-frame tables and the windows' scratch. */
size_t vkn_vpq_state_bytes(const VknVpqCfg* cfg);

/* ---- byte offsets of the four parts.  offsets4: HOST array of 4. */
int vkn_vpq_state_layout(const VknVpqCfg* cfg, size_t* offsets4);

/* ---- an empty state (1 fill): all `state_bytes` bytes are written, with zero. */
int vkn_vpq_reset(const VknVpqCfg* cfg, void* state, size_t state_bytes, void* stream);

/* ---- B CONSECUTIVE frames of ONE sequence, behind the frames of earlier calls: gt_sem, gt_ins, pred_sem, pred_ins int32 [B][HW].
 *      With gt_id = ((int64)gt_sem << shift) + gt_ins and pred_id alike (eval_dvpq_step.py:108-113), per frame f of the sequence and per
 *      window length k = ks[i] with f + 1 >= k (eval_dvpq_step.py:187), the window is frames f - k + 1 .. f and
 *        areas: gt[gt_id], pred[pred_id], int[gt_id * offset + pred_id], each summed over the window's frames (eval_dvpq_step.py:37-47);
 *        a pair of equal classes is a true positive iff 2 * int > gt + pred - int - void, void = int[(ign_id << shift) * offset + pred_id]
 *        (eval_dvpq_step.py:49-51, :68-75: `int / union > 0.5` in float64 is this predicate for areas below 2^40): tp[class] += 1, one log record;
 *        a gt segment with no true positive and a class other than ign_id: fn[class] += 1 (eval_dvpq_step.py:81-87);
 *        a prediction with no true positive: fp[class] += 1 unless 2 * (its overlap with ALL gt ids of class ign_id) > its area
 *        (eval_dvpq_step.py:53-58, :89-95).
 *      What the reference cannot take is flagged in the status word and the pixel skipped: an instance id outside [0, 2^shift) ->
 *      VKN_VPQ_STATUS_ID_RANGE; a prediction class outside [0, num_cat), or a gt class neither in [0, num_cat) nor ign_id ->
 *      VKN_VPQ_STATUS_CLASS_RANGE.  A full table -> its VKN_VPQ_STATUS_FULL_* bit; that count or record is dropped, nothing else is
 *      disturbed, a probe sequence ends after `cap` slots.  All sums are integer atomics: the result does not depend on the order of
 *      arrival.  Launches: three per VKN_VPQ_GROUP frames of the call (clear the frames' ring slots, count, windows).
 *      Envelope: the cfg's, 1 <= B, 1 <= HW, B * HW * 4 < 2^31.  state 16-byte aligned, the maps 4-byte aligned (HW is arbitrary, frame b
 *      starts at b * HW: the kernel peels to its 16-byte loads per span). */
int vkn_vpq_update_i32(const VknVpqCfg* cfg, void* state, size_t state_bytes, const int* gt_sem, const int* gt_ins, const int* pred_sem,
                       const int* pred_ins, int B, int HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_VPQ_H */
