/* vkn_track.h — C ABI of libvkn.so, second part: the video detector's tracking tail.
 *
 * Conventions, error codes and structs are those of vkn.h (included below): `extern "C"`, DEVICE pointers into caller-owned contiguous
 * memory, nothing allocated inside, work enqueued asynchronously on `stream`, no host synchronisation, 0 = VKN_OK.
 *
 * What it replaces: the stretch of `simple_test` between the panoptic merge and the two maps the detector returns,
 * knet/video/knet_quansi_dense_embed_fc_joint_train.py:536-603 with the helpers `get_things_id_for_tracking` (:673-685),
 * `get_semantic_seg` (:698-722) and `generate_track_id_maps` (:724-736).  Upstream of it is vkn_panoptic_joint_f32, between the two
 * entry points sits vkn_qd_tracker_match_f32 (vkn.h) or its device-count form below: the chain needs no host copy.
 */
#ifndef VKN_TRACK_H
#define VKN_TRACK_H
#include "vkn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Capacity of the per-frame LDS tables: K = max_per_img + num_stuff_classes entries.  The largest shipped config is VIP-Seg with
 * 100 + 66 = 166 (KITTI-STEP: 100 + 17, Cityscapes: 100 + 11). */
#define VKN_TRACK_MAX_K 512

/* ---- thing boxes for the tracker, the frames [B] of one geometry in one launch sequence (3 launches).
 *      in : panoptic_seg int32 [B][Ho][Wo], info int32 [B][K][6], nseg int32 [B] — exactly as vkn_panoptic_joint_f32 writes them;
 *           sem_logits fp32 [B][Cs][hs][ws] (the kernel-initialisation head's `seg_preds`) or NULL: no semantic filter.
 *      out: the ENTRIES = the accepted thing entries of info (info[.][2] > 0 and joint label < num_thing_classes), compacted in
 *           ascending segment-id order — the order of `get_things_id_for_tracking` over `segments_info` (:673-685):
 *           det fp32 [B][K][5] rows (xmin, ymin, xmax, ymax, score); labels int64 [B][K]; rows int32 [B][K] = the mask row (kernel
 *           index) of the entry, for gathering `object_feats`; segid int32 [B][K]; count int32 [B].  Rows >= count[b] are zero.
 *           (nseg[b] < 0, vkn_panoptic_joint_f32's capacity error, gives count[b] = 0.)
 *           thing_mask uint8 [B][Ho][Wo] or NULL: semantic_thing per pixel (1 everywhere when sem_logits is NULL) — the detector's
 *           own intermediate (:551).
 *      The box is `tensor_mask2box` (unitrack/utils/mask.py:80-90) of `(panoptic_seg == id) * semantic_thing` (:567, :583), in the
 *      coordinate convention of vkn_panoptic_joint_f32's `bbox`; an empty product gives (-1, -1, 10, 10) and the entry still counts.
 *      semantic_thing(p): sem_logits interpolated bilinearly to (Ho, Wo) (align_corners=False, ATen's source-index rule, fp32), then
 *      the channel arg-max; a thing pixel when that channel is < num_thing_classes.  The reference applies a sigmoid before the
 *      arg-max (:549); here the arg-max is taken on the logits, ties to the LOWEST channel: sigmoid is monotone, so this differs
 *      from the reference only where two different logits give the same fp32 sigmoid value (saturation, |logit| beyond ~17),
 *      where the reference's arg-max picks the lowest of the collided channels.  With thing_mask == NULL the interpolation is
 *      evaluated only for pixels of thing segments.
 *      Deterministic: per-workgroup (min, max) per entry in LDS through integer atomics, then global integer atomicMin / atomicMax.
 *      Segment ids are distinct in vkn_panoptic_joint_f32's info; of a repeated id only the first entry is kept.
 *      Before any launch: K > VKN_TRACK_MAX_K, Ho * Wo * 4 >= 2^31 (or the same for one frame of sem_logits), Ho > 16 * 65535 or
 *      B > 65535 -> VKN_E_SHAPE; a NULL or host pointer -> VKN_E_ARG; a pointer that is not 16-byte aligned -> VKN_E_ALIGN;
 *      ws: vkn_track_boxes_workspace_bytes. */
size_t vkn_track_boxes_workspace_bytes(int B, int K);
int vkn_track_boxes_f32(const int* panoptic_seg, const int* info, const int* nseg, const float* sem_logits, int Cs, int hs, int ws_w,
                        int num_thing_classes, int B, int K, int Ho, int Wo, float* det, int64_t* labels, int* rows, int* segid,
                        int* count, unsigned char* thing_mask, void* ws, size_t ws_bytes, void* stream);

/* ---- the two maps the detector returns (2 launches: per-frame look-up tables by segment id, then out[p] = lut[panoptic_seg[p]]).
 *      in : panoptic_seg, info as above; segid [B][K], count [B] from vkn_track_boxes_f32;
 *           ids int64 [B][max_dets], n_ids int32 [B]: the tracker's `out_ids` / `out_count` (for B = 1 the pointers of one
 *           vkn_qd_tracker_match_f32 call, passed straight on; n_ids needs 4-byte alignment only);
 *           sem_of_label int32 [num_labels], num_labels = num_thing_classes + num_stuff_classes: the semantic class of a joint label,
 *           built by the caller on the host from `get_semantic_seg` (:698-722) and kept in device memory.
 *      out: track_map int32 [B][Ho][Wo] = `generate_track_id_maps` (:724-736) on the ids of :591-592: the i-th thing segment in
 *           segment order gets ids[i] + 1 (a result of -1 becomes 0) for i < min(count, n_ids); every other pixel 0.  This KEEPS the
 *           reference's pairing of the tracker's i-th RETURNED row (score order, suppressed detections removed) with the i-th
 *           segment: it is the reference's behaviour, not a property anyone should rely on beyond parity.
 *           semantic_map int32 [B][Ho][Wo] = sem_of_label[joint label of the pixel's segment], void 0 (`np.zeros`).
 *      The reference returns float64 NumPy arrays; these are int32 device tensors with the same values.
 *      Error codes as vkn_track_boxes_f32; ws: vkn_track_maps_workspace_bytes. */
size_t vkn_track_maps_workspace_bytes(int B, int K);
int vkn_track_maps_i32(const int* panoptic_seg, const int* segid, const int* count, const int64_t* ids, const int* n_ids, int max_dets,
                       const int* info, const int* sem_of_label, int num_labels, int B, int K, int Ho, int Wo, int* track_map,
                       int* semantic_map, void* ws, size_t ws_bytes, void* stream);

/* ---- the tracker's envelope (vkn_qd_tracker_* of vkn.h and the entry below): max_dets <= 256, max_tracklets +
 *      max(memo_backdrop_frames, 1) * max_dets <= 4096, embed_dim <= 1024 and memo_backdrop_frames <= VKN_TRACKER_MAX_BACKDROP_FRAMES
 *      (the match kernel keeps one offset per backdrop frame in LDS).  Outside it vkn_qd_tracker_state_bytes / _workspace_bytes answer
 *      0 and _state_layout, _reset, _match_f32 and _match_dev_f32 return VKN_E_SHAPE before any launch.
 *      Full tracklet table: a birth that finds max_tracklets live rows is dropped (status bit 1 of that call; its id is consumed and
 *      returned).  The capacity test runs BEFORE the expiry compaction of the same call, so a birth into a full table is dropped
 *      even when another track expires in that very frame; the freed row serves the next frame. */
#define VKN_TRACKER_MAX_BACKDROP_FRAMES 64

/* ---- vkn_qd_tracker_match_f32 (vkn.h) with the number of detections in DEVICE memory: n = min(*n_dev, n_max), where n_max <=
 *      cfg->max_dets is the number of rows the input buffers hold (count / K of vkn_track_boxes_f32).  n == 0 — a frame without
 *      things, which the detector does not hand to its tracker (:569-573, :597-598) — writes out_count = (0, 0) and leaves the state
 *      untouched.  Everything else as vkn_qd_tracker_match_f32; all pointers required (VKN_E_ARG), n_max in [1, cfg->max_dets]
 *      (VKN_E_ARG below, VKN_E_SHAPE above). */
int vkn_qd_tracker_match_dev_f32(const VknTrackerCfg* cfg, void* state, size_t state_bytes, const float* bboxes, const int64_t* labels,
                                 const float* embeds, const int* n_dev, int n_max, int frame_id, float* out_bboxes, int64_t* out_labels,
                                 int64_t* out_ids, int* out_count, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_TRACK_H */
