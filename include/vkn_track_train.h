/* vkn_track_train.h — C ABI of libvkn.so, third part: the tracking loss of a training step.
 *
 * Conventions, error codes and the status word are those of vkn.h (included through vkn_track.h): `extern "C"`, DEVICE pointers into
 * caller-owned contiguous memory, nothing allocated inside, work enqueued asynchronously on `stream`, no host synchronisation,
 * 0 = VKN_OK.
 *
 * What it replaces: the end of the "Tracking Part" of `forward_train`, knet/video/knet_quansi_dense_embed_fc_joint_train.py:439-460 —
 * the gather of the positive rows (:440-452), `track_head.match` (knet/video/track_heads.py:678-697), `get_track_targets` (:658-676)
 * and `loss` (:699-716) with `MultiPosCrossEntropyLoss` (knet/video/qdtrack/losses/multipos_cross_entropy_loss.py:6-40) and `L2Loss`
 * (knet/video/qdtrack/losses/l2_loss.py:24-113, `hard_mining=True` or no mining) — and autograd's backward of all of it down to the two
 * embedding tensors.  Upstream of it are the embedding layers and the track head (torch, under autograd) and the assigner's `gt_inds`.
 */
#ifndef VKN_TRACK_TRAIN_H
#define VKN_TRACK_TRAIN_H
#include "vkn_track.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows per image (`num_proposals`; every shipped config has 100).  The [Kk x Kr] similarity matrix of an image lives in LDS. */
#define VKN_TRACK_LOSS_MAX_ROWS 128

/* The head's loss configuration (track_heads.py:552-636): `softmax_temp` (> 0: dists = cosine / softmax_temp, else dot products),
 * `has_aux` (0: no `loss_track_aux`, losses[1] = 0), the two `loss_weight`s, and L2Loss's `neg_pos_ub` (an integer ratio; <= 0: no
 * mining), `pos_margin`, `neg_margin` (applied only when > 0). */
typedef struct VknTrackLossCfg {
    float softmax_temp;
    int has_aux;
    float w_track;
    float w_aux;
    int neg_pos_ub;
    float pos_margin;
    float neg_margin;
} VknTrackLossCfg;
size_t vkn_sizeof_track_loss_cfg(void);

/* ---- forward (2 launches: one workgroup per image, then the mean over the images).
 *      in : key_embeds, ref_embeds fp32 [B][N][E]: the track head's outputs for ALL N rows of an image;
 *           key_gt, ref_gt int64 [B][N]: the assigner's `gt_inds` (0: no ground truth, g + 1 otherwise).  The positives of an image are
 *           its rows with gt > 0 in ascending row order — the order of `pos_inds` (:440-452); the kernel compacts them itself
 *           (Kk key rows, Kr reference rows).  A caller with compact rows passes `pos_assigned_gt_inds + 1`, zero-padded to N;
 *           match int64 [n_match]: the images' `gt_match_indices` concatenated, match_off int64 [B + 1] their offsets: entry g of
 *           image b is the partner instance in the reference frame, or -1.
 *      Per image (track_heads.py:658-716):
 *           t[k][r] = (match[key_gt_k - 1] == ref_gt_r - 1),  w[k] = any_r t[k][r];
 *           cos = the product of the L2-normalised rows (norm clamped at 1e-12 from below, `F.normalize`),
 *           dists = K R^T, or cos / softmax_temp when softmax_temp > 0;
 *           loss_track = w_track * sum_k w_k softplus(lse_{t=0}(dists_k) + lse_{t=1}(-dists_k)) / sum_k w_k, logsumexp in the
 *           max-shifted form, a row without a positive or without a negative contributing 0;
 *           loss_track_aux = L2Loss(weight=None): pred = clamp(cos - margin(t), 0, 1); num_pos = sum t, num_neg = Kk Kr - num_pos; when
 *           neg_pos_ub > 0 and num_neg / (num_pos + 1) > neg_pos_ub only the num_pos * neg_pos_ub negatives of largest pred^2 stay
 *           (hard mining); w_aux * sum_kept (pred - t)^2 / #kept.
 *           Mining is a k-th-largest selection inside the workgroup (radix select over the bit patterns of the non-negative fp32
 *           costs); TIES AT THE CUT go to the lowest (k, r) in row-major order of the compacted matrix (`topk` leaves them open).
 *      out: losses fp32 [2] = (loss_track, loss_track_aux), each the mean over the B images; a 0 / 0 (no key with a partner: sum w = 0,
 *           #kept = 0) is NaN as on the host path;
 *           stats int32 [B][4] = (Kk, Kr, num_pos, kept negatives; the last 0 without the auxiliary loss);
 *           aux_kept uint8 [B][N][N] or NULL: the final `weight > 0` mask of the L2 loss by ORIGINAL (key row, reference row);
 *           status: the status word of a workspace (vkn_workspace_status): VKN_STATUS_RANGE is ORed into it when a key_gt entry lies
 *           outside [0, G_b] (G_b = the image's number of match entries), a ref_gt entry is negative or >= 2^31, a match entry is
 *           < -1 or >= 2^31 - 1, or match_off is not ascending inside [0, n_match]; such an entry counts as 0 (-1 for match), nothing
 *           is read out of bounds, the losses of that call are meaningless;
 *           ws: what the backward reads (per image: the compaction, the row norms, cos, d loss / d dists, d loss / d cos);
 *           vkn_track_loss_workspace_bytes.  It must stay untouched until the backward has run.
 *      An image with Kk == 0 or Kr == 0 is not this entry point's case (the host path asserts there): its results are unspecified.
 *      Every reduction runs in a fixed order without floating-point atomics: the same inputs give the same bits, and the compact and
 *      the full-row form of the same rows give the same bits.
 *      Before any launch: NULL cfg / key_embeds / ref_embeds / key_gt / ref_gt / match / match_off / losses / stats / status or
 *      n_match < 0 -> VKN_E_ARG; N outside [1, VKN_TRACK_LOSS_MAX_ROWS], E % 4 != 0, E outside [4, 1024], B outside [1, 65535] ->
 *      VKN_E_SHAPE; a pointer that is not 16-byte aligned (status: 4-byte) -> VKN_E_ALIGN; ws NULL / too small -> VKN_E_WORKSPACE;
 *      a host pointer -> VKN_E_ARG. */
size_t vkn_track_loss_workspace_bytes(int B, int N);
int vkn_track_loss_fwd_f32(const VknTrackLossCfg* cfg, const float* key_embeds, const float* ref_embeds, const int64_t* key_gt,
                           const int64_t* ref_gt, const int64_t* match, const int64_t* match_off, long long n_match, int B, int N, int E,
                           float* losses, int* stats, unsigned char* aux_kept, int* status, void* ws, size_t ws_bytes, void* stream);

/* ---- backward (1 launch, one workgroup per image): autograd's backward of the above (l2_loss.py / multipos_cross_entropy_loss.py
 *      under `loss.backward()`).  gout fp32 [2] in DEVICE memory: the upstream gradients of the two losses, honoured independently;
 *      cfg, key_embeds, ref_embeds, B, N, E and ws as in the forward call.
 *      out: d_key, d_ref fp32 [B][N][E]; exactly zero on rows with gt == 0.  The cosine goes through the normalisation; the clamp
 *      passes gradient where 0 <= cos - margin <= 1 (ATen's clamp_backward).  Error codes as above. */
int vkn_track_loss_bwd_f32(const VknTrackLossCfg* cfg, const float* key_embeds, const float* ref_embeds, const float* gout, int B, int N,
                           int E, float* d_key, float* d_ref, const void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_TRACK_TRAIN_H */
