/* vkn_wattn_train.h — C ABI of libvkn.so, a backbone training part: the backward of the (shifted-)window attention core of
 * `SwinTransformerDIY`, whose forward is vkn_swin_window_attn_f32 of vkn_swin.h.
 *
 * Conventions and error codes are those of vkn.h: `extern "C"`, DEVICE pointers into caller-owned fp32 memory, 16-byte aligned, nothing
 * allocated inside, work enqueued asynchronously on `stream`, no host synchronisation (capturable), 0 = VKN_OK.  The entry refuses before
 * any launch, in this order: NULL pointers / counts <= 0 / `dqkv_bias` given without `qkv_bias` or the reverse -> VKN_E_ARG, a shape
 * outside the envelope -> VKN_E_SHAPE, a workspace that is NULL or smaller than vkn_wattn_bwd_workspace_bytes -> VKN_E_WORKSPACE, a
 * misaligned pointer (the workspace included) -> VKN_E_ALIGN.  The workspace has no status header: it is used from offset 0.
 * No float atomics: every sum has a fixed order, two runs on the same inputs are bitwise equal.  Non-finite inputs propagate as they
 * do in the torch composition; there is no status word.
 *
 * Nothing of the forward is saved.  Geometry, pad tokens (k and v of a pad token are the bias of `qkv`, zero without one), rel(i, j),
 * regions and mask are those of vkn_swin.h, and for head m of one window the scores, their maximum and the softmax are recomputed from
 * `qkv` with the forward's arithmetic in the forward's order: q scale first, the dot product, + bias_table[rel(i, j)][m],
 * + VKN_SWIN_MASK across regions, p_ij = expf(s_ij - max_i) summed in key order, P_ij = p_ij (1 / sum_i).  Then, in plain fp32 FMA,
 *     dP_ij = dout_i . v_j          delta_i = sum_j P_ij dP_ij          dS_ij = P_ij (dP_ij - delta_i)
 *     dv_j  = sum_i P_ij dout_i     dq_i = scale sum_j dS_ij k_j        dk_j = sum_i dS_ij (scale q_i)
 *     dbias_table[rel(i, j)][m] += dS_ij
 * with the sums over j in key order and the sums over i in query order (y ws + x inside the window).  delta_i alone is formed in
 * fp64, as (sum_j p_ij dP_ij) / (sum_j p_ij) rounded once: keys with the same v (all pad keys of a window: their v is the bias) then
 * get dS_ij = 0 exactly where the softmax's weight lies on them alone.  A pad query has no output (it is cropped), so its row takes
 * dout = 0 and adds nothing anywhere.
 *
 * Each real token lies in exactly one window: its row of `dqkv` is written once, by that window, without atomics.  A pad KEY receives
 * dk and dv like any other key but has no row of `dqkv`: its k and v are the bias, so those gradients are summed into `dqkv_bias`, the
 * part of the bias gradient that flows through pad tokens ONLY (the part through real tokens is the `qkv` Linear's own business: it
 * follows from `dqkv`).  The q third of `dqkv_bias` is written as zeros.  The sums across windows — `dbias_table`, the pad part of
 * `dqkv_bias` — go through per-(image, window, head) partials in the workspace (VKN_WATTN_PART_FLOATS floats of dk | dv and
 * (2 window - 1)^2 floats of the table image each) and a second launch that adds them in fp64 in a fixed order:
 * VKN_WATTN_MERGE_SLICES interleaved slices of the windows, each in window order, then the slices in order.
 *
 * Safety: every global address is formed from a token position that was reduced modulo the padded extent and compared with H, W first;
 * pad positions form no address into `qkv`, `dout` or `dqkv`.  No input VALUE reaches an address.
 *
 * Envelope: the forward's (vkn_swin.h: head_dim = VKN_SWIN_HEAD_DIM, window^2 <= VKN_SWIN_MAX_WINDOW_TOKENS, 0 <= shift < window,
 * heads <= VKN_SWIN_MAX_HEADS, every tensor below 2^31 bytes) and a workspace below 2^31 bytes.
 *
 * Not built: a backward of the Linears, LayerNorms or the MLP around the core, another head_dim, attention dropout, an MFMA variant. */
#ifndef VKN_WATTN_TRAIN_H
#define VKN_WATTN_TRAIN_H
#include "vkn_swin.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_WATTN_PART_FLOATS 64          /* one (image, window, head)'s pad partial: dk [32] | dv [32] */
#define VKN_WATTN_MERGE_SLICES 16         /* the merge adds the windows in this many interleaved slices, then the slices in order */
#define VKN_WATTN_WS_ALIGN 256            /* the table partials are rounded up to this many bytes; the pad partials follow */

/* 1 inside the envelope above (sizes included), else 0.  Asks the runtime nothing. */
int vkn_wattn_bwd_supported(int B, int H, int W, int heads, int window, int shift);

/* With nW the windows of one padded image and T = (2 window - 1)^2: 4 B nW heads T rounded up to VKN_WATTN_WS_ALIGN, plus
 * 4 B nW heads VKN_WATTN_PART_FLOATS.  Exact; 0 outside the envelope (which no `shift` changes). */
size_t vkn_wattn_bwd_workspace_bytes(int B, int H, int W, int heads, int window);

/* qkv, qkv_bias (or NULL), bias_table: the forward's operands, as vkn_swin.h states them;
 * dout        [B][H][W][heads 32], the gradient of the forward's `out`;
 * dqkv        [B][H][W][3][heads][32]: every element written, exactly once;
 * dqkv_bias   [3][heads][32]: the pad part of the bias gradient (q third zeros), every element written; NULL exactly when qkv_bias is;
 * dbias_table [(2 window - 1)^2][heads]: every element written.
 * Two launches. */
int vkn_wattn_bwd_f32(const float* qkv, const float* qkv_bias, const float* bias_table, const float* dout, float* dqkv, float* dqkv_bias,
                      float* dbias_table, int B, int H, int W, int heads, int window, int shift, float scale, void* workspace,
                      size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_WATTN_TRAIN_H */
