/* vkn_swin.h — C ABI of libvkn.so, a backbone part: the (shifted-)window attention core of `SwinTransformerDIY`
 * (swin/swin_transformer.py:79-180 and :245-305), everything between the `qkv` Linear and the `proj` Linear of one block.
 *
 * Conventions and error codes are those of vkn.h: `extern "C"`, DEVICE pointers into caller-owned fp32 memory, 16-byte aligned, nothing
 * allocated inside, work enqueued asynchronously on `stream`, no host synchronisation (capturable), 0 = VKN_OK.  The entry refuses before
 * any launch, in this order: NULL pointers / counts <= 0 -> VKN_E_ARG, a shape outside the envelope -> VKN_E_SHAPE, a misaligned
 * pointer -> VKN_E_ALIGN.  No workspace, no atomics: every sum has a fixed order, two runs on the same inputs are bitwise equal.
 *
 * The tokens stay where they are.  With Hp, Wp = H, W rounded up to multiples of `window`, the reference pads the [H][W] map to
 * [Hp][Wp], rolls it by -shift along both axes, cuts it into window x window tiles, attends inside each tile, and undoes all three.
 * Here those are index arithmetic: position s of the rolled map holds token (s + shift) mod E of the padded map, along each axis.
 * A token of the padded map outside [H][W] is a PAD token.  The reference pads after `norm1` and before `qkv`, so a pad token's q, k, v
 * are the bias of `qkv`: pad tokens are keys and values like any other (they are not masked in unshifted blocks), and are
 * synthesised here from `qkv_bias`.  Outputs of pad tokens are never written.
 *
 * For head m, query i and key j of one tile (y, x: row and column inside the tile)
 *     score[i][j] = (q_i scale) . k_j + bias_table[rel(i, j)][m] + (shift > 0 && region(i) != region(j) ? VKN_SWIN_MASK : 0)
 *     rel(i, j)   = (y_i - y_j + window - 1) (2 window - 1) + (x_i - x_j + window - 1)          (= relative_position_index)
 *     region      = 3 r(row, Hp) + r(column, Wp) on the ROLLED map,  r(s, E) = s < E - window ? 0 : s < E - shift ? 1 : 2
 *     out_i       = sum_j softmax_j(score[i][.]) v_j          (maximum subtracted; summed in key order, divided by the sum last)
 * all in plain fp32 FMA.  The mask value is the reference's -100, not -inf (swin/swin_transformer.py:428-451).
 *
 * Envelope: head_dim = VKN_SWIN_HEAD_DIM (every shipped config: 128 / 4 ... 1536 / 48), 1 <= window, window^2 <=
 * VKN_SWIN_MAX_WINDOW_TOKENS, 0 <= shift < window, 1 <= heads <= VKN_SWIN_MAX_HEADS, every tensor below 2^31 bytes.
 *
 * Not built: a backward, another head_dim, attention dropout. */
#ifndef VKN_SWIN_H
#define VKN_SWIN_H
#include "vkn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VKN_SWIN_HEAD_DIM 32
#define VKN_SWIN_MAX_WINDOW_TOKENS 64     /* window^2: one query per lane of a wave */
#define VKN_SWIN_MAX_WINDOW 8
#define VKN_SWIN_MAX_HEADS 64
#define VKN_SWIN_MASK (-100)              /* added to a score whose two tokens lie in different regions of a shifted block */

/* 1 inside the envelope above (sizes included), else 0.  Asks the runtime nothing. */
int vkn_swin_window_attn_supported(int B, int H, int W, int heads, int window, int shift);

/* qkv        [B][H][W][3][heads][32]: the rows of `attn.qkv(norm1(x))` on the tokens as they are (not padded, shifted or partitioned);
 * qkv_bias   [3][heads][32], the bias of that Linear, or NULL = zeros (qkv_bias=False): what a pad token's k and v are;
 * bias_table [(2 window - 1)^2][heads]: relative_position_bias_table;
 * out        [B][H][W][heads 32]: the attention output in the same order, what `proj` takes.  Every element written.  One launch. */
int vkn_swin_window_attn_f32(const float* qkv, const float* qkv_bias, const float* bias_table, float* out, int B, int H, int W, int heads,
                             int window, int shift, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VKN_SWIN_H */
