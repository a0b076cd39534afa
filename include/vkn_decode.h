/* vkn_decode.h — fifth part of the C ABI of libvkn.so (behind vkn.h, vkn_track.h, vkn_track_train.h, vkn_gt.h): the mask decode on a
 * workgroup budget.  Conventions as in vkn.h. */
#ifndef VKN_DECODE_H
#define VKN_DECODE_H
#include "vkn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- vkn_mask_decode_planes_x (the MFMA decode on pre-split kernel planes, see vkn.h) on a workgroup BUDGET:
 *      at most max_workgroups workgroups in the launch (0 = the default split; fewer than B cannot be
 *      honoured: one workgroup per frame then).  Every frame gets the same number of workgroups, each an equal share of P rounded up
 *      to 512 pixels (vkn_decode_px_per_wg); the budget counts the WHOLE grid, so the few-frame row split over blockIdx.z
 *      (which multiplies it) is dropped where the grid would not fit with it.  The output is bit-identical whatever the split: an accumulator sees the same MFMA
 *      sequence for its pixel.  The head call uses it to leave CUs free for the tracking link beside its last decode
 *      (VKN_FLAG_LINK_RESERVE); tests force splits at small sizes through it.  Arguments otherwise as for vkn_mask_decode_planes_f32. */
int vkn_mask_decode_planes_wg_f32(const float* x, const void* kf_hi, const void* kf_lo, const float* bias, float* out, int B,
                                  int N, int C, int P, int max_workgroups, void* stream);
/*      ... with x stored as x_dtype (VKN_X_F32 / VKN_X_F16 / VKN_X_BF16) */
int vkn_mask_decode_planes_wg_x(const void* x, int x_dtype, const void* kf_hi, const void* kf_lo, const float* bias, float* out, int B,
                                int N, int C, int P, int max_workgroups, void* stream);
/*      The split itself (pure host arithmetic, no device): pixels per decode workgroup for B frames of P pixels under the budget;
 *      the launch then has B * ceil(P / px_per_wg) workgroups.  max_workgroups == 0, or a budget the default grid already meets,
 *      returns the default: ceil(B * P / 256) rounded up to 512 (one workgroup per CU from 256 * 512 pixels on).  < 0: VKN_E_ARG. */
int vkn_decode_px_per_wg(int B, int P, int max_workgroups);

#ifdef __cplusplus
}
#endif
#endif
