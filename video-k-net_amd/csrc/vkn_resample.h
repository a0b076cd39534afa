// vkn_resample.h — the bilinear resampling rules that the joint panoptic merge (vkn_panoptic.hip) and the fused instance-mask rescale
// (vkn_instmask.hip) share: ATen's align_corners=False coefficients and its evaluation order, fp32.  There are no cross-file device symbols
// in this build, so the two device functions are shared as text: every source that includes this header compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// ATen's linear-interpolation coefficients, align_corners=False (aten/src/ATen/native/UpSample.h:
// area_pixel_compute_source_index + guard_index_and_lambda), fp32 opmath.
__device__ __forceinline__ void pan_coef(float scale, int dst, int in_size, int& i0, int& i1, float& lam) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = min((int)floorf(src), in_size - 1);
    lam = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
}

// value of one output pixel of a level from its input region in LDS (row pitch `pitch`), ATen's evaluation order:
// x first, then y; each as v0*w0 + v1*w1.  Region buffers carry one replicated column and row past their extent, so the
// second tap is always at +1 (ATen clamps it onto the first at the image border — same value, same arithmetic) and the two
// taps of a row are one ds_read2.
__device__ __forceinline__ float pan_lerp(const float* __restrict__ ldsf, int base, int pitch, int y0, float ly, int x0,
                                          float lx) {
    // `ldsf` is the dynamic-LDS base itself and every buffer is addressed by a word offset: a pointer selected at run time
    // (level 1 or 2 buffer) loses its address space and turns these reads into flat loads (measured: 2.5x slower)
    const int o = base + y0 * pitch + x0;
    const float wx0 = 1.f - lx, wy0 = 1.f - ly;
    const float r0 = ldsf[o] * wx0 + ldsf[o + 1] * lx;
    const float r1 = ldsf[o + pitch] * wx0 + ldsf[o + pitch + 1] * lx;
    return r0 * wy0 + r1 * ly;
}
