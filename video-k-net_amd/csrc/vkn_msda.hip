// vkn_msda.hip — the sampling core of multi-scale deformable attention (include/vkn_msda.h) for gfx950.
//
// One GROUP of G = D / 4 lanes owns one (b, q, m): every lane holds four of the head's D channels, so a corner read is ONE coalesced
// segment of D * 4 bytes (128 at D = 32) and a wave of 64 lanes covers 64 / G heads of a query at once (all eight at the shipped
// M = 8, D = 32).  The 3 L P floats of the (q, m) — offsets and logits — are read by every lane of the group from the same addresses
// (one transaction per group), the softmax runs in registers: a first walk for the maximum, then e = exp(logit - max) per point,
// the sum of e beside the weighted samples, ONE division at the end.  No LDS, no workspace, no atomics.
//
// Safety (the header's contract): a point is tested with the four float comparisons FIRST; a point that fails them has its
// coordinates replaced by 0 before floor / float -> int, its corners are clamped into the level before an address is formed, and the
// loaded values are dropped by a select (never multiplied by a zero weight: 0 * inf would be a NaN).  Every load therefore lies
// inside the level's [H][W] block whatever the offsets hold.  That arithmetic is msda::point / msda::pick of vkn_msda_point.h, which
// the backward (vkn_msda_bwd.hip) shares.
#include "vkn_msda_point.h"

namespace {

using MsdaLevels = msda::Levels;

template <int G>
__global__ __launch_bounds__(256) void k_msda_sample(const float* __restrict__ value, const float* __restrict__ off, int ld_off,
                                                     const float* __restrict__ logits, int ld_logits, const float* __restrict__ ref,
                                                     float* __restrict__ out, MsdaLevels lv, int S, int Q, int M, int L, int P,
                                                     int ngroups) {
    const int g = blockIdx.x * (256 / G) + (int)threadIdx.x / G;
    if (g >= ngroups) return;
    const int j = (int)threadIdx.x % G;
    const int m = g % M, bq = g / M, q = bq % Q, b = bq / Q;
    const int LP = L * P;
    const size_t C = (size_t)M * G * 4;                                   // floats of one position of `value`, of one row of `out`
    const float* lg = logits + (size_t)bq * ld_logits + (size_t)m * LP;
    const float* of = off + (size_t)bq * ld_off + (size_t)m * LP * 2;
    float mx = lg[0];
    for (int i = 1; i < LP; ++i) mx = fmaxf(mx, lg[i]);
    const float* vb = value + (size_t)b * S * C + (size_t)m * (G * 4) + j * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    for (int l = 0; l < L; ++l) {
        const int H = lv.H[l], W = lv.W[l];
        const float rx = ref[((size_t)q * L + l) * 2], ry = ref[((size_t)q * L + l) * 2 + 1];
        const float* vl = vb + (size_t)lv.start[l] * C;
#pragma unroll 2
        for (int p = 0; p < P; ++p) {
            const int i = l * P + p;
            const float e = expf(lg[i] - mx);
            den += e;
            const msda::Point pt = msda::point(rx, ry, of[2 * i], of[2 * i + 1], H, W);
            const float lw = pt.lw, lh = pt.lh, hw = pt.hw, hh = pt.hh;
            const f32x4 v1 = msda::pick(pt.in1, vl + ((size_t)pt.ya * W + pt.xa) * C);
            const f32x4 v2 = msda::pick(pt.in2, vl + ((size_t)pt.ya * W + pt.xb) * C);
            const f32x4 v3 = msda::pick(pt.in3, vl + ((size_t)pt.yb * W + pt.xa) * C);
            const f32x4 v4 = msda::pick(pt.in4, vl + ((size_t)pt.yb * W + pt.xb) * C);
            const f32x4 s = (hh * hw) * v1 + (hh * lw) * v2 + (lh * hw) * v3 + (lh * lw) * v4;
            acc += e * s;
        }
    }
    *reinterpret_cast<f32x4*>(out + (size_t)bq * C + (size_t)m * (G * 4) + j * 4) = acc / den;
}

}  // namespace

extern "C" int vkn_msda_sample_f32(const float* value, const float* off, int ld_off, const float* logits, int ld_logits, const float* ref,
                                   const int* shapes, float* out, int B, int Q, int M, int D, int L, int P, void* stream) {
    if (!value || !off || !logits || !ref || !shapes || !out) return VKN_E_ARG;
    MsdaLevels lv;
    long long S = 0;
    if (const int rc = msda::check(shapes, B, Q, M, D, L, P, ld_off, ld_logits, &lv, &S)) return rc;
    const long long rows = (long long)B * Q;
    if (!vkn_aligned(value, 16) || !vkn_aligned(off, 16) || !vkn_aligned(logits, 16) || !vkn_aligned(ref, 16) || !vkn_aligned(out, 16))
        return VKN_E_ALIGN;
    const int ngroups = (int)(rows * M);                                  // < 2^31 / (4 D)
    hipStream_t st = static_cast<hipStream_t>(stream);
#define MSDA_LAUNCH(GV)                                                                                                              \
    hipLaunchKernelGGL((k_msda_sample<GV>), dim3((ngroups + 256 / GV - 1) / (256 / GV)), dim3(256), 0, st, value, off, ld_off, logits, \
                       ld_logits, ref, out, lv, (int)S, Q, M, L, P, ngroups)
    if (D == 16) MSDA_LAUNCH(4);
    else if (D == 32) MSDA_LAUNCH(8);
    else MSDA_LAUNCH(16);
#undef MSDA_LAUNCH
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}
