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
// inside the level's [H][W] block whatever the offsets hold.
#include "../../include/vkn_msda.h"
#include "vkn_common.h"

namespace {

struct MsdaLevels {
    int H[VKN_MSDA_MAX_LEVELS], W[VKN_MSDA_MAX_LEVELS], start[VKN_MSDA_MAX_LEVELS];
};

__device__ __forceinline__ f32x4 msda_pick(bool keep, const float* p) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    return keep ? v : z;
}

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
        const float Hf = (float)H, Wf = (float)W;
        const float rx = ref[((size_t)q * L + l) * 2], ry = ref[((size_t)q * L + l) * 2 + 1];
        const float* vl = vb + (size_t)lv.start[l] * C;
#pragma unroll 2
        for (int p = 0; p < P; ++p) {
            const int i = l * P + p;
            const float e = expf(lg[i] - mx);
            den += e;
            const float x = (rx + of[2 * i] / Wf) * Wf - 0.5f, y = (ry + of[2 * i + 1] / Hf) * Hf - 0.5f;
            const bool ok = (y > -1.f) && (x > -1.f) && (y < Hf) && (x < Wf);          // false for a NaN
            const float xs = ok ? x : 0.f, ys = ok ? y : 0.f;                           // in (-1, W) x (-1, H) from here on
            const float xf = floorf(xs), yf = floorf(ys);
            const int x0 = (int)xf, y0 = (int)yf;                                       // in [-1, W - 1], [-1, H - 1]
            const float lw = xs - xf, lh = ys - yf, hw = 1.f - lw, hh = 1.f - lh;
            const bool xa_in = x0 >= 0, xb_in = x0 + 1 <= W - 1, ya_in = y0 >= 0, yb_in = y0 + 1 <= H - 1;
            const int xa = x0 < 0 ? 0 : x0, xb = x0 + 1 > W - 1 ? W - 1 : x0 + 1;       // clamped: inside the level in any case
            const int ya = y0 < 0 ? 0 : y0, yb = y0 + 1 > H - 1 ? H - 1 : y0 + 1;
            const f32x4 v1 = msda_pick(ok && ya_in && xa_in, vl + ((size_t)ya * W + xa) * C);
            const f32x4 v2 = msda_pick(ok && ya_in && xb_in, vl + ((size_t)ya * W + xb) * C);
            const f32x4 v3 = msda_pick(ok && yb_in && xa_in, vl + ((size_t)yb * W + xa) * C);
            const f32x4 v4 = msda_pick(ok && yb_in && xb_in, vl + ((size_t)yb * W + xb) * C);
            const f32x4 s = (hh * hw) * v1 + (hh * lw) * v2 + (lh * hw) * v3 + (lh * lw) * v4;
            acc += e * s;
        }
    }
    *reinterpret_cast<f32x4*>(out + (size_t)bq * C + (size_t)m * (G * 4) + j * 4) = acc / den;
}

}  // namespace

extern "C" int vkn_msda_sample_f32(const float* value, const float* off, int ld_off, const float* logits, int ld_logits, const float* ref,
                                   const int* shapes, float* out, int B, int Q, int M, int D, int L, int P, void* stream) {
    if (!value || !off || !logits || !ref || !shapes || !out || B <= 0 || Q <= 0 || M <= 0 || D <= 0 || L <= 0 || P <= 0) return VKN_E_ARG;
    const long long mlp = (long long)M * L * P;
    if (ld_off < 2 * mlp || ld_logits < mlp) return VKN_E_ARG;
    const int nl = L < VKN_MSDA_MAX_LEVELS ? L : VKN_MSDA_MAX_LEVELS;
    for (int l = 0; l < nl; ++l)
        if (shapes[2 * l] <= 0 || shapes[2 * l + 1] <= 0) return VKN_E_ARG;
    if (D != 16 && D != 32 && D != 64) return VKN_E_SHAPE;
    if (((long long)M * D) % 32 != 0 || (long long)M * D > VKN_MSDA_MAX_CHANNELS) return VKN_E_SHAPE;
    if (L > VKN_MSDA_MAX_LEVELS || P > VKN_MSDA_MAX_POINTS) return VKN_E_SHAPE;
    const long long lim = 1ll << 31;
    MsdaLevels lv{};
    long long S = 0;
    for (int l = 0; l < L; ++l) {
        lv.H[l] = shapes[2 * l];
        lv.W[l] = shapes[2 * l + 1];
        lv.start[l] = (int)S;
        S += (long long)lv.H[l] * lv.W[l];
        if (S * 4 >= lim) return VKN_E_SHAPE;
    }
    const long long C = (long long)M * D, rows = (long long)B * Q;
    if (rows >= lim || (long long)B * S * C * 4 >= lim || rows * C * 4 >= lim || rows * ld_off * 4 >= lim || rows * ld_logits * 4 >= lim ||
        (long long)Q * L * 2 * 4 >= lim)
        return VKN_E_SHAPE;
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
