// vkn_msda_bwd.hip — backward of the sampling core of multi-scale deformable attention (include/vkn_msda_train.h) for gfx950, the
// forward being k_msda_sample of vkn_msda.hip.  Nothing of the forward is saved: the softmax (max walk, then the sum of
// e = exp(logit - max) in the forward's (l, p) order) and every point (msda::point of vkn_msda_point.h, the forward's own code) are
// recomputed.  Five launches and one memset:
//   * k_msda_bwd_absmax_part / _fin: max |dout| and, from it, the power of two 2^e of the fixed-point scatter (device side, no host read);
//   * k_msda_bwd_gather: dlogits and doff, in the FORWARD's layout — G = D / 4 lanes own one (b, q, m), four channels each, a corner
//     read is one coalesced segment.  The three sums over d of a point (G_i and the two offset gradients) run over the lane's four
//     channels, then across the group's lanes as an xor butterfly (G / 2, .., 1): a fixed order, the same value in every lane;
//   * k_msda_bwd_scatter: dvalue, ONE channel per lane, D lanes per (b, q, m): an atomic wave-instruction then touches whole
//     [M][D]-row segments of D int64 = 8 D contiguous bytes (256 at D = 32) instead of 32-byte pieces of many rows.  Each contribution
//     dout[d] w_i (corner weight) is rounded once to an integer, llrint(c 2^e), and added with a 64-bit integer atomic: integer
//     addition has no order, so the sum is the same on every run;
//   * k_msda_bwd_finish: dvalue = (float)acc 2^-e, every element.
// Safety: a corner's index is formed from msda::point's clamped coordinates and used only if the point passed the four comparisons
// and the corner lies inside, so no input value can produce an access outside `value` or the accumulator.  A non-finite dout or
// contribution ORs VKN_STATUS_RANGE into the status word and is never converted to an integer.
#include "../../include/vkn_msda_train.h"
#include "vkn_msda_point.h"
#include "vkn_convtile.h"

#include <algorithm>

#define MSDA_BWD_MAX_PART 256   // workgroups of the max |dout| pass
#define MSDA_BWD_KEEP 8         // VKN_MSDA_MAX_LEVELS * VKN_MSDA_MAX_POINTS / 4: the points one lane of the smallest group finishes

static_assert(VKN_MSDA_MAX_LEVELS * VKN_MSDA_MAX_POINTS <= MSDA_BWD_KEEP * 4, "a lane of a 4-lane group keeps L P / 4 points");

namespace {

// ------------------------------------------------------------------------------------------------ the power of two of the scatter
__global__ __launch_bounds__(256) void k_msda_bwd_absmax_part(const float* __restrict__ x, long long n, float* __restrict__ part,
                                                              unsigned* status) {
    float m = 0.f;
    unsigned bad = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float a = fabsf(x[i]);
        bad |= !(a < INFINITY);                                           // fmaxf drops a NaN: count it here
        m = fmaxf(m, a);
    }
    if (bad) atomicOr(status, (unsigned)VKN_STATUS_RANGE);
    const float mx = convtile::block_absmax(m);
    if (threadIdx.x == 0) part[blockIdx.x] = mx;
}

// sc = {2^e, 2^-e}, e the largest with mx * qp * 2^e < 2^62; {1, 1} for an all-zero or non-finite dout (the first pass flags the latter)
__global__ __launch_bounds__(256) void k_msda_bwd_absmax_fin(const float* __restrict__ part, int nblk, double qp, double* __restrict__ sc) {
    const float mx = convtile::block_absmax((int)threadIdx.x < nblk ? part[threadIdx.x] : 0.f);
    if (threadIdx.x != 0) return;
    int e = 0;
    if (mx > 0.f && mx < INFINITY) {
        int k;
        frexp((double)mx * qp, &k);                                       // exact product: 24 x 25 bits.  = f 2^k, f in [0.5, 1)
        e = 62 - k;                                                       // f 2^62 < 2^62 <= f 2^63
    }
    sc[0] = ldexp(1.0, e);                                                // |e| < 300: a double holds it
    sc[1] = ldexp(1.0, -e);
}

// ------------------------------------------------------------------------------------------------ dlogits and doff: gathers
__device__ __forceinline__ float dot4(const f32x4 a, const f32x4 b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }

template <int G>
__global__ __launch_bounds__(256) void k_msda_bwd_gather(const float* __restrict__ value, const float* __restrict__ off, int ld_off,
                                                         const float* __restrict__ logits, int ld_logits, const float* __restrict__ ref,
                                                         const float* __restrict__ dout, float* __restrict__ doff, int ld_doff,
                                                         float* __restrict__ dlogits, int ld_dlogits, msda::Levels lv, int S, int Q, int M,
                                                         int L, int P, int ngroups) {
    const int g0 = blockIdx.x * (256 / G) + (int)threadIdx.x / G;
    const bool live = g0 < ngroups;                                       // the same for the G lanes of a group; all stay for the butterfly
    const int g = live ? g0 : ngroups - 1;
    const int j = (int)threadIdx.x % G;
    const int m = g % M, bq = g / M, q = bq % Q, b = bq / Q;
    const int LP = L * P;
    const size_t C = (size_t)M * G * 4;
    const float* lg = logits + (size_t)bq * ld_logits + (size_t)m * LP;
    const float* of = off + (size_t)bq * ld_off + (size_t)m * LP * 2;
    float* dof = doff + (size_t)bq * ld_doff + (size_t)m * LP * 2;
    float* dlg = dlogits + (size_t)bq * ld_dlogits + (size_t)m * LP;
    float mx = lg[0];
    for (int i = 1; i < LP; ++i) mx = fmaxf(mx, lg[i]);
    float den = 0.f;
    for (int i = 0; i < LP; ++i) den += expf(lg[i] - mx);                 // the forward's sum, in its order
    const float* vb = value + (size_t)b * S * C + (size_t)m * (G * 4) + j * 4;
    const f32x4 go = *reinterpret_cast<const f32x4*>(dout + (size_t)bq * C + (size_t)m * (G * 4) + j * 4);
    float keep[MSDA_BWD_KEEP];                                            // G_i of the points i = s G + j
#pragma unroll
    for (int s = 0; s < MSDA_BWD_KEEP; ++s) keep[s] = 0.f;
    float T = 0.f;                                                        // sum_j w_j G_j
    for (int l = 0; l < L; ++l) {
        const int H = lv.H[l], W = lv.W[l];
        const float rx = ref[((size_t)q * L + l) * 2], ry = ref[((size_t)q * L + l) * 2 + 1];
        const float* vl = vb + (size_t)lv.start[l] * C;
        for (int p = 0; p < P; ++p) {
            const int i = l * P + p;
            const float w = expf(lg[i] - mx) / den;
            const msda::Point pt = msda::point(rx, ry, of[2 * i], of[2 * i + 1], H, W);
            const float lw = pt.lw, lh = pt.lh, hw = pt.hw, hh = pt.hh;
            const f32x4 v1 = msda::pick(pt.in1, vl + ((size_t)pt.ya * W + pt.xa) * C);
            const f32x4 v2 = msda::pick(pt.in2, vl + ((size_t)pt.ya * W + pt.xb) * C);
            const f32x4 v3 = msda::pick(pt.in3, vl + ((size_t)pt.yb * W + pt.xa) * C);
            const f32x4 v4 = msda::pick(pt.in4, vl + ((size_t)pt.yb * W + pt.xb) * C);
            const f32x4 s = (hh * hw) * v1 + (hh * lw) * v2 + (lh * hw) * v3 + (lh * lw) * v4;
            float Gi = dot4(go, s);
            float gx = dot4(go, hh * (v2 - v1) + lh * (v4 - v3));
            float gy = dot4(go, hw * (v3 - v1) + lw * (v4 - v2));
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {                         // partners stay inside the group: its lanes are G-aligned
                Gi += __shfl_xor(Gi, o, G);
                gx += __shfl_xor(gx, o, G);
                gy += __shfl_xor(gy, o, G);
            }
            T += w * Gi;
            if (live && j == 0) {
                dof[2 * i] = pt.ok ? w * gx : 0.f;                        // d x / d off_x = 1; a point that fails the test: exactly 0
                dof[2 * i + 1] = pt.ok ? w * gy : 0.f;
            }
#pragma unroll
            for (int s2 = 0; s2 < MSDA_BWD_KEEP; ++s2) keep[s2] = (i == s2 * G + j) ? Gi : keep[s2];
        }
    }
#pragma unroll
    for (int s = 0; s < MSDA_BWD_KEEP; ++s) {
        const int i = s * G + j;
        if (live && i < LP) dlg[i] = (expf(lg[i] - mx) / den) * (keep[s] - T);      // L P = 1: w = 1, T = G_0, exactly 0
    }
}

// ------------------------------------------------------------------------------------------------ dvalue: the fixed-point scatter
__device__ __forceinline__ void msda_bwd_add(bool in, unsigned long long* cell, float c, double scale, unsigned& bad) {
    if (!in) return;                                                      // a corner outside, or a point that failed: no address is used
    const double t = (double)c * scale;
    if (fabs(t) < 0x1p62) {                                               // false for a NaN: never converted
        const long long v = llrint(t);
        if (v != 0) atomicAdd(cell, (unsigned long long)v);               // two's complement: the wrap-around sum is the signed sum
    } else {
        bad = 1;
    }
}

template <int D>
__global__ __launch_bounds__(256) void k_msda_bwd_scatter(const float* __restrict__ off, int ld_off, const float* __restrict__ logits,
                                                          int ld_logits, const float* __restrict__ ref, const float* __restrict__ dout,
                                                          msda::Levels lv, int S, int Q, int M, int L, int P, int ngroups,
                                                          const double* __restrict__ sc, unsigned long long* __restrict__ acc,
                                                          unsigned* status) {
    const int g = blockIdx.x * (256 / D) + (int)threadIdx.x / D;
    if (g >= ngroups) return;
    const int d = (int)threadIdx.x % D;
    const int m = g % M, bq = g / M, q = bq % Q, b = bq / Q;
    const int LP = L * P;
    const size_t C = (size_t)M * D;
    const float* lg = logits + (size_t)bq * ld_logits + (size_t)m * LP;
    const float* of = off + (size_t)bq * ld_off + (size_t)m * LP * 2;
    float mx = lg[0];
    for (int i = 1; i < LP; ++i) mx = fmaxf(mx, lg[i]);
    float den = 0.f;
    for (int i = 0; i < LP; ++i) den += expf(lg[i] - mx);
    const float go = dout[(size_t)bq * C + (size_t)m * D + d];
    const double scale = sc[0];
    unsigned long long* ab = acc + (size_t)b * S * C + (size_t)m * D + d;
    unsigned bad = 0;
    for (int l = 0; l < L; ++l) {
        const int H = lv.H[l], W = lv.W[l];
        const float rx = ref[((size_t)q * L + l) * 2], ry = ref[((size_t)q * L + l) * 2 + 1];
        unsigned long long* al = ab + (size_t)lv.start[l] * C;
        for (int p = 0; p < P; ++p) {
            const int i = l * P + p;
            const float gw = go * (expf(lg[i] - mx) / den);
            const msda::Point pt = msda::point(rx, ry, of[2 * i], of[2 * i + 1], H, W);
            msda_bwd_add(pt.in1, al + ((size_t)pt.ya * W + pt.xa) * C, gw * (pt.hh * pt.hw), scale, bad);
            msda_bwd_add(pt.in2, al + ((size_t)pt.ya * W + pt.xb) * C, gw * (pt.hh * pt.lw), scale, bad);
            msda_bwd_add(pt.in3, al + ((size_t)pt.yb * W + pt.xa) * C, gw * (pt.lh * pt.hw), scale, bad);
            msda_bwd_add(pt.in4, al + ((size_t)pt.yb * W + pt.xb) * C, gw * (pt.lh * pt.lw), scale, bad);
        }
    }
    if (bad) atomicOr(status, (unsigned)VKN_STATUS_RANGE);
}

__global__ __launch_bounds__(256) void k_msda_bwd_finish(const long long* __restrict__ acc, long long n, const double* __restrict__ sc,
                                                         float* __restrict__ dvalue) {
    const double inv = sc[1];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        dvalue[i] = (float)((double)(float)acc[i] * inv);                 // ONE rounding, int64 -> fp32; the power of two is exact
}

struct BwdWs {
    size_t sc, part, acc, total;
    long long n;                                                          // accumulator elements
};

BwdWs bwd_carve(int B, long long S, int M, int D) {
    BwdWs w;
    w.n = (long long)B * S * M * D;
    w.sc = 256;
    w.part = 512;
    w.acc = VKN_MSDA_BWD_WS_HEAD;
    w.total = w.acc + convtile::align256((size_t)w.n * sizeof(long long));
    return w;
}
static_assert(512 + MSDA_BWD_MAX_PART * sizeof(float) == VKN_MSDA_BWD_WS_HEAD, "the workspace's head");

// the forward's envelope for the operands AND for the gradients' strides, then the scatter's own limit
int bwd_check(const int* shapes, int B, int Q, int M, int D, int L, int P, long long ld_off, long long ld_logits, long long ld_doff,
              long long ld_dlogits, msda::Levels* lv, long long* S) {
    const int rc1 = msda::check(shapes, B, Q, M, D, L, P, ld_off, ld_logits, lv, S);
    const int rc2 = msda::check(shapes, B, Q, M, D, L, P, ld_doff, ld_dlogits, lv, S);
    if (rc1 == VKN_E_ARG || rc2 == VKN_E_ARG) return VKN_E_ARG;
    if (rc1 != VKN_OK || rc2 != VKN_OK) return VKN_E_SHAPE;
    if ((long long)Q * P > VKN_MSDA_BWD_MAX_QP) return VKN_E_SHAPE;
    return VKN_OK;
}

}  // namespace

extern "C" {

size_t vkn_msda_bwd_workspace_bytes(const int* shapes, int B, int Q, int M, int D, int L, int P) {
    if (!shapes) return 0;
    msda::Levels lv;
    long long S = 0;
    const long long mlp = (long long)M * L * P;
    if (bwd_check(shapes, B, Q, M, D, L, P, 2 * mlp, mlp, 2 * mlp, mlp, &lv, &S) != VKN_OK) return 0;
    return bwd_carve(B, S, M, D).total;
}

int vkn_msda_sample_bwd_f32(const float* value, const float* off, int ld_off, const float* logits, int ld_logits, const float* ref,
                            const int* shapes, const float* dout, float* dvalue, float* doff, int ld_doff, float* dlogits,
                            int ld_dlogits, int B, int Q, int M, int D, int L, int P, void* ws, size_t ws_bytes, void* stream) {
    if (!value || !off || !logits || !ref || !shapes || !dout || !dvalue || !doff || !dlogits) return VKN_E_ARG;
    msda::Levels lv;
    long long S = 0;
    if (const int rc = bwd_check(shapes, B, Q, M, D, L, P, ld_off, ld_logits, ld_doff, ld_dlogits, &lv, &S)) return rc;
    const BwdWs w = bwd_carve(B, S, M, D);
    if (!ws || ws_bytes < w.total) return VKN_E_WORKSPACE;
    for (const void* p : {(const void*)value, (const void*)off, (const void*)logits, (const void*)ref, (const void*)dout,
                          (const void*)dvalue, (const void*)doff, (const void*)dlogits, (const void*)ws})
        if (!vkn_aligned(p, 16)) return VKN_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    unsigned* status = reinterpret_cast<unsigned*>(base);
    double* sc = reinterpret_cast<double*>(base + w.sc);
    float* part = reinterpret_cast<float*>(base + w.part);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(base + w.acc);
    const long long rows = (long long)B * Q, nout = rows * M * D;
    const int ngroups = (int)(rows * M);
    if (hipMemsetAsync(acc, 0, (size_t)w.n * sizeof(long long), st) != hipSuccess) return VKN_E_LAUNCH;
    const int nblk = (int)std::min<long long>((nout + 255) / 256, MSDA_BWD_MAX_PART);
    hipLaunchKernelGGL(k_msda_bwd_absmax_part, dim3(nblk), dim3(256), 0, st, dout, nout, part, status);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_msda_bwd_absmax_fin, dim3(1), dim3(256), 0, st, part, nblk, (double)((long long)Q * P), sc);
    VKN_CHECK_LAUNCH();
#define MSDA_BWD_LAUNCH(DV)                                                                                                            \
    do {                                                                                                                               \
        hipLaunchKernelGGL((k_msda_bwd_gather<DV / 4>), dim3((ngroups + 1024 / DV - 1) / (1024 / DV)), dim3(256), 0, st, value, off,   \
                           ld_off, logits, ld_logits, ref, dout, doff, ld_doff, dlogits, ld_dlogits, lv, (int)S, Q, M, L, P, ngroups); \
        hipLaunchKernelGGL((k_msda_bwd_scatter<DV>), dim3((ngroups + 256 / DV - 1) / (256 / DV)), dim3(256), 0, st, off, ld_off,       \
                           logits, ld_logits, ref, dout, lv, (int)S, Q, M, L, P, ngroups, sc, acc, status);                            \
    } while (0)
    if (D == 16) MSDA_BWD_LAUNCH(16);
    else if (D == 32) MSDA_BWD_LAUNCH(32);
    else MSDA_BWD_LAUNCH(64);
#undef MSDA_BWD_LAUNCH
    VKN_CHECK_LAUNCH();
    const int fblk = (int)std::min<long long>((w.n + 255) / 256, 8192);
    hipLaunchKernelGGL(k_msda_bwd_finish, dim3(fblk), dim3(256), 0, st, reinterpret_cast<const long long*>(acc), w.n, sc, dvalue);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

}  // extern "C"
