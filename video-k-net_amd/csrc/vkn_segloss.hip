// vkn_segloss.hip — the dense semantic loss of the kernel-initialisation head from the LOW-RES logits (include/vkn_seg_loss.h): the
// painted one-byte target map, the focal / soft-max loss and its backward.  The up-scaled logits [B][ncls][S h][S w] — the widest
// tensor of a training step — exist in registers only.
//
// Geometry (k_ml_fwd_lr / k_ml_bwd_lr of vkn_loss.hip): a thread owns one S x S block of up-scaled pixels SHIFTED by S / 2, rows
// S bi + S / 2 .., bi = -1 .. h - 1.  Every pixel of the block lies between the low-res rows bi, bi + 1 and columns bj, bj + 1 (clamped
// at the borders) with the compile-time weights (a + 0.5) / S, so a class plane costs the block FOUR loads.  At S = 1 the block is the
// pixel (bi, bj) itself with weight 0: the identity.  A workgroup is SEG_NW waves (block rows) x 64 lanes (block columns).
#include "../../include/vkn_seg_loss.h"
#include "vkn_common.h"

namespace {

constexpr int SEG_NW = 4;                      // waves (block rows) per workgroup of the loss kernels
constexpr int SEG_THREADS = 64 * SEG_NW;
constexpr int SEG_HEADER = 64;                 // bytes in front of the partial sums: the scale of the loss
constexpr int ST_ROWS = 4, ST_COLS = 64 * 4;   // the target kernel: a wave per row, 4 neighbouring pixels per lane
constexpr int ST_CHUNK = 256;                  // layers staged in LDS at a time

struct SegBatch { VknSegImage img[VKN_SEG_MAX_IMAGES]; };

// --------------------------------------------------------------------------------------------------------------------- targets
// grid (ceil(W / ST_COLS), ceil(H / ST_ROWS), B).  The layers of the image — n_sem stuff masks, then the Np proposal rows — are staged
// in LDS in chunks of ST_CHUNK as (plane, label); label -1: the row paints nothing.  A thread walks them from the LAST one down and
// keeps, per pixel, the first layer that covers it.
__global__ __launch_bounds__(256) void k_seg_targets(SegBatch batch, int H, int W, int ncls, unsigned char* __restrict__ tgt,
                                                     int* __restrict__ dense_pos, int* __restrict__ status) {
    __shared__ const float* s_plane[ST_CHUNK];
    __shared__ int s_label[ST_CHUNK];
    __shared__ int s_cnt[ST_ROWS];
    const VknSegImage& im = batch.img[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int y = blockIdx.y * ST_ROWS + wv, x0 = (blockIdx.x * 64 + lane) * 4;
    const bool inside = y < H && x0 < W;
    const size_t P = (size_t)H * W;
    const size_t e0 = inside ? (size_t)y * W + x0 : 0;
    const int nx = inside ? min(4, W - x0) : 0;
    const int n_sem = im.sem ? im.n_sem : 0;
    const int layers = n_sem + im.Np;
    int t[4] = {ncls, ncls, ncls, ncls};
    unsigned open = inside ? (1u << nx) - 1u : 0u;           // the pixels no layer has covered yet
    bool bad = false;
    for (int hi = layers; hi > 0; hi -= ST_CHUNK) {
        const int lo = max(hi - ST_CHUNK, 0);
        if (lo + tid < hi) {
            const int L = lo + tid;
            const float* plane = nullptr;
            long long label = -1;
            if (L < n_sem) {
                plane = im.sem + (size_t)L * P;
                label = im.sem_cls[L];
            } else {
                const long long k = im.gt_inds[L - n_sem];
                if (k > (long long)im.G) bad = true;
                else if (k > 0) {
                    plane = im.masks + (size_t)(k - 1) * P;
                    label = im.labels[k - 1];
                }
            }
            if (plane && (label < 0 || label >= ncls)) {
                bad = true;
                label = ncls;
            }
            s_plane[tid] = plane;
            s_label[tid] = plane ? (int)label : -1;
        }
        __syncthreads();
        for (int k = hi - lo - 1; k >= 0 && open; --k) {
            const int label = s_label[k];
            if (label < 0) continue;
            const float* p = s_plane[k] + e0;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (nx == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                const float4 q = *reinterpret_cast<const float4*>(p);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < nx) v[e] = p[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (((open >> e) & 1u) && v[e] != 0.f) {
                    t[e] = label;
                    open &= ~(1u << e);
                }
        }
        __syncthreads();
    }
    int cnt = 0;
    if (inside) {
        unsigned char* out = tgt + (size_t)blockIdx.z * P + e0;
        if (nx == 4 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
            *reinterpret_cast<unsigned*>(out) = (unsigned)t[0] | ((unsigned)t[1] << 8) | ((unsigned)t[2] << 16) | ((unsigned)t[3] << 24);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < nx) out[e] = (unsigned char)t[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) cnt += (e < nx && t[e] < ncls) ? 1 : 0;
    }
    if (bad && blockIdx.x == 0 && blockIdx.y == 0) atomicOr(status, (int)VKN_STATUS_RANGE);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    if (tid == 0) {
        const int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (total) atomicAdd(dense_pos, total);
    }
}

// ------------------------------------------------------------------------------------------------------------- the block geometry
template <int S>
struct Blk {
    static constexpr int OFF = S / 2;
    // weight of the SECOND tap of pixel a of the block ((a + 0.5) / S; 0 at S = 1)
    __device__ static constexpr float l(int a) { return S == 1 ? 0.f : ((float)a + 0.5f) / (float)S; }
};

struct Taps { size_t o00, o01, o10, o11; };

// the four clamped low-res taps of block (bi, bj) as element offsets inside a class plane
__device__ __forceinline__ Taps seg_taps(int bi, int bj, int h, int w) {
    const int r0 = min(max(bi, 0), h - 1), r1 = min(max(bi + 1, 0), h - 1), c0 = min(max(bj, 0), w - 1), c1 = min(max(bj + 1, 0), w - 1);
    return Taps{(size_t)r0 * w + c0, (size_t)r0 * w + c1, (size_t)r1 * w + c0, (size_t)r1 * w + c1};
}

// z[a][c] of the block from its four taps: the same expression in every kernel, so that forward and backward see the same logits
template <int S>
__device__ __forceinline__ void seg_logits(const float* __restrict__ plane, const Taps& tp, float (&z)[S][S]) {
    const float v00 = plane[tp.o00], v01 = plane[tp.o01], v10 = plane[tp.o10], v11 = plane[tp.o11];
    float h0[S], h1[S];
#pragma unroll
    for (int c = 0; c < S; ++c) {
        const float lx = Blk<S>::l(c);
        h0[c] = __fmaf_rn(lx, v01, __fmul_rn(1.f - lx, v00));
        h1[c] = __fmaf_rn(lx, v11, __fmul_rn(1.f - lx, v10));
    }
#pragma unroll
    for (int a = 0; a < S; ++a) {
        const float ly = Blk<S>::l(a);
#pragma unroll
        for (int c = 0; c < S; ++c) z[a][c] = __fmaf_rn(ly, h1[c], __fmul_rn(1.f - ly, h0[c]));
    }
}

// which pixels of the block lie inside the up-scaled map (bit a * S + c), and the block's target bytes (row a: byte c; ncls elsewhere)
template <int S>
__device__ __forceinline__ unsigned seg_block(const unsigned char* __restrict__ tgt, int bi, int bj, int h, int w, int ncls,
                                              unsigned (&tb)[S]) {
    const int H = S * h, W = S * w, Y0 = S * bi + Blk<S>::OFF, X0 = S * bj + Blk<S>::OFF;
    unsigned vmask = 0;
#pragma unroll
    for (int a = 0; a < S; ++a) {
        tb[a] = 0;
#pragma unroll
        for (int c = 0; c < S; ++c) {
            const int Y = Y0 + a, X = X0 + c;
            const bool in = bi <= h - 1 && bj <= w - 1 && Y >= 0 && Y < H && X >= 0 && X < W;
            unsigned t = (unsigned)ncls;
            if (in) {
                t = tgt[(size_t)Y * W + X];
                vmask |= 1u << (a * S + c);
            }
            tb[a] |= t << (8 * c);
        }
    }
    return vmask;
}

// mmdet's py_sigmoid_focal_loss element and its derivative (k_focal of vkn_loss.hip): t is 0 or 1
__device__ __forceinline__ float seg_pow(float pt, float gamma, bool g2) { return g2 ? pt * pt : powf(pt, gamma); }

__device__ __forceinline__ float seg_focal(float v, float t, float alpha, float gamma, bool g2) {
    const float e = expf(-fabsf(v));
    const float p = v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    const float bce = fmaxf(v, 0.f) - v * t + log1pf(e);
    const float pt = (1.f - p) * t + p * (1.f - t);
    const float at = alpha * t + (1.f - alpha) * (1.f - t);
    return bce * at * seg_pow(pt, gamma, g2);
}

__device__ __forceinline__ float seg_focal_dz(float v, float t, float alpha, float gamma, bool g2) {
    const float e = expf(-fabsf(v));
    const float p = v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    const float bce = fmaxf(v, 0.f) - v * t + log1pf(e);
    const float pt = (1.f - p) * t + p * (1.f - t);
    const float at = alpha * t + (1.f - alpha) * (1.f - t);
    const float ptg = seg_pow(pt, gamma, g2);
    const float dp = g2 ? 2.f * pt : (pt > 0.f ? gamma * powf(pt, gamma - 1.f) : 0.f);
    return at * ((p - t) * ptg + bce * dp * p * (1.f - p) * (1.f - 2.f * t));
}

// --------------------------------------------------------------------------------------------------------------------- forward
// grid (ceil((w + 1) / 64), ceil((h + 1) / SEG_NW), B).  partial [gridDim.z][gridDim.y][gridDim.x] fp64; CE: ml [B][S h][S w] float2 =
// (max, log-sum) of the pixel's soft-max, log-sum = +inf on an ignored pixel (its soft-max term in the backward is exactly 0).
template <int S, int MODE>
__global__ __launch_bounds__(SEG_THREADS) void k_seg_fwd(const float* __restrict__ low, const unsigned char* __restrict__ tgt, int ncls,
                                                         int h, int w, float alpha, float gamma, double* __restrict__ partial,
                                                         float2* __restrict__ ml) {
    __shared__ double red[SEG_NW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.z;
    const int bi = (int)blockIdx.y * SEG_NW - 1 + wv, bj = (int)blockIdx.x * 64 - 1 + lane;
    const size_t lp = (size_t)h * w, P = lp * S * S;
    const float* lb = low + (size_t)b * ncls * lp;
    unsigned tb[S];
    const unsigned vmask = seg_block<S>(tgt + (size_t)b * P, bi, bj, h, w, ncls, tb);
    const Taps tp = seg_taps(bi, bj, h, w);
    double acc = 0.0;
    float z[S][S];
    if (vmask) {
        if (MODE == VKN_SEG_LOSS_FOCAL) {
            const bool g2 = gamma == 2.f;
            for (int c = 0; c < ncls; ++c) {
                seg_logits<S>(lb + (size_t)c * lp, tp, z);
                float s = 0.f;
#pragma unroll
                for (int a = 0; a < S; ++a)
#pragma unroll
                    for (int q = 0; q < S; ++q) {
                        const float t = ((tb[a] >> (8 * q)) & 255u) == (unsigned)c ? 1.f : 0.f;
                        const float v = seg_focal(z[a][q], t, alpha, gamma, g2);
                        s += ((vmask >> (a * S + q)) & 1u) ? v : 0.f;
                    }
                acc += (double)s;
            }
        } else {
            float m[S][S], s[S][S], zt[S][S];
#pragma unroll
            for (int a = 0; a < S; ++a)
#pragma unroll
                for (int q = 0; q < S; ++q) { m[a][q] = -INFINITY; s[a][q] = 0.f; zt[a][q] = 0.f; }
            for (int c = 0; c < ncls; ++c) {
                seg_logits<S>(lb + (size_t)c * lp, tp, z);
#pragma unroll
                for (int a = 0; a < S; ++a)
#pragma unroll
                    for (int q = 0; q < S; ++q) m[a][q] = fmaxf(m[a][q], z[a][q]);
            }
            for (int c = 0; c < ncls; ++c) {
                seg_logits<S>(lb + (size_t)c * lp, tp, z);
#pragma unroll
                for (int a = 0; a < S; ++a)
#pragma unroll
                    for (int q = 0; q < S; ++q) {
                        const float d = z[a][q] - m[a][q];
                        s[a][q] += expf(d);
                        if (((tb[a] >> (8 * q)) & 255u) == (unsigned)c) zt[a][q] = d;
                    }
            }
            const int W = S * w, Y0 = S * bi + Blk<S>::OFF, X0 = S * bj + Blk<S>::OFF;
            float sum = 0.f;
#pragma unroll
            for (int a = 0; a < S; ++a)
#pragma unroll
                for (int q = 0; q < S; ++q)
                    if ((vmask >> (a * S + q)) & 1u) {
                        const bool counted = ((tb[a] >> (8 * q)) & 255u) < (unsigned)ncls;
                        const float l = logf(s[a][q]);
                        sum += counted ? l - zt[a][q] : 0.f;
                        ml[(size_t)b * P + (size_t)(Y0 + a) * W + (X0 + q)] = make_float2(m[a][q], counted ? l : INFINITY);
                    }
            acc = (double)sum;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if (lane == 0) red[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ONE workgroup: the partial sums in a fixed order, the scale (kept for the backward) and the loss
__global__ __launch_bounds__(256) void k_seg_finish(const double* __restrict__ partial, int n, int mode, const int* __restrict__ dense_pos,
                                                    float loss_weight, double pixels, float* __restrict__ scale_out,
                                                    float* __restrict__ loss) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double den = mode == VKN_SEG_LOSS_FOCAL ? (double)max(dense_pos[0], 1) : pixels;
        const float scale = (float)((double)loss_weight / den);
        scale_out[0] = scale;
        loss[0] = (float)(red[0] * ((double)loss_weight / den));
    }
}

// -------------------------------------------------------------------------------------------------------------------- backward
// grid (ceil(w / 63), ceil(h / (SEG_NW - 1)), B x nsplit): the classes of an image are shared by `nsplit` workgroups per tile.  The block's
// S x S element derivatives are folded onto its four taps with the separable adjoint; low-res pixel (i, j) collects tap (0, 0) of block
// (i, j), (0, 1) of (i, j - 1), (1, 0) of (i - 1, j) and (1, 1) of (i - 1, j - 1): columns through one wave shift, rows through one LDS
// value per thread and class (double-buffered: one barrier per class).  At the clamped borders both taps of a direction are the same
// pixel and are summed before the exchange.  The first wave / lane of a workgroup only feed their neighbours.
template <int S, int MODE>
__global__ __launch_bounds__(SEG_THREADS) void k_seg_bwd(const float* __restrict__ low, const unsigned char* __restrict__ tgt,
                                                         const float* __restrict__ gout, const float* __restrict__ scale, int ncls, int h,
                                                         int w, int nsplit, float alpha, float gamma, const float2* __restrict__ ml,
                                                         float* __restrict__ grad_low) {
    __shared__ float xch[2][SEG_NW][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.z / nsplit, part = blockIdx.z - b * nsplit;
    const int cpp = (ncls + nsplit - 1) / nsplit, c_lo = part * cpp, c_hi = min(ncls, c_lo + cpp);
    const int bi = (int)blockIdx.y * (SEG_NW - 1) - 1 + wv, bj = (int)blockIdx.x * 63 - 1 + lane;
    const bool own = bi <= h - 1 && bj <= w - 1 && wv >= 1 && lane >= 1;
    const size_t lp = (size_t)h * w, P = lp * S * S;
    const float* lb = low + (size_t)b * ncls * lp;
    float* gb = grad_low + (size_t)b * ncls * lp;
    const float coef = gout[0] * scale[0];
    unsigned tb[S];
    const unsigned vmask = seg_block<S>(tgt + (size_t)b * P, bi, bj, h, w, ncls, tb);
    const Taps tp = seg_taps(bi, bj, h, w);
    const bool g2 = gamma == 2.f;
    unsigned active = vmask;                        // CE: the pixels that count (inside the map, not ignored)
    float mx[S][S], ls[S][S];
    if (MODE == VKN_SEG_LOSS_CE) {
        const int W = S * w, Y0 = S * bi + Blk<S>::OFF, X0 = S * bj + Blk<S>::OFF;
#pragma unroll
        for (int a = 0; a < S; ++a)
#pragma unroll
            for (int q = 0; q < S; ++q) {
                mx[a][q] = 0.f;
                ls[a][q] = 0.f;
                if ((vmask >> (a * S + q)) & 1u) {
                    if (((tb[a] >> (8 * q)) & 255u) < (unsigned)ncls) {
                        const float2 v = ml[(size_t)b * P + (size_t)(Y0 + a) * W + (X0 + q)];
                        mx[a][q] = v.x;
                        ls[a][q] = v.y;
                    } else {
                        active &= ~(1u << (a * S + q));
                    }
                }
            }
    }
    const size_t oown = (size_t)max(bi, 0) * w + max(bj, 0);
    for (int c = c_lo; c < c_hi; ++c) {
        float z[S][S], g[S][S];
        seg_logits<S>(lb + (size_t)c * lp, tp, z);
#pragma unroll
        for (int a = 0; a < S; ++a)
#pragma unroll
            for (int q = 0; q < S; ++q) {
                const float t = ((tb[a] >> (8 * q)) & 255u) == (unsigned)c ? 1.f : 0.f;
                float v;
                if (MODE == VKN_SEG_LOSS_FOCAL) v = seg_focal_dz(z[a][q], t, alpha, gamma, g2);
                else v = expf((z[a][q] - mx[a][q]) - ls[a][q]) - t;
                g[a][q] = ((active >> (a * S + q)) & 1u) ? coef * v : 0.f;
            }
        // the adjoint onto the four taps: columns first, in a fixed order
        float t00 = 0.f, t01 = 0.f, t10 = 0.f, t11 = 0.f;
#pragma unroll
        for (int a = 0; a < S; ++a) {
            float r0 = 0.f, r1 = 0.f;
#pragma unroll
            for (int q = 0; q < S; ++q) {
                const float lx = Blk<S>::l(q);
                r0 += (1.f - lx) * g[a][q];
                r1 += lx * g[a][q];
            }
            const float ly = Blk<S>::l(a);
            t00 += (1.f - ly) * r0; t01 += (1.f - ly) * r1;
            t10 += ly * r0;         t11 += ly * r1;
        }
        if (bj < 0) { t01 += t00; t00 = 0.f; t11 += t10; t10 = 0.f; }               // column -1 is column 0
        else if (bj >= w - 1) { t00 += t01; t01 = 0.f; t10 += t11; t11 = 0.f; }     // column w is column w - 1
        float up = t00 + __shfl_up(t01, 1);       // row bi of column bj
        float dn = t10 + __shfl_up(t11, 1);       // row bi + 1 of column bj
        if (bi < 0) { dn += up; up = 0.f; }
        else if (bi >= h - 1) { up += dn; dn = 0.f; }
        xch[c & 1][wv][lane] = dn;
        __syncthreads();
        if (own) gb[(size_t)c * lp + oown] = up + xch[c & 1][wv - 1][lane];
    }
}

struct SegShape { int gx, gy, bx, by, nsplit; };

inline int seg_check_shape(int mode, int B, int ncls, int h, int w, int S) {
    if (mode != VKN_SEG_LOSS_FOCAL && mode != VKN_SEG_LOSS_CE) return VKN_E_SHAPE;
    if (!(S == 1 || S == 2 || S == 4) || ncls < 1 || ncls > VKN_SEG_MAX_CLASSES || B < 1 || B > VKN_SEG_MAX_IMAGES || h < 1 || w < 1)
        return VKN_E_SHAPE;
    if ((long long)ncls * h * w * 4 >= (1ll << 31)) return VKN_E_SHAPE;
    if (h > (SEG_NW - 1) * 65535) return VKN_E_SHAPE;     // grid.y of the backward
    return VKN_OK;
}

inline SegShape seg_shape(int ncls, int h, int w) {
    SegShape s;
    s.gx = (w + 1 + 63) / 64;
    s.gy = (h + 1 + SEG_NW - 1) / SEG_NW;
    s.bx = (w + 62) / 63;
    s.by = (h + SEG_NW - 2) / (SEG_NW - 1);
    s.nsplit = ncls >= 8 ? 4 : 1;
    return s;
}

template <int MODE>
void seg_launch_fwd(int S, dim3 grid, hipStream_t st, const float* low, const unsigned char* tgt, int ncls, int h, int w, float alpha,
                    float gamma, double* partial, float2* ml) {
    if (S == 4) hipLaunchKernelGGL((k_seg_fwd<4, MODE>), grid, dim3(SEG_THREADS), 0, st, low, tgt, ncls, h, w, alpha, gamma, partial, ml);
    else if (S == 2) hipLaunchKernelGGL((k_seg_fwd<2, MODE>), grid, dim3(SEG_THREADS), 0, st, low, tgt, ncls, h, w, alpha, gamma, partial, ml);
    else hipLaunchKernelGGL((k_seg_fwd<1, MODE>), grid, dim3(SEG_THREADS), 0, st, low, tgt, ncls, h, w, alpha, gamma, partial, ml);
}

template <int MODE>
void seg_launch_bwd(int S, dim3 grid, hipStream_t st, const float* low, const unsigned char* tgt, const float* gout, const float* scale,
                    int ncls, int h, int w, int nsplit, float alpha, float gamma, const float2* ml, float* grad_low) {
    if (S == 4) hipLaunchKernelGGL((k_seg_bwd<4, MODE>), grid, dim3(SEG_THREADS), 0, st, low, tgt, gout, scale, ncls, h, w, nsplit, alpha, gamma, ml, grad_low);
    else if (S == 2) hipLaunchKernelGGL((k_seg_bwd<2, MODE>), grid, dim3(SEG_THREADS), 0, st, low, tgt, gout, scale, ncls, h, w, nsplit, alpha, gamma, ml, grad_low);
    else hipLaunchKernelGGL((k_seg_bwd<1, MODE>), grid, dim3(SEG_THREADS), 0, st, low, tgt, gout, scale, ncls, h, w, nsplit, alpha, gamma, ml, grad_low);
}

}  // namespace

extern "C" {

size_t vkn_sizeof_seg_image(void) { return sizeof(VknSegImage); }

int vkn_seg_targets_u8(const VknSegImage* imgs, int B, int H, int W, int ncls, unsigned char* tgt, int* dense_pos, int* status,
                       void* stream) {
    if (!imgs || !tgt || !dense_pos || !status || B < 0) return VKN_E_ARG;
    if (B < 1 || B > VKN_SEG_MAX_IMAGES) return VKN_E_SHAPE;
    for (int b = 0; b < B; ++b) {
        const VknSegImage& im = imgs[b];
        if (im.G < 0 || im.n_sem < 0 || im.Np < 0) return VKN_E_ARG;
        if ((im.G > 0 && (!im.masks || !im.labels)) || (im.sem && im.n_sem > 0 && !im.sem_cls) || (im.Np > 0 && !im.gt_inds)) return VKN_E_ARG;
    }
    if (ncls < 1 || ncls > VKN_SEG_MAX_CLASSES || H < 1 || W < 1 || (long long)H * W >= (1ll << 31) || H > ST_ROWS * 65535) return VKN_E_SHAPE;
    for (int b = 0; b < B; ++b)
        if (imgs[b].G > VKN_SEG_MAX_ROWS || imgs[b].Np > VKN_SEG_MAX_ROWS || imgs[b].n_sem > VKN_SEG_MAX_ROWS) return VKN_E_SHAPE;
    if (!vkn_aligned(dense_pos, 4) || !vkn_aligned(status, 4)) return VKN_E_ALIGN;
    for (int b = 0; b < B; ++b)
        if (!vkn_aligned(imgs[b].masks, 4) || !vkn_aligned(imgs[b].sem, 4) || !vkn_aligned(imgs[b].labels, 8) ||
            !vkn_aligned(imgs[b].sem_cls, 8) || !vkn_aligned(imgs[b].gt_inds, 8))
            return VKN_E_ALIGN;
    if (!vkn_on_device(tgt) || !vkn_on_device(dense_pos) || !vkn_on_device(status)) return VKN_E_ARG;
    SegBatch batch = {};
    for (int b = 0; b < B; ++b) {
        const VknSegImage& im = imgs[b];
        if ((im.G > 0 && (!vkn_on_device(im.masks) || !vkn_on_device(im.labels))) ||
            (im.sem && im.n_sem > 0 && (!vkn_on_device(im.sem) || !vkn_on_device(im.sem_cls))) || (im.Np > 0 && !vkn_on_device(im.gt_inds)))
            return VKN_E_ARG;
        batch.img[b] = im;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(dense_pos, 0, sizeof(int), st) != hipSuccess) return VKN_E_LAUNCH;
    const dim3 grid((W + ST_COLS - 1) / ST_COLS, (H + ST_ROWS - 1) / ST_ROWS, B);
    hipLaunchKernelGGL(k_seg_targets, grid, dim3(256), 0, st, batch, H, W, ncls, tgt, dense_pos, status);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

size_t vkn_seg_loss_state_bytes(int mode, int B, int h, int w, int S) {
    if (seg_check_shape(mode, B, 1, h, w, S) != VKN_OK) return 0;
    const SegShape s = seg_shape(1, h, w);
    size_t bytes = SEG_HEADER + (((size_t)s.gx * s.gy * B * sizeof(double) + 15) & ~(size_t)15);
    if (mode == VKN_SEG_LOSS_CE) bytes += (size_t)B * h * w * S * S * sizeof(float2);
    return bytes;
}

int vkn_seg_loss_fwd_f32(const float* low, const unsigned char* tgt, const int* dense_pos, int mode, int B, int ncls, int h, int w, int S,
                         float alpha, float gamma, float loss_weight, float* loss, void* state, void* stream) {
    if (!low || !tgt || !loss || !state || (mode == VKN_SEG_LOSS_FOCAL && !dense_pos)) return VKN_E_ARG;
    const int rc = seg_check_shape(mode, B, ncls, h, w, S);
    if (rc != VKN_OK) return rc;
    if (!vkn_aligned(low, 4) || !vkn_aligned(loss, 4) || !vkn_aligned(dense_pos, 4) || !vkn_aligned(state, 16)) return VKN_E_ALIGN;
    if (!vkn_on_device(low) || !vkn_on_device(tgt) || !vkn_on_device(loss) || !vkn_on_device(state) ||
        (mode == VKN_SEG_LOSS_FOCAL && !vkn_on_device(dense_pos)))
        return VKN_E_ARG;
    const SegShape s = seg_shape(ncls, h, w);
    const int n = s.gx * s.gy * B;
    char* base = static_cast<char*>(state);
    double* partial = reinterpret_cast<double*>(base + SEG_HEADER);
    float2* ml = reinterpret_cast<float2*>(base + SEG_HEADER + (((size_t)n * sizeof(double) + 15) & ~(size_t)15));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(s.gx, s.gy, B);
    if (mode == VKN_SEG_LOSS_FOCAL) seg_launch_fwd<VKN_SEG_LOSS_FOCAL>(S, grid, st, low, tgt, ncls, h, w, alpha, gamma, partial, ml);
    else seg_launch_fwd<VKN_SEG_LOSS_CE>(S, grid, st, low, tgt, ncls, h, w, alpha, gamma, partial, ml);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_seg_finish, dim3(1), dim3(256), 0, st, partial, n, mode, dense_pos, loss_weight, (double)B * h * w * S * S,
                       reinterpret_cast<float*>(base), loss);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

int vkn_seg_loss_bwd_f32(const float* low, const unsigned char* tgt, const float* gout, int mode, int B, int ncls, int h, int w, int S,
                         float alpha, float gamma, const void* state, float* grad_low, void* stream) {
    if (!low || !tgt || !gout || !state || !grad_low) return VKN_E_ARG;
    const int rc = seg_check_shape(mode, B, ncls, h, w, S);
    if (rc != VKN_OK) return rc;
    if (!vkn_aligned(low, 4) || !vkn_aligned(gout, 4) || !vkn_aligned(grad_low, 4) || !vkn_aligned(state, 16)) return VKN_E_ALIGN;
    if (!vkn_on_device(low) || !vkn_on_device(tgt) || !vkn_on_device(gout) || !vkn_on_device(state) || !vkn_on_device(grad_low))
        return VKN_E_ARG;
    const SegShape s = seg_shape(ncls, h, w);
    const int n = s.gx * s.gy * B;
    const char* base = static_cast<const char*>(state);
    const float2* ml = reinterpret_cast<const float2*>(base + SEG_HEADER + (((size_t)n * sizeof(double) + 15) & ~(size_t)15));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(s.bx, s.by, B * s.nsplit);
    if (mode == VKN_SEG_LOSS_FOCAL)
        seg_launch_bwd<VKN_SEG_LOSS_FOCAL>(S, grid, st, low, tgt, gout, reinterpret_cast<const float*>(base), ncls, h, w, s.nsplit, alpha, gamma, ml, grad_low);
    else
        seg_launch_bwd<VKN_SEG_LOSS_CE>(S, grid, st, low, tgt, gout, reinterpret_cast<const float*>(base), ncls, h, w, s.nsplit, alpha, gamma, ml, grad_low);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

}  // extern "C"
