// vkn_fpn.hip — the localization FPN of the kernel-initialisation head ("RPN"): `SemanticFPNWrapper` with GroupNorm'ed 3x3 convs
// (knet/det/semantic_fpn_wrapper.py:73-176, forward :197-237) followed by the head's `loc_convs` / `seg_convs`
// (knet/det/kernel_head.py:150-159, 207-230), everything between the backbone's P2..P5 and `vkn_kernel_init_f32`.
//
// One engine, k_fpn_conv: an implicit GEMM out[co][px] = sum_{tap, ci} W[co][ci][tap] * in[ci][px + shift(tap)] on MFMA
// (v_mfma_f32_32x32x16_f16, the two-term f16 split of vkn_common.h: hi*hi + hi*lo + lo*hi, fp32 accumulation; 2^-22 relative where the
// low half is a normal f16, absolute 2^-24 for staged activations below 2^-3 and for weights below 2^-3 after the pre-scale: the
// resolution paragraph of include/vkn.h at the localization FPN).
//   * workgroup = 4 waves = 256 output channels x one 64-pixel run of an output row; wave w owns channels 64w .. 64w+63
//     (two 32-row MFMA blocks) x the 64 pixels (two 32-column blocks);
//   * B operand (activations): per 32-channel chunk the input patch under the run (3 rows x (63 s + 3) columns for a 3x3 conv of
//     stride s) is staged in LDS as f16 hi / lo planes [row][column][channel], TRANSFORMED ON LOAD: raw input (+ the positional
//     map), or a previous conv's raw output with its GroupNorm + ReLU applied from its statistics (normalisation in the consumer,
//     DESIGN §4), optionally bilinear x2 (align_corners=False) of those normalised taps, or the sum of up to four such sources
//     (the FPN's level sum).  No im2col: the nine taps are nine shifted reads of the same patch;
//   * A operand (weights): fragment images prepared once per weight update (k_fpn_wsplit), pre-scaled by a power of two per matrix
//     so that the lo terms of N(0, 0.01) weights stay normal f16; the epilogue multiplies by the inverse power (exact);
//   * epilogue: raw fp32 output + per (frame, channel, run) (mean, M2) partials; k_fpn_gn_finish merges them in a fixed order in
//     fp64 (Chan) into mean / rstd per (frame, group).  No float atomics: bitwise deterministic.
// Range: every staged activation must satisfy |v| < 65504 (the f16 split's envelope); a non-finite or larger value ORs
// VKN_STATUS_RANGE into the workspace status word (include/vkn.h).
#include "../../include/vkn.h"
#include "../../include/vkn_fpn_train.h"
#include "vkn_common.h"
#include "vkn_convtile.h"

#include <algorithm>

#define FPN_TRY(expr)             \
    do {                          \
        const int rc_ = (expr);   \
        if (rc_ != VKN_OK) return rc_; \
    } while (0)

#define FPN_MAX_SRC 4

enum { FPN_RAW = 0, FPN_NORM = 1, FPN_UP = 2 };

struct FpnSrc {
    const float* x;      // [B][..][Hs][Ws], frame stride bstride floats
    const float* st;     // (mean, rstd) per (frame, group): st[2 * (b * gstride + g) + {0, 1}]; NULL = raw
    const float* gamma;  // GroupNorm affine, per channel of this source
    const float* beta;
    long long bstride;
    int gstride, cpg;    // groups per frame in `st`, channels per group
};

struct FpnConvArgs {
    FpnSrc src[FPN_MAX_SRC];
    int nsrc, mode;
    const float* pos;            // [Cin][Hin][Win] added to a raw input (shared by the frames) or NULL
    const _Float16* wimg;        // prepared fragments (after the header)
    const float* wscale;         // {scale, 1 / scale}
    float* out;                  // [B][Cout][Ho][Wo] (frame stride out_bstride)
    long long out_bstride;
    float* part;                 // [B][Cout][T][2] (mean, M2) per 64-pixel run, T = Ho * ntx
    unsigned* status;
    int Cin, Cout, Hs, Ws, Hin, Win, Ho, Wo, ntx;
};

__device__ __forceinline__ float fpn_norm(const FpnSrc& s, int b, int c, float v) {
    const float* st = s.st + 2 * ((long long)b * s.gstride + c / s.cpg);
    return fmaxf(convtile::gn_preact(v, st[0], st[1], s.gamma[c], s.beta[c]), 0.f);
}

// value of input channel c at conv-input position (iy, ix), inside [0, Hin) x [0, Win)
__device__ __forceinline__ float fpn_load(const FpnConvArgs& a, int b, int c, int iy, int ix) {
    if (a.mode == FPN_UP) {  // at::upsample_bilinear2d, align_corners=False, scale 1/2 (aten/src/ATen/native/UpSample.h)
        const FpnSrc& s = a.src[0];
        const float hr = fmaxf(0.5f * (iy + 0.5f) - 0.5f, 0.f), wr = fmaxf(0.5f * (ix + 0.5f) - 0.5f, 0.f);
        const int h1 = (int)hr, w1 = (int)wr;
        const int hp = h1 < a.Hs - 1 ? a.Ws : 0, wp = w1 < a.Ws - 1 ? 1 : 0;
        const float l1h = hr - h1, l0h = 1.f - l1h, l1w = wr - w1, l0w = 1.f - l1w;
        const float* p = s.x + b * s.bstride + (long long)c * a.Hs * a.Ws + h1 * a.Ws + w1;
        const float v00 = fpn_norm(s, b, c, p[0]), v01 = fpn_norm(s, b, c, p[wp]);
        const float v10 = fpn_norm(s, b, c, p[hp]), v11 = fpn_norm(s, b, c, p[hp + wp]);
        return l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11);
    }
    const long long off = (long long)c * a.Hin * a.Win + iy * a.Win + ix;
    if (a.mode == FPN_RAW) return a.src[0].x[b * a.src[0].bstride + off] + (a.pos ? a.pos[off] : 0.f);
    float v = 0.f;  // FPN_NORM: the sum of nsrc normalised sources, in source order (Python's sum(), :216-219)
    for (int k = 0; k < a.nsrc; ++k) v += fpn_norm(a.src[k], b, c, a.src[k].x[b * a.src[k].bstride + off]);
    return v;
}

// sum over each 32-lane half: the result is in lane 31 (lanes 0-31) and lane 63 (lanes 32-63); fixed order
#define FPN_DPP_ADD(X, CTRL, ROWMASK) \
    X += __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(X), CTRL, ROWMASK, 0xF, false))
__device__ __forceinline__ float fpn_half_sum(float v) {
    FPN_DPP_ADD(v, 0x111, 0xF);  // row_shr:1
    FPN_DPP_ADD(v, 0x112, 0xF);  // row_shr:2
    FPN_DPP_ADD(v, 0x114, 0xF);  // row_shr:4
    FPN_DPP_ADD(v, 0x118, 0xF);  // row_shr:8
    FPN_DPP_ADD(v, 0x142, 0xA);  // row_bcast:15 into rows 1, 3
    return v;
}
#undef FPN_DPP_ADD

template <int KS, int S>
__global__ __launch_bounds__(convtile::THREADS) void k_fpn_conv(FpnConvArgs a) {
    using namespace convtile;
    constexpr int XW = (TILE - 1) * S + KS;  // patch columns
    constexpr int PL = KS * XW * PITCH;      // halfs per plane
    extern __shared__ _Float16 fpn_lds[];
    _Float16* lhi = fpn_lds;
    _Float16* llo = fpn_lds + PL;
    const int ncog = (a.Cout + 255) >> 8;
    const int tx = blockIdx.x, oy = blockIdx.y, b = blockIdx.z / ncog, cog = blockIdx.z % ncog;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ncb = a.Cout >> 5, nks = a.Cin >> 4;
    const WaveMap wm = wave_map(cog, wave, ncb);
    const int cb0 = wm.cb0;
    const int ox0 = tx * TILE, iy0 = oy * S - KS / 2, ix0 = ox0 * S - KS / 2;
    f32x16 acc[2][2] = {};
    unsigned bad = 0;
    const half8* wimg = reinterpret_cast<const half8*>(a.wimg);
    for (int c0 = 0; c0 < a.Cin; c0 += KC) {
        for (int e = threadIdx.x; e < KC * KS * XW; e += THREADS) {
            const int j = e % XW, r = (e / XW) % KS, ci = e / (XW * KS);
            const int iy = iy0 + r, ix = ix0 + j;
            float v = 0.f;  // zero padding of the conv input
            if (iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win) v = fpn_load(a, b, c0 + ci, iy, ix);
            stage(v, bad, lhi, llo, (r * XW + j) * PITCH + ci);
        }
        __syncthreads();
        if (wm.has0) {
#pragma unroll
            for (int tap = 0; tap < KS * KS; ++tap) {
                const int ky = tap / KS, kx = tap % KS;
                tap_product(acc, wimg, tap, nks, ncb, c0, cb0, wm.has1, lane, lhi, llo, (ky * XW + (lane & 31) * S + kx) * PITCH,
                            32 * S * PITCH);
            }
        }
        __syncthreads();
    }
    if (bad) atomicOr(a.status, (unsigned)VKN_STATUS_RANGE);
    const float isc = a.wscale[1];
    const int nvalid = min(TILE, a.Wo - ox0);
    const float inv_n = 1.f / (float)nvalid;
    const bool ok0 = (lane & 31) < nvalid, ok1 = 32 + (lane & 31) < nvalid;
    const long long P = (long long)a.Ho * a.Wo;
    const int T = a.Ho * a.ntx, t = oy * a.ntx + tx;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int cb = cb0 + q;
        if (cb >= ncb) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = cb * 32 + vkn_cd_row(r, lane);
            const float v0 = acc[q][0][r] * isc, v1 = acc[q][1][r] * isc;
            float* o = a.out + b * a.out_bstride + co * P + (long long)oy * a.Wo + ox0 + (lane & 31);
            if (ok0) o[0] = v0;
            if (ok1) o[32] = v1;
            // (mean, M2) of the row over the run's valid pixels: two passes over the registers
            const float sm = fpn_half_sum((ok0 ? v0 : 0.f) + (ok1 ? v1 : 0.f));
            const float mean = __shfl(sm, (lane & 32) + 31) * inv_n;
            const float d0 = ok0 ? v0 - mean : 0.f, d1 = ok1 ? v1 - mean : 0.f;
            const float m2 = fpn_half_sum(d0 * d0 + d1 * d1);
            if ((lane & 31) == 31) {
                float* p = a.part + 2 * (((long long)b * a.Cout + co) * T + t);
                p[0] = mean;
                p[1] = m2;
            }
        }
    }
}

// mean / rstd per (frame, group) from the run partials: fixed-order Chan merge in fp64 (256 contiguous segments, then a fixed tree)
__global__ __launch_bounds__(256) void k_fpn_gn_finish(const float* __restrict__ part, float* __restrict__ st, int Cout, int G,
                                                       int Ho, int Wo, int ntx, float eps) {
    __shared__ double sn[256], sm[256], sq[256];
    const int b = blockIdx.x / G, g = blockIdx.x % G, cpg = Cout / G, T = Ho * ntx;
    const long long items = (long long)cpg * T;
    const long long i0 = items * threadIdx.x / 256, i1 = items * (threadIdx.x + 1) / 256;
    double n = 0, m = 0, q = 0;
    for (long long i = i0; i < i1; ++i) {
        const int c = g * cpg + (int)(i / T), t = (int)(i % T);
        const float* p = part + 2 * (((long long)b * Cout + c) * T + t);
        const double nb = (double)min(convtile::TILE, Wo - (t % ntx) * convtile::TILE), mb = p[0], qb = p[1];
        const double nn = n + nb, d = mb - m;
        m += d * nb / nn;
        q += qb + d * d * n * nb / nn;
        n = nn;
    }
    sn[threadIdx.x] = n;
    sm[threadIdx.x] = m;
    sq[threadIdx.x] = q;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double na = sn[threadIdx.x], nb = sn[threadIdx.x + s];
            if (nb > 0) {
                const double nn = na + nb, d = sm[threadIdx.x + s] - sm[threadIdx.x];
                sm[threadIdx.x] += d * nb / nn;
                sq[threadIdx.x] += sq[threadIdx.x + s] + d * d * na * nb / nn;
                sn[threadIdx.x] = nn;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        st[2 * (b * G + g)] = (float)sm[0];
        st[2 * (b * G + g) + 1] = (float)(1.0 / sqrt(sq[0] / sn[0] + (double)eps));  // biased variance, as nn.GroupNorm
    }
}

// y = relu(GN(x)) for C channels of a raw output (frame stride in_bstride) -> dst [B][C][P]; may run in place
__global__ __launch_bounds__(256) void k_fpn_gn_apply(const float* x, long long in_bstride, const float* __restrict__ st,
                                                      int gstride, int cpg, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* dst, int C, long long P) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (long long)C * P; i += (long long)gridDim.x * 256) {
        const int b = blockIdx.y, c = (int)(i / P);
        const float* s = st + 2 * ((long long)b * gstride + c / cpg);
        const float v = x[b * in_bstride + i];
        dst[(long long)b * C * P + i] = fmaxf(convtile::gn_preact(v, s[0], s[1], gamma[c], beta[c]), 0.f);
    }
}

// weight preparation: the power-of-two scale of one matrix (max |w| * scale in [2^14, 2^15)) ...
__global__ __launch_bounds__(256) void k_fpn_wscale(const float* __restrict__ w, long long n, float* __restrict__ sc) {
    float m = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(w[i]));
    const float mx = convtile::block_absmax(m);
    if (threadIdx.x == 0) convtile::pow2_scale(mx, sc);
}

// ... and the fragment images (vkn_convtile.h: frag_index)
__global__ __launch_bounds__(256) void k_fpn_wsplit(const float* __restrict__ w, const float* __restrict__ sc, _Float16* __restrict__ img,
                                                    int Cout, int Cin, int taps) {
    const long long n = (long long)taps * Cin * Cout;  // one thread per (tap, ks, cb, lane, j)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
    long long rest = i >> 9;
    const int ncb = Cout >> 5, nks = Cin >> 4;
    const int cb = (int)(rest % ncb);
    rest /= ncb;
    const int ks = (int)(rest % nks), tap = (int)(rest / nks);
    const int co = cb * 32 + (lane & 31), ci = ks * 16 + (lane >> 5) * 8 + j;
    _Float16 h, l;
    vkn_split_f16(w[((long long)co * Cin + ci) * taps + tap] * sc[0], h, l);
    img[convtile::frag_index(tap, nks, ks, ncb, cb, 0, lane) * 8 + j] = h;
    img[convtile::frag_index(tap, nks, ks, ncb, cb, 1, lane) * 8 + j] = l;
}

// ------------------------------------------------------------------------------------------------------------------ host side
namespace {

using convtile::align256;
using convtile::conv_out;

inline size_t fpn_part_bytes(int B, int Cout, int Ho, int Wo) {
    return align256((size_t)B * Cout * Ho * convtile::runs(Wo) * 2 * sizeof(float));
}

struct FpnGn {  // a conv output's statistics for its consumers
    const float* st;
    const float* gamma;
    const float* beta;
    int gstride, cpg;
};

FpnSrc fpn_src(const float* x, long long bstride, const FpnGn* gn) {
    FpnSrc s{};
    s.x = x;
    s.bstride = bstride;
    if (gn) {
        s.st = gn->st;
        s.gamma = gn->gamma;
        s.beta = gn->beta;
        s.gstride = gn->gstride;
        s.cpg = gn->cpg;
    }
    return s;
}

// one conv (+ its GN statistics): a.src / nsrc / mode / pos / Cin / Hs / Ws / Hin / Win filled by the caller
int fpn_conv(FpnConvArgs a, int ks, int stride, const void* wimg, int Cout, int B, float* out, long long out_bstride, float* st,
             int G, float* part, unsigned* status, hipStream_t stream) {
    a.wscale = convtile::image_scale(wimg);
    a.wimg = convtile::image_frags(wimg);
    a.Cout = Cout;
    a.Ho = conv_out(a.Hin, stride);
    a.Wo = conv_out(a.Win, stride);
    a.ntx = convtile::runs(a.Wo);
    a.out = out;
    a.out_bstride = out_bstride;
    a.part = part;
    a.status = status;
    const dim3 grid(a.ntx, a.Ho, B * ((Cout + 255) / 256));
    const int xw = (convtile::TILE - 1) * stride + ks;
    const size_t lds = (size_t)2 * ks * xw * convtile::PITCH * sizeof(_Float16);
    if (ks == 3 && stride == 1) hipLaunchKernelGGL((k_fpn_conv<3, 1>), grid, dim3(convtile::THREADS), lds, stream, a);
    else if (ks == 3 && stride == 2) hipLaunchKernelGGL((k_fpn_conv<3, 2>), grid, dim3(convtile::THREADS), lds, stream, a);
    else if (ks == 1 && stride == 1) hipLaunchKernelGGL((k_fpn_conv<1, 1>), grid, dim3(convtile::THREADS), lds, stream, a);
    else return VKN_E_SHAPE;
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fpn_gn_finish, dim3(B * G), dim3(256), 0, stream, part, st, Cout, G, a.Ho, a.Wo, a.ntx, 1e-5f);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

int fpn_apply(const float* x, long long in_bstride, const FpnGn& gn, float* dst, int B, int C, long long P, hipStream_t stream) {
    const long long n = (long long)C * P;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_fpn_gn_apply, dim3(blocks, B), dim3(256), 0, stream, x, in_bstride, gn.st, gn.gstride, gn.cpg, gn.gamma,
                       gn.beta, dst, C, P);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

}  // namespace

extern "C" {

size_t vkn_conv_weight_bytes(int Cout, int Cin, int ksize) {
    if (!convtile::chan_chunks(Cout) || !convtile::chan_chunks(Cin) || !convtile::conv_ok(ksize, 1)) return 0;
    return convtile::image_bytes(Cout, Cin, ksize * ksize);
}

int vkn_conv_prepare_f32(const float* w, int Cout, int Cin, int ksize, void* image, size_t image_bytes, void* stream) {
    if (!w || !image) return VKN_E_ARG;
    const size_t need = vkn_conv_weight_bytes(Cout, Cin, ksize);
    if (!need) return VKN_E_SHAPE;
    if (image_bytes < need) return VKN_E_WORKSPACE;
    if (!vkn_aligned(image, 16)) return VKN_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int taps = ksize * ksize;
    float* sc = static_cast<float*>(image);
    hipLaunchKernelGGL(k_fpn_wscale, dim3(1), dim3(256), 0, st, w, (long long)Cout * Cin * taps, sc);
    VKN_CHECK_LAUNCH();
    const long long n = (long long)taps * Cin * Cout;
    hipLaunchKernelGGL(k_fpn_wsplit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, sc,
                       const_cast<_Float16*>(convtile::image_frags(image)), Cout, Cin, taps);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

size_t vkn_conv_gn_workspace_bytes(int B, int Cout, int H, int W, int stride, int upsample) {
    if (B <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (stride != 1 && stride != 2)) return 0;
    const int Hin = upsample ? 2 * H : H, Win = upsample ? 2 * W : W;
    return 256 + fpn_part_bytes(B, Cout, conv_out(Hin, stride), conv_out(Win, stride));
}

int vkn_conv_gn_f32(const float* x, const float* pos, const float* in_stats, const float* in_gamma, const float* in_beta, int in_groups,
                    int upsample, const void* wimg, int ksize, int stride, int groups, float* out, float* out_stats, int B, int Cin,
                    int H, int W, int Cout, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !wimg || !out || !out_stats) return VKN_E_ARG;
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return VKN_E_ARG;
    if (!convtile::chan_ok(Cin) || !convtile::chan_ok(Cout) || !convtile::conv_ok(ksize, stride) || groups <= 0 || Cout % groups ||
        (upsample && !in_stats) || (in_stats && pos) || (in_stats && (!in_gamma || !in_beta || in_groups <= 0 || Cin % in_groups)))
        return VKN_E_SHAPE;
    if (!ws) return VKN_E_WORKSPACE;   // (include/vkn.h: a workspace that is NULL is VKN_E_WORKSPACE, as one that is too small)
    if (!vkn_aligned(x, 16) || !vkn_aligned(out, 16) || !vkn_aligned(wimg, 16) || !vkn_aligned(ws, 16)) return VKN_E_ALIGN;
    const size_t need = vkn_conv_gn_workspace_bytes(B, Cout, H, W, stride, upsample);
    if (ws_bytes < need) return VKN_E_WORKSPACE;
    const FpnGn gn{in_stats, in_gamma, in_beta, in_groups, in_groups > 0 ? Cin / in_groups : 1};
    FpnConvArgs a{};
    a.src[0] = fpn_src(x, (long long)Cin * H * W, in_stats ? &gn : nullptr);
    a.nsrc = 1;
    a.mode = upsample ? FPN_UP : in_stats ? FPN_NORM : FPN_RAW;
    a.pos = pos;
    a.Cin = Cin;
    a.Hs = H;
    a.Ws = W;
    a.Hin = upsample ? 2 * H : H;
    a.Win = upsample ? 2 * W : W;
    const long long P = (long long)conv_out(a.Hin, stride) * conv_out(a.Win, stride);
    return fpn_conv(a, ksize, stride, wimg, Cout, B, out, (long long)Cout * P, out_stats, groups,
                    reinterpret_cast<float*>(static_cast<char*>(ws) + 256), static_cast<unsigned*>(ws), static_cast<hipStream_t>(stream));
}

// the block's output from its raw output (include/vkn_fpn_train.h): the kernel that ends vkn_localization_fpn_f32
int vkn_gn_relu_apply_f32(const float* r, const float* stats, const float* gamma, const float* beta, int groups, float* y, int B, int C,
                          int H, int W, void* stream) {
    if (!r || !stats || !gamma || !beta || !y) return VKN_E_ARG;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return VKN_E_ARG;
    if (!convtile::chan_ok(C) || groups <= 0 || C % groups || !convtile::fits_i32(B, C, H, W)) return VKN_E_SHAPE;
    for (const void* p : {(const void*)r, (const void*)stats, (const void*)gamma, (const void*)beta, (const void*)y})
        if (!vkn_aligned(p, 16)) return VKN_E_ALIGN;
    const long long P = (long long)H * W;
    return fpn_apply(r, C * P, FpnGn{stats, gamma, beta, groups, C / groups}, y, B, C, P, static_cast<hipStream_t>(stream));
}

// workspace carve of vkn_localization_fpn_f32: header | partials | stats[11] | raw maps
struct FpnWs {
    float *part, *st[11], *r0, *r1, *r2a, *r2, *r3a, *r3b, *r3, *tail;
};

static size_t fpn_carve(int B, int C, int h, int w, int H4, int W4, int H5, int W5, char* base, FpnWs* o) {
    size_t off = 256;
    auto take = [&](size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += align256(bytes);
        return reinterpret_cast<float*>(p);
    };
    size_t part = fpn_part_bytes(B, 2 * C, h, w);
    part = std::max(part, fpn_part_bytes(B, C, H4, W4));
    part = std::max(part, fpn_part_bytes(B, C, H5, W5));
    o->part = take(part);
    for (int i = 0; i < 11; ++i) o->st[i] = take((size_t)B * 2 * C * 2 * sizeof(float));  // up to 2C groups (the 512-row tail)
    const size_t full = (size_t)B * C * h * w * sizeof(float);
    o->r0 = take(full);
    o->r1 = take(full);
    o->r2a = take((size_t)B * C * H4 * W4 * sizeof(float));
    o->r2 = take(full);
    o->r3a = take((size_t)B * C * H5 * W5 * sizeof(float));
    o->r3b = take((size_t)B * C * H4 * W4 * sizeof(float));
    o->r3 = take(full);
    o->tail = take(2 * full);
    return off;
}

static bool fpn_shapes_ok(int H2, int W2, int H3, int W3, int H4, int W4, int H5, int W5) {
    if (H2 <= 0 || W2 <= 0 || H3 <= 0 || W3 <= 0 || H4 <= 0 || W4 <= 0 || H5 <= 0 || W5 <= 0) return false;
    // every level reaches the stride-8 grid of P3: P2 by a stride-2 conv, P4 by one x2, P5 by two (:216-219 adds them)
    return conv_out(H2, 2) == H3 && conv_out(W2, 2) == W3 && 2 * H4 == H3 && 2 * W4 == W3 && 4 * H5 == H3 && 4 * W5 == W3;
}

size_t vkn_localization_fpn_workspace_bytes(int B, int C, int H2, int W2, int H3, int W3, int H4, int W4, int H5, int W5) {
    if (B <= 0 || C <= 0 || !fpn_shapes_ok(H2, W2, H3, W3, H4, W4, H5, W5)) return 0;
    FpnWs o;
    return fpn_carve(B, C, H3, W3, H4, W4, H5, W5, nullptr, &o);
}

int vkn_localization_fpn_f32(const float* p2, const float* p3, const float* p4, const float* p5, const float* pos5,
                             const void* const* wimg, const float* const* gamma, const float* const* beta, int groups, float* loc,
                             float* sem, int B, int C, int H2, int W2, int H3, int W3, int H4, int W4, int H5, int W5, void* ws,
                             size_t ws_bytes, void* stream) {
    if (!p2 || !p3 || !p4 || !p5 || !wimg || !gamma || !beta || !loc || !sem) return VKN_E_ARG;
    if (B <= 0 || C <= 0) return VKN_E_ARG;
    if (!convtile::chan_chunks(C) || C > 256 || groups <= 0 || C % groups || !fpn_shapes_ok(H2, W2, H3, W3, H4, W4, H5, W5)) return VKN_E_SHAPE;
    const bool with_ls = wimg[8] != nullptr;
    for (int i = 0; i < (with_ls ? 10 : 8); ++i)
        if (!wimg[i] || !gamma[i] || !beta[i] || !vkn_aligned(wimg[i], 16)) return VKN_E_ARG;
    if (with_ls != (wimg[9] != nullptr)) return VKN_E_ARG;
    if (!ws) return VKN_E_WORKSPACE;
    for (const void* p : {(const void*)p2, (const void*)p3, (const void*)p4, (const void*)p5, (const void*)loc, (const void*)sem, (const void*)ws})
        if (!vkn_aligned(p, 16)) return VKN_E_ALIGN;
    FpnWs w;
    const size_t need = fpn_carve(B, C, H3, W3, H4, W4, H5, W5, static_cast<char*>(ws), &w);
    if (ws_bytes < need) return VKN_E_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned* status = static_cast<unsigned*>(ws);
    const int h = H3, wd = W3, cpg = C / groups;
    const long long P = (long long)h * wd, P4 = (long long)H4 * W4, P5 = (long long)H5 * W5;
    auto gn = [&](int i, int gstride = 0) { return FpnGn{w.st[i], gamma[i], beta[i], gstride ? gstride : groups, cpg}; };
    auto raw = [&](const float* x, long long bs, const float* pos, int H, int W) {
        FpnConvArgs a{};
        a.src[0] = fpn_src(x, bs, nullptr);
        a.nsrc = 1;
        a.mode = FPN_RAW;
        a.pos = pos;
        a.Cin = C;
        a.Hs = a.Hin = H;
        a.Ws = a.Win = W;
        return a;
    };
    auto normed = [&](const float* x, long long bs, const FpnGn& g, int H, int W, bool up) {
        FpnConvArgs a{};
        a.src[0] = fpn_src(x, bs, &g);
        a.nsrc = 1;
        a.mode = up ? FPN_UP : FPN_NORM;
        a.Cin = C;
        a.Hs = H;
        a.Ws = W;
        a.Hin = up ? 2 * H : H;
        a.Win = up ? 2 * W : W;
        return a;
    };
    const long long fC = (long long)C * P;
    // level 0: conv0 (stride 2) on P2; level 1: conv0 on P3 (:77-106, :108-123)
    FPN_TRY(fpn_conv(raw(p2, (long long)C * H2 * W2, nullptr, H2, W2), 3, 2, wimg[0], C, B, w.r0, fC, w.st[0], groups, w.part, status, st));
    FPN_TRY(fpn_conv(raw(p3, fC, nullptr, h, wd), 3, 1, wimg[1], C, B, w.r1, fC, w.st[1], groups, w.part, status, st));
    // level 2: conv0 on P4, upsample0, conv1
    FPN_TRY(fpn_conv(raw(p4, (long long)C * P4, nullptr, H4, W4), 3, 1, wimg[2], C, B, w.r2a, (long long)C * P4, w.st[2], groups, w.part, status, st));
    FPN_TRY(fpn_conv(normed(w.r2a, (long long)C * P4, gn(2), H4, W4, true), 3, 1, wimg[3], C, B, w.r2, fC, w.st[3], groups, w.part, status, st));
    // level 3 (cat_coors_level): P5 + positional encoding, conv0, upsample0, conv1, upsample1, conv2 (:203-212)
    FPN_TRY(fpn_conv(raw(p5, (long long)C * P5, pos5, H5, W5), 3, 1, wimg[4], C, B, w.r3a, (long long)C * P5, w.st[4], groups, w.part, status, st));
    FPN_TRY(fpn_conv(normed(w.r3a, (long long)C * P5, gn(4), H5, W5, true), 3, 1, wimg[5], C, B, w.r3b, (long long)C * P4, w.st[5], groups, w.part, status, st));
    FPN_TRY(fpn_conv(normed(w.r3b, (long long)C * P4, gn(5), H4, W4, true), 3, 1, wimg[6], C, B, w.r3, fC, w.st[6], groups, w.part, status, st));
    // conv_pred ‖ aux_convs.0 on sum(levels): one 2C-row 1x1 GEMM reading the normalised sum once (:216-233)
    const FpnGn g0 = gn(0), g1 = gn(1), g3 = gn(3), g6 = gn(6);
    FpnConvArgs t{};
    t.src[0] = fpn_src(w.r0, fC, &g0);
    t.src[1] = fpn_src(w.r1, fC, &g1);
    t.src[2] = fpn_src(w.r2, fC, &g3);
    t.src[3] = fpn_src(w.r3, fC, &g6);
    t.nsrc = 4;
    t.mode = FPN_NORM;
    t.Cin = C;
    t.Hs = t.Hin = h;
    t.Ws = t.Win = wd;
    FPN_TRY(fpn_conv(t, 1, 1, wimg[7], 2 * C, B, w.tail, 2 * fC, w.st[7], 2 * groups, w.part, status, st));
    const FpnGn gout{w.st[7], gamma[7], beta[7], 2 * groups, cpg};
    const FpnGn gaux{w.st[7] + 2 * groups, gamma[7] + C, beta[7] + C, 2 * groups, cpg};
    if (!with_ls) {  // the module's own outputs [out, aux]
        FPN_TRY(fpn_apply(w.tail, 2 * fC, gout, loc, B, C, P, st));
        FPN_TRY(fpn_apply(w.tail + fC, 2 * fC, gaux, sem, B, C, P, st));
        return VKN_OK;
    }
    // loc_convs.0 on out, seg_convs.0 on aux (knet/det/kernel_head.py:207-230): raw into loc / sem, then GN + ReLU in place
    FpnConvArgs l = normed(w.tail, 2 * fC, gout, h, wd, false), s = normed(w.tail + fC, 2 * fC, gaux, h, wd, false);
    FPN_TRY(fpn_conv(l, 1, 1, wimg[8], C, B, loc, fC, w.st[8], groups, w.part, status, st));
    FPN_TRY(fpn_conv(s, 1, 1, wimg[9], C, B, sem, fC, w.st[9], groups, w.part, status, st));
    FPN_TRY(fpn_apply(loc, fC, gn(8), loc, B, C, P, st));
    FPN_TRY(fpn_apply(sem, fC, gn(9), sem, B, C, P, st));
    return VKN_OK;
}

}  // extern "C"
