// vkn_fpn_bwd.hip — backward of one localization-FPN block y = ReLU(GN(conv(x))) (include/vkn_fpn_train.h), the forward being
// vkn_conv_gn_f32 of vkn_fpn.hip (where vkn_gn_relu_apply_f32, the block's output from its raw output, lives too).  Three entry points:
//   * vkn_gn_relu_bwd_f32: GroupNorm + ReLU backward.  Sums per (frame, channel, 2048-pixel run) in fp32 per thread, fp64 per
//     workgroup; one workgroup per group merges them in a fixed order in fp64; then the elementwise pass;
//   * vkn_conv_wgrad_f32: dW = dr x^T over B Ho Wo, on v_mfma_f32_32x32x16_f16 with the two-term f16 split of vkn_common.h.  k (the
//     reduction) runs over the 64 pixels of an output-row run, so BOTH operands need 8 consecutive pixels per lane: dr straight
//     from memory, the input patch through LDS as one shifted copy per kx ([kx][ci][pixel], aligned 16-byte reads at any stride);
//   * vkn_conv_dgrad_f32: dx in gather form on the forward's tile (vkn_convtile.h: 256 output rows x 64 pixels per workgroup, 32-channel
//     chunks in LDS as [row][column][channel]); the A operand is the forward's prepared image of the flipped, transposed weight.
// Operand range: both MFMA kernels stage v * 2^e, 2^e per tensor from its max |v| (k_bwd_absmax_*), and undo it in the epilogue.
#include "../../include/vkn_fpn_train.h"
#include "vkn_common.h"
#include "vkn_convtile.h"

#include <algorithm>

#define BWD_XP 72        // wgrad: halfs per (kx, channel) row, 64 pixels + 8 pad (144-byte stride: 16 lanes cover the 64 banks once)
#define BWD_XW 66        // dgrad: patch columns, 64 + one on either side
#define BWD_MAX_PART 256 // workgroups of the max |v| pass

// ------------------------------------------------------------------------------------------------ power of two of one tensor
__global__ __launch_bounds__(256) void k_bwd_absmax_part(const float* __restrict__ x, long long n, float* __restrict__ part) {
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
    const float mx = convtile::block_absmax(m);
    if (threadIdx.x == 0) part[blockIdx.x] = mx;
}

__global__ __launch_bounds__(256) void k_bwd_absmax_fin(const float* __restrict__ part, int nblk, float* __restrict__ sc) {
    const float mx = convtile::block_absmax((int)threadIdx.x < nblk ? part[threadIdx.x] : 0.f);
    if (threadIdx.x == 0) convtile::pow2_scale(mx, sc);
}

// ------------------------------------------------------------------------------------------------ GroupNorm + ReLU
using convtile::gn_preact;  // the ReLU mask is the sign of the forward's own pre-activation

// part[b][c][run] = (sum dz, sum dz xhat) over the run's pixels
__global__ __launch_bounds__(256) void k_gnb_partial(const float* __restrict__ dy, const float* __restrict__ r,
                                                     const float* __restrict__ st, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, int G, int C, long long P, int nrun,
                                                     double* __restrict__ part, unsigned* status) {
    __shared__ double s1[256], s2[256];
    const int run = blockIdx.x, c = blockIdx.y, b = blockIdx.z, cpg = C / G;
    const float* s = st + 2 * ((long long)b * G + c / cpg);
    const float mean = s[0], rstd = s[1], ga = gamma[c], be = beta[c];
    const long long base = ((long long)b * C + c) * P;
    const long long p0 = (long long)run * VKN_FPN_BWD_RUN_PX, p1 = min(P, p0 + VKN_FPN_BWD_RUN_PX);
    float a1 = 0.f, a2 = 0.f;
    unsigned bad = 0;
    for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
        const float d = dy[base + p], v = r[base + p];
        bad |= !(fabsf(d) < INFINITY);
        const float xh = (v - mean) * rstd;
        const float dz = gn_preact(v, mean, rstd, ga, be) > 0.f ? d : 0.f;
        a1 += dz;
        a2 += dz * xh;
    }
    if (bad) atomicOr(status, (unsigned)VKN_STATUS_RANGE);
    s1[threadIdx.x] = a1;
    s2[threadIdx.x] = a2;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            s1[threadIdx.x] += s1[threadIdx.x + k];
            s2[threadIdx.x] += s2[threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* o = part + 2 * ((base / P) * nrun + run);
        o[0] = s1[0];
        o[1] = s2[0];
    }
}

// one workgroup per group: S[b][c] = the runs in order; gm[b][g] = (mean_grp(g), mean_grp(g xhat)) over the group's channels in
// order; dgamma / dbeta[c] over the frames in order.  All in fp64.
__global__ __launch_bounds__(256) void k_gnb_finish(const double* __restrict__ part, const float* __restrict__ gamma, int B, int C, int G,
                                                    long long P, int nrun, double* S, float* __restrict__ gm, float* __restrict__ dgamma,
                                                    float* __restrict__ dbeta) {
    const int g = blockIdx.x, cpg = C / G;
    for (int i = threadIdx.x; i < B * cpg; i += 256) {
        const long long bc = (long long)(i / cpg) * C + g * cpg + i % cpg;
        double a1 = 0, a2 = 0;
        for (int k = 0; k < nrun; ++k) {
            a1 += part[2 * (bc * nrun + k)];
            a2 += part[2 * (bc * nrun + k) + 1];
        }
        S[2 * bc] = a1;
        S[2 * bc + 1] = a2;
    }
    __syncthreads();
    const double inv_n = 1.0 / ((double)cpg * (double)P);
    for (int b = threadIdx.x; b < B; b += 256) {
        double m1 = 0, m2 = 0;
        for (int k = 0; k < cpg; ++k) {
            const int c = g * cpg + k;
            m1 += (double)gamma[c] * S[2 * ((long long)b * C + c)];
            m2 += (double)gamma[c] * S[2 * ((long long)b * C + c) + 1];
        }
        gm[2 * ((long long)b * G + g)] = (float)(m1 * inv_n);
        gm[2 * ((long long)b * G + g) + 1] = (float)(m2 * inv_n);
    }
    for (int k = threadIdx.x; k < cpg; k += 256) {
        const int c = g * cpg + k;
        double dg = 0, db = 0;
        for (int b = 0; b < B; ++b) {
            db += S[2 * ((long long)b * C + c)];
            dg += S[2 * ((long long)b * C + c) + 1];
        }
        dgamma[c] = (float)dg;
        dbeta[c] = (float)db;
    }
}

__global__ __launch_bounds__(256) void k_gnb_apply(const float* dy, const float* __restrict__ r, const float* __restrict__ st,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   const float* __restrict__ gm, int G, int cpg, int C, long long P, float* dr) {
    const int b = blockIdx.y;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (long long)C * P; i += (long long)gridDim.x * 256) {
        const int c = (int)(i / P);
        const long long sg = 2 * ((long long)b * G + c / cpg), o = (long long)b * C * P + i;
        const float mean = st[sg], rstd = st[sg + 1], ga = gamma[c], v = r[o];
        const float xh = (v - mean) * rstd;
        // the product rounded on its own (no contraction into g - mean_grp(g)): a group of ONE element has mean_grp(g) == g, dr == 0
        float g = (gn_preact(v, mean, rstd, ga, beta[c]) > 0.f ? dy[o] : 0.f) * ga;
        asm volatile("" : "+v"(g));
        dr[o] = rstd * ((g - gm[sg]) - xh * gm[sg + 1]);
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct WgArgs {
    const float* dr;    // [B][Cout][Ho][Wo]
    const float* x;     // [B][Cin][H][W]
    const float* sc;    // {2^e_dr, 2^-e_dr, 2^e_x, 2^-e_x}
    float* part;        // [nsplit][Cout][Cin][taps]
    unsigned* status;
    int Cin, Cout, H, W, Ho, Wo, ntx, nsplit;
    long long nruns;    // B * Ho * ntx
};

// workgroup = (32 input channels, 128 output channels, one split of the runs); wave w owns output channels 32 w .. 32 w + 31 of
// the 128 and all k^2 taps: k^2 accumulator tiles [32 co][32 ci].  Per run and ky the patch row is staged once per kx.
template <int KS, int S>
__global__ __launch_bounds__(convtile::THREADS) void k_conv_wgrad(WgArgs a) {
    using namespace convtile;
    constexpr int PAD = KS / 2;
    constexpr int PL = KS * KC * BWD_XP;  // halfs per plane
    __shared__ __attribute__((aligned(16))) _Float16 wg_lds[2 * PL];
    _Float16* lhi = wg_lds;
    _Float16* llo = wg_lds + PL;
    const int ci0 = blockIdx.x * KC, sp = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int co0 = blockIdx.y * 128 + wave * 32;
    const bool has = co0 < a.Cout;
    f32x16 acc[KS * KS];
#pragma unroll
    for (int t = 0; t < KS * KS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const float sdr = a.sc[0], sx = a.sc[2];
    unsigned bad = 0;
    const long long run0 = a.nruns * sp / a.nsplit, run1 = a.nruns * (sp + 1) / a.nsplit;
    for (long long run = run0; run < run1; ++run) {
        const int tx = (int)(run % a.ntx), oy = (int)((run / a.ntx) % a.Ho), b = (int)(run / ((long long)a.ntx * a.Ho));
        const int ox0 = tx * TILE;
        // A operand: lane l holds dr[co0 + (l & 31)][oy][ox0 + 16 ks + 8 (l >> 5) + j], j = 0..7, of k-step ks
        half8 ah[4], al[4];
        if (has) {
            const float* p = a.dr + (((long long)b * a.Cout + co0 + (lane & 31)) * a.Ho + oy) * a.Wo;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int ox = ox0 + ks * 16 + (lane >> 5) * 8 + j;
                    _Float16 h, l;
                    range_split(ox < a.Wo ? p[ox] * sdr : 0.f, bad, h, l);
                    ah[ks][j] = h;
                    al[ks][j] = l;
                }
        }
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
            const int iy = oy * S + ky - PAD;
            __syncthreads();  // the previous row's fragment reads are done
            for (int e = threadIdx.x; e < KS * KC * TILE; e += THREADS) {
                const int j = e % TILE, ci = (e / TILE) % KC, kx = e / (TILE * KC);
                const int ox = ox0 + j, ix = ox * S + kx - PAD;
                float v = 0.f;  // zero padding of the conv input, and the columns past the run's end
                if (ox < a.Wo && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                    v = a.x[(((long long)b * a.Cin + ci0 + ci) * a.H + iy) * a.W + ix] * sx;
                stage(v, bad, lhi, llo, (kx * KC + ci) * BWD_XP + j);
            }
            __syncthreads();
            if (has) {
#pragma unroll
                for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        // B operand: lane l holds x[ci0 + (l & 31)][iy][(ox0 + 16 ks + 8 (l >> 5) + j) S + kx - PAD]
                        const int o = (kx * KC + (lane & 31)) * BWD_XP + ks * 16 + (lane >> 5) * 8;
                        const half8 bh = *reinterpret_cast<const half8*>(lhi + o);
                        const half8 bl = *reinterpret_cast<const half8*>(llo + o);
                        f32x16 c = acc[ky * KS + kx];
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ks], bh, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[ks], bl, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[ks], bh, c, 0, 0, 0);
                        acc[ky * KS + kx] = c;
                    }
            }
        }
    }
    if (bad) atomicOr(a.status, (unsigned)VKN_STATUS_RANGE);
    if (!has) return;
    const float isd = a.sc[1], isx = a.sc[3];
    float* out = a.part + (long long)sp * a.Cout * a.Cin * (KS * KS);
#pragma unroll
    for (int t = 0; t < KS * KS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + vkn_cd_row(r, lane), ci = ci0 + (lane & 31);
            out[((long long)co * a.Cin + ci) * (KS * KS) + t] = acc[t][r] * isx * isd;
        }
}

__global__ __launch_bounds__(256) void k_wgrad_sum(const float* __restrict__ part, int nsplit, long long n, float* __restrict__ dw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0;
    for (int k = 0; k < nsplit; ++k) s += part[k * n + i];
    dw[i] = (float)s;
}

// ------------------------------------------------------------------------------------------------ input gradient
struct DgArgs {
    const float* dr;       // [B][Cout][Ho][Wo]
    const _Float16* wimg;  // fragments of wt[ci][co][k - 1 - ky][k - 1 - kx] (after the header)
    const float* wscale;   // the image's {scale, 1 / scale}
    const float* sc;       // {2^e_dr, 2^-e_dr}
    float* dx;             // [B][Cin][H][W]
    unsigned* status;
    int Cin, Cout, H, W, Ho, Wo;
};

// workgroup = 4 waves = 256 input channels x 64 input pixels ix = (x0 + j) S + par of row iy (par: the column parity class,
// always 0 at stride 1); wave w owns channels 64 w .. 64 w + 63.  Tap (ky, kx) reaches the run iff (iy + PAD - ky) and
// (par + PAD - kx) are multiples of S: then pixel j reads dr row (iy + PAD - ky) / S, column x0 + j + (par + PAD - kx) / S.
template <int KS, int S>
__global__ __launch_bounds__(convtile::THREADS) void k_conv_dgrad(DgArgs a) {
    using namespace convtile;
    constexpr int PAD = KS / 2;
    constexpr int PL = KS * BWD_XW * PITCH;  // halfs per plane
    __shared__ __attribute__((aligned(16))) _Float16 dg_lds[2 * PL];
    _Float16* lhi = dg_lds;
    _Float16* llo = dg_lds + PL;
    const int ncig = (a.Cin + 255) >> 8;
    const int par = blockIdx.x % S, tx = blockIdx.x / S, iy = blockIdx.y, b = blockIdx.z / ncig, cig = blockIdx.z % ncig;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ncb = a.Cin >> 5, nks = a.Cout >> 4;
    const WaveMap wm = wave_map(cig, wave, ncb);
    const int cb0 = wm.cb0;
    const int x0 = tx * TILE;
    f32x16 acc[2][2] = {};
    const float sdr = a.sc[0];
    unsigned bad = 0;
    const half8* wimg = reinterpret_cast<const half8*>(a.wimg);
    for (int c0 = 0; c0 < a.Cout; c0 += KC) {
        for (int e = threadIdx.x; e < KC * KS * BWD_XW; e += THREADS) {
            const int j = e % BWD_XW, ky = (e / BWD_XW) % KS, co = e / (BWD_XW * KS);
            const int t = iy + PAD - ky, ox = x0 - 1 + j;
            float v = 0.f;
            if (t >= 0 && t % S == 0 && t / S < a.Ho && ox >= 0 && ox < a.Wo)
                v = a.dr[(((long long)b * a.Cout + c0 + co) * a.Ho + t / S) * a.Wo + ox] * sdr;
            stage(v, bad, lhi, llo, (ky * BWD_XW + j) * PITCH + co);
        }
        __syncthreads();
        if (wm.has0) {
#pragma unroll
            for (int ky = 0; ky < KS; ++ky) {
                const int t = iy + PAD - ky;
                if (t < 0 || t % S != 0 || t / S >= a.Ho) continue;  // uniform: the run is one row
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) {
                    const int u = par + PAD - kx;  // -1 .. 2
                    if (u % S != 0) continue;      // uniform: the run is one parity class
                    const int dxo = u / S;         // -1 .. 1
                    const int tap = (KS - 1 - ky) * KS + (KS - 1 - kx);
                    tap_product(acc, wimg, tap, nks, ncb, c0, cb0, wm.has1, lane, lhi, llo, (ky * BWD_XW + (lane & 31) + dxo + 1) * PITCH,
                                32 * PITCH);
                }
            }
        }
        __syncthreads();
    }
    if (bad) atomicOr(a.status, (unsigned)VKN_STATUS_RANGE);
    const float isc = a.wscale[1], isd = a.sc[1];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int cb = cb0 + q;
        if (cb >= ncb) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = cb * 32 + vkn_cd_row(r, lane);
            float* o = a.dx + (((long long)b * a.Cin + ci) * a.H + iy) * a.W;
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                const int ix = (x0 + pb * 32 + (lane & 31)) * S + par;
                if (ix < a.W) o[ix] = acc[q][pb][r] * isc * isd;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
namespace {

int bwd_pow2(const float* x, long long n, float* partials, float* sc, hipStream_t st) {
    const int nblk = (int)std::min<long long>((n + 1023) / 1024, BWD_MAX_PART);
    hipLaunchKernelGGL(k_bwd_absmax_part, dim3(nblk), dim3(256), 0, st, x, n, partials);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bwd_absmax_fin, dim3(1), dim3(256), 0, st, partials, nblk, sc);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

struct GnbWs {
    size_t part, S, gm, total;
    int nrun;
};
GnbWs gnb_carve(int B, int C, int H, int W, int G) {
    GnbWs w;
    const long long P = (long long)H * W;
    w.nrun = (int)((P + VKN_FPN_BWD_RUN_PX - 1) / VKN_FPN_BWD_RUN_PX);
    size_t off = 256;
    w.part = off;
    off += convtile::align256((size_t)B * C * w.nrun * 2 * sizeof(double));
    w.S = off;
    off += convtile::align256((size_t)B * C * 2 * sizeof(double));
    w.gm = off;
    off += convtile::align256((size_t)B * G * 2 * sizeof(float));
    w.total = off;
    return w;
}

struct WgWs {
    size_t sc, amax, part, total;
    int nsplit, ntx;
    long long nruns;
};
WgWs wg_carve(int B, int Cin, int H, int W, int Cout, int ksize, int stride) {
    WgWs w;
    const int Ho = convtile::conv_out(H, stride), Wo = convtile::conv_out(W, stride);
    w.ntx = convtile::runs(Wo);
    w.nruns = (long long)B * Ho * w.ntx;
    const int tiles = (Cin / convtile::KC) * ((Cout + 127) / 128);
    long long ns = std::max(1, VKN_FPN_WGRAD_TARGET_WGS / tiles);
    ns = std::min<long long>(ns, std::min<long long>(VKN_FPN_WGRAD_MAX_SPLITS, w.nruns));
    w.nsplit = (int)ns;
    size_t off = 256;
    w.sc = off;
    off += 256;
    w.amax = off;
    off += convtile::align256(BWD_MAX_PART * sizeof(float));
    w.part = off;
    off += convtile::align256((size_t)w.nsplit * Cout * Cin * ksize * ksize * sizeof(float));
    w.total = off;
    return w;
}

}  // namespace

extern "C" {

size_t vkn_gn_relu_bwd_workspace_bytes(int B, int C, int H, int W, int groups) {
    if (B <= 0 || H <= 0 || W <= 0 || !convtile::chan_ok(C) || groups <= 0 || C % groups || !convtile::fits_i32(B, C, H, W)) return 0;
    return gnb_carve(B, C, H, W, groups).total;
}

int vkn_gn_relu_bwd_f32(const float* dy, const float* r, const float* stats, const float* gamma, const float* beta, int groups, float* dr,
                        float* dgamma, float* dbeta, int B, int C, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !r || !stats || !gamma || !beta || !dr || !dgamma || !dbeta) return VKN_E_ARG;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return VKN_E_ARG;
    if (!convtile::chan_ok(C) || groups <= 0 || C % groups || !convtile::fits_i32(B, C, H, W) || B > 65535) return VKN_E_SHAPE;
    const GnbWs w = gnb_carve(B, C, H, W, groups);
    if (!ws || ws_bytes < w.total) return VKN_E_WORKSPACE;
    for (const void* p : {(const void*)dy, (const void*)r, (const void*)stats, (const void*)gamma, (const void*)beta, (const void*)dr,
                          (const void*)dgamma, (const void*)dbeta, (const void*)ws})
        if (!vkn_aligned(p, 16)) return VKN_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    double* part = reinterpret_cast<double*>(base + w.part);
    double* S = reinterpret_cast<double*>(base + w.S);
    float* gm = reinterpret_cast<float*>(base + w.gm);
    const long long P = (long long)H * W, n = (long long)C * P;
    hipLaunchKernelGGL(k_gnb_partial, dim3(w.nrun, C, B), dim3(256), 0, st, dy, r, stats, gamma, beta, groups, C, P, w.nrun, part,
                       reinterpret_cast<unsigned*>(base));
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gnb_finish, dim3(groups), dim3(256), 0, st, part, gamma, B, C, groups, P, w.nrun, S, gm, dgamma, dbeta);
    VKN_CHECK_LAUNCH();
    const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_gnb_apply, dim3(blocks, B), dim3(256), 0, st, dy, r, stats, gamma, beta, gm, groups, C / groups, C, P, dr);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

size_t vkn_conv_wgrad_workspace_bytes(int B, int Cin, int H, int W, int Cout, int ksize, int stride) {
    if (B <= 0 || H <= 0 || W <= 0 || !convtile::chan_ok(Cin) || !convtile::chan_ok(Cout) || !convtile::conv_ok(ksize, stride)) return 0;
    if (!convtile::fits_i32(B, Cin, H, W) || !convtile::fits_i32(B, Cout, convtile::conv_out(H, stride), convtile::conv_out(W, stride))) return 0;
    return wg_carve(B, Cin, H, W, Cout, ksize, stride).total;
}

int vkn_conv_wgrad_f32(const float* dr, const float* x, float* dw, int B, int Cin, int H, int W, int Cout, int ksize, int stride, void* ws,
                       size_t ws_bytes, void* stream) {
    if (!dr || !x || !dw) return VKN_E_ARG;
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return VKN_E_ARG;
    if (!vkn_conv_wgrad_workspace_bytes(B, Cin, H, W, Cout, ksize, stride)) return VKN_E_SHAPE;
    const WgWs w = wg_carve(B, Cin, H, W, Cout, ksize, stride);
    if (!ws || ws_bytes < w.total) return VKN_E_WORKSPACE;
    if (!vkn_aligned(dr, 16) || !vkn_aligned(x, 16) || !vkn_aligned(dw, 16) || !vkn_aligned(ws, 16)) return VKN_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    float* sc = reinterpret_cast<float*>(base + w.sc);
    float* amax = reinterpret_cast<float*>(base + w.amax);
    const int Ho = convtile::conv_out(H, stride), Wo = convtile::conv_out(W, stride);
    int rc = bwd_pow2(dr, (long long)B * Cout * Ho * Wo, amax, sc, st);
    if (rc != VKN_OK) return rc;
    rc = bwd_pow2(x, (long long)B * Cin * H * W, amax, sc + 2, st);
    if (rc != VKN_OK) return rc;
    WgArgs a{};
    a.dr = dr;
    a.x = x;
    a.sc = sc;
    a.part = reinterpret_cast<float*>(base + w.part);
    a.status = reinterpret_cast<unsigned*>(base);
    a.Cin = Cin;
    a.Cout = Cout;
    a.H = H;
    a.W = W;
    a.Ho = Ho;
    a.Wo = Wo;
    a.ntx = w.ntx;
    a.nsplit = w.nsplit;
    a.nruns = w.nruns;
    const dim3 grid(Cin / convtile::KC, (Cout + 127) / 128, w.nsplit);
    if (ksize == 3 && stride == 1) hipLaunchKernelGGL((k_conv_wgrad<3, 1>), grid, dim3(convtile::THREADS), 0, st, a);
    else if (ksize == 3) hipLaunchKernelGGL((k_conv_wgrad<3, 2>), grid, dim3(convtile::THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_conv_wgrad<1, 1>), grid, dim3(convtile::THREADS), 0, st, a);
    VKN_CHECK_LAUNCH();
    const long long n = (long long)Cout * Cin * ksize * ksize;
    hipLaunchKernelGGL(k_wgrad_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.part, w.nsplit, n, dw);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

size_t vkn_conv_dgrad_workspace_bytes(int B, int Cout, int H, int W, int stride) {
    if (B <= 0 || H <= 0 || W <= 0 || !convtile::chan_ok(Cout) || (stride != 1 && stride != 2)) return 0;
    if (!convtile::fits_i32(B, Cout, convtile::conv_out(H, stride), convtile::conv_out(W, stride))) return 0;
    return 256 + 256 + convtile::align256(BWD_MAX_PART * sizeof(float));
}

int vkn_conv_dgrad_f32(const float* dr, const void* wimg_t, float* dx, int B, int Cin, int H, int W, int Cout, int ksize, int stride,
                       void* ws, size_t ws_bytes, void* stream) {
    if (!dr || !wimg_t || !dx) return VKN_E_ARG;
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return VKN_E_ARG;
    const size_t need = vkn_conv_dgrad_workspace_bytes(B, Cout, H, W, stride);
    if (!need || !convtile::chan_ok(Cin) || !convtile::conv_ok(ksize, stride) || !convtile::fits_i32(B, Cin, H, W) || H > 65535) return VKN_E_SHAPE;
    if (!ws || ws_bytes < need) return VKN_E_WORKSPACE;
    if (!vkn_aligned(dr, 16) || !vkn_aligned(wimg_t, 16) || !vkn_aligned(dx, 16) || !vkn_aligned(ws, 16)) return VKN_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    float* sc = reinterpret_cast<float*>(base + 256);
    const int Ho = convtile::conv_out(H, stride), Wo = convtile::conv_out(W, stride);
    const int rc = bwd_pow2(dr, (long long)B * Cout * Ho * Wo, reinterpret_cast<float*>(base + 512), sc, st);
    if (rc != VKN_OK) return rc;
    DgArgs a{};
    a.dr = dr;
    a.wscale = convtile::image_scale(wimg_t);
    a.wimg = convtile::image_frags(wimg_t);
    a.sc = sc;
    a.dx = dx;
    a.status = reinterpret_cast<unsigned*>(base);
    a.Cin = Cin;
    a.Cout = Cout;
    a.H = H;
    a.W = W;
    a.Ho = Ho;
    a.Wo = Wo;
    const int ntx = convtile::runs(Wo);
    const dim3 grid(ntx * stride, H, B * ((Cin + 255) / 256));
    if (ksize == 3 && stride == 1) hipLaunchKernelGGL((k_conv_dgrad<3, 1>), grid, dim3(convtile::THREADS), 0, st, a);
    else if (ksize == 3) hipLaunchKernelGGL((k_conv_dgrad<3, 2>), grid, dim3(convtile::THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_conv_dgrad<1, 1>), grid, dim3(convtile::THREADS), 0, st, a);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

}  // extern "C"
