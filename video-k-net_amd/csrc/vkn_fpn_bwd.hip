// vkn_fpn_bwd.hip — backward of one localization-FPN block y = ReLU(GN(conv(x))) (include/vkn_fpn_train.h), the forward being
// vkn_conv_gn_f32 of vkn_fpn.hip.  Four entry points:
//   * vkn_gn_relu_apply_f32: the block's output materialised from the raw conv output and its statistics;
//   * vkn_gn_relu_bwd_f32: GroupNorm + ReLU backward.  Sums per (frame, channel, 2048-pixel run) in fp32 per thread, fp64 per
//     workgroup; one workgroup per group merges them in a fixed order in fp64; then the elementwise pass;
//   * vkn_conv_wgrad_f32: dW = dr x^T over B Ho Wo, on v_mfma_f32_32x32x16_f16 with the two-term f16 split of vkn_common.h.  k (the
//     reduction) runs over the 64 pixels of an output-row run, so BOTH operands need 8 consecutive pixels per lane: dr straight
//     from memory, the input patch through LDS as one shifted copy per kx ([kx][ci][pixel], aligned 16-byte reads at any stride);
//   * vkn_conv_dgrad_f32: dx in gather form on the forward's tiling (256 output rows x 64 pixels per workgroup, 32-channel chunks
//     in LDS as [row][column][channel]); the A operand is the forward's prepared image of the flipped, transposed weight.
// Operand range: both MFMA kernels stage v * 2^e, 2^e per tensor from its max |v| (k_bwd_absmax_*), and undo it in the epilogue.
#include "../../include/vkn_fpn_train.h"
#include "vkn_common.h"

#include <algorithm>

#define BWD_THREADS 256
#define BWD_TILE 64      // pixels per run (vkn_fpn.hip: FPN_TILE)
#define BWD_KC 32        // channels per staged chunk (FPN_KC)
#define BWD_PITCH 40     // dgrad: halfs per patch column, 32 channels + 8 pad (FPN_PITCH)
#define BWD_XP 72        // wgrad: halfs per (kx, channel) row, 64 pixels + 8 pad (144-byte stride: 16 lanes cover the 64 banks once)
#define BWD_XW 66        // dgrad: patch columns, 64 + one on either side
#define BWD_IMG_HDR 256  // prepared image: {scale, 1 / scale}, fragments from byte 256 (vkn_fpn.hip: FPN_IMG_HDR)
#define BWD_MAX_PART 256 // workgroups of the max |v| pass

// ------------------------------------------------------------------------------------------------ power of two of one tensor
__global__ __launch_bounds__(256) void k_bwd_absmax_part(const float* __restrict__ x, long long n, float* __restrict__ part) {
    __shared__ float red[256];
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// sc = {2^e, 2^-e} with max |v| 2^e in [2^14, 2^15); 1 for an all-zero or non-finite tensor (the staging pass flags the latter)
__global__ __launch_bounds__(256) void k_bwd_absmax_fin(const float* __restrict__ part, int nblk, float* __restrict__ sc) {
    __shared__ float red[256];
    red[threadIdx.x] = (int)threadIdx.x < nblk ? part[threadIdx.x] : 0.f;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int e = 15;
        const float mx = red[0];
        if (mx > 0.f && mx < INFINITY) frexpf(mx, &e);  // mx = f 2^e, f in [0.5, 1)
        e = max(e, -100);                               // 2^(15 - e) stays finite
        sc[0] = ldexpf(1.f, 15 - e);
        sc[1] = ldexpf(1.f, e - 15);
    }
}

// ------------------------------------------------------------------------------------------------ GroupNorm + ReLU
// the forward's own expression (vkn_fpn.hip: fpn_norm, k_fpn_gn_apply) before the max with 0
__device__ __forceinline__ float bwd_preact(float v, float mean, float rstd, float ga, float be) { return (v - mean) * rstd * ga + be; }

__global__ __launch_bounds__(256) void k_gnb_fwd(const float* r, const float* __restrict__ st, int G, int cpg,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float* y, int C,
                                                 long long P) {
    const int b = blockIdx.y;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < (long long)C * P; i += (long long)gridDim.x * 256) {
        const int c = (int)(i / P);
        const float* s = st + 2 * ((long long)b * G + c / cpg);
        const long long o = (long long)b * C * P + i;
        y[o] = fmaxf(bwd_preact(r[o], s[0], s[1], gamma[c], beta[c]), 0.f);
    }
}

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
        const float dz = bwd_preact(v, mean, rstd, ga, be) > 0.f ? d : 0.f;
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
        float g = (bwd_preact(v, mean, rstd, ga, beta[c]) > 0.f ? dy[o] : 0.f) * ga;
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
__global__ __launch_bounds__(BWD_THREADS) void k_conv_wgrad(WgArgs a) {
    constexpr int PAD = KS / 2;
    constexpr int PL = KS * BWD_KC * BWD_XP;  // halfs per plane
    __shared__ __attribute__((aligned(16))) _Float16 wg_lds[2 * PL];
    _Float16* lhi = wg_lds;
    _Float16* llo = wg_lds + PL;
    const int ci0 = blockIdx.x * BWD_KC, sp = blockIdx.z;
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
        const int ox0 = tx * BWD_TILE;
        // A operand: lane l holds dr[co0 + (l & 31)][oy][ox0 + 16 ks + 8 (l >> 5) + j], j = 0..7, of k-step ks
        half8 ah[4], al[4];
        if (has) {
            const float* p = a.dr + (((long long)b * a.Cout + co0 + (lane & 31)) * a.Ho + oy) * a.Wo;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int ox = ox0 + ks * 16 + (lane >> 5) * 8 + j;
                    const float v = ox < a.Wo ? p[ox] * sdr : 0.f;
                    bad |= !(fabsf(v) < 65504.f);
                    _Float16 h, l;
                    vkn_split_f16(v, h, l);
                    ah[ks][j] = h;
                    al[ks][j] = l;
                }
        }
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
            const int iy = oy * S + ky - PAD;
            __syncthreads();  // the previous row's fragment reads are done
            for (int e = threadIdx.x; e < KS * BWD_KC * BWD_TILE; e += BWD_THREADS) {
                const int j = e % BWD_TILE, ci = (e / BWD_TILE) % BWD_KC, kx = e / (BWD_TILE * BWD_KC);
                const int ox = ox0 + j, ix = ox * S + kx - PAD;
                float v = 0.f;  // zero padding of the conv input, and the columns past the run's end
                if (ox < a.Wo && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                    v = a.x[(((long long)b * a.Cin + ci0 + ci) * a.H + iy) * a.W + ix] * sx;
                bad |= !(fabsf(v) < 65504.f);
                _Float16 h, l;
                vkn_split_f16(v, h, l);
                const int o = (kx * BWD_KC + ci) * BWD_XP + j;
                lhi[o] = h;
                llo[o] = l;
            }
            __syncthreads();
            if (has) {
#pragma unroll
                for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        // B operand: lane l holds x[ci0 + (l & 31)][iy][(ox0 + 16 ks + 8 (l >> 5) + j) S + kx - PAD]
                        const int o = (kx * BWD_KC + (lane & 31)) * BWD_XP + ks * 16 + (lane >> 5) * 8;
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
__global__ __launch_bounds__(BWD_THREADS) void k_conv_dgrad(DgArgs a) {
    constexpr int PAD = KS / 2;
    constexpr int PL = KS * BWD_XW * BWD_PITCH;  // halfs per plane
    __shared__ __attribute__((aligned(16))) _Float16 dg_lds[2 * PL];
    _Float16* lhi = dg_lds;
    _Float16* llo = dg_lds + PL;
    const int ncig = (a.Cin + 255) >> 8;
    const int par = blockIdx.x % S, tx = blockIdx.x / S, iy = blockIdx.y, b = blockIdx.z / ncig, cig = blockIdx.z % ncig;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ncb = a.Cin >> 5, nks = a.Cout >> 4;
    const int cb0 = cig * 8 + wave * 2;
    const bool has0 = cb0 < ncb, has1 = cb0 + 1 < ncb;
    const int x0 = tx * BWD_TILE;
    f32x16 acc[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][pb][r] = 0.f;
    const float sdr = a.sc[0];
    unsigned bad = 0;
    const half8* wimg = reinterpret_cast<const half8*>(a.wimg);
    for (int c0 = 0; c0 < a.Cout; c0 += BWD_KC) {
        for (int e = threadIdx.x; e < BWD_KC * KS * BWD_XW; e += BWD_THREADS) {
            const int j = e % BWD_XW, ky = (e / BWD_XW) % KS, co = e / (BWD_XW * KS);
            const int t = iy + PAD - ky, ox = x0 - 1 + j;
            float v = 0.f;
            if (t >= 0 && t % S == 0 && t / S < a.Ho && ox >= 0 && ox < a.Wo)
                v = a.dr[(((long long)b * a.Cout + c0 + co) * a.Ho + t / S) * a.Wo + ox] * sdr;
            bad |= !(fabsf(v) < 65504.f);
            _Float16 h, l;
            vkn_split_f16(v, h, l);
            const int o = (ky * BWD_XW + j) * BWD_PITCH + co;
            lhi[o] = h;
            llo[o] = l;
        }
        __syncthreads();
        if (has0) {
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
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int ks = (c0 >> 4) + s;
                        half8 ah[2], al[2];
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const int cb = has1 ? cb0 + q : cb0;
                            const half8* p = wimg + ((((size_t)tap * nks + ks) * ncb + cb) * 2) * 64 + lane;
                            ah[q] = p[0];
                            al[q] = p[64];
                        }
#pragma unroll
                        for (int pb = 0; pb < 2; ++pb) {
                            const int o = (ky * BWD_XW + pb * 32 + (lane & 31) + dxo + 1) * BWD_PITCH + s * 16 + (lane >> 5) * 8;
                            const half8 bh = *reinterpret_cast<const half8*>(lhi + o);
                            const half8 bl = *reinterpret_cast<const half8*>(llo + o);
#pragma unroll
                            for (int q = 0; q < 2; ++q) {
                                acc[q][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[q], bh, acc[q][pb], 0, 0, 0);
                                acc[q][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[q], bl, acc[q][pb], 0, 0, 0);
                                acc[q][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[q], bh, acc[q][pb], 0, 0, 0);
                            }
                        }
                    }
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

inline size_t bwd_align(size_t v) { return (v + 255) & ~(size_t)255; }
inline int bwd_out(int n, int s) { return (n - 1) / s + 1; }
inline bool bwd_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool bwd_fits(int B, int C, int H, int W) { return (long long)B * C * H * W * 4 < (1ll << 31); }
inline bool bwd_chan(int C) { return C > 0 && C % 32 == 0 && C <= 512; }
inline bool bwd_conv_ok(int ksize, int stride) { return (ksize == 3 && (stride == 1 || stride == 2)) || (ksize == 1 && stride == 1); }

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
    off += bwd_align((size_t)B * C * w.nrun * 2 * sizeof(double));
    w.S = off;
    off += bwd_align((size_t)B * C * 2 * sizeof(double));
    w.gm = off;
    off += bwd_align((size_t)B * G * 2 * sizeof(float));
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
    const int Ho = bwd_out(H, stride), Wo = bwd_out(W, stride);
    w.ntx = (Wo + BWD_TILE - 1) / BWD_TILE;
    w.nruns = (long long)B * Ho * w.ntx;
    const int tiles = (Cin / BWD_KC) * ((Cout + 127) / 128);
    long long ns = std::max(1, VKN_FPN_WGRAD_TARGET_WGS / tiles);
    ns = std::min<long long>(ns, std::min<long long>(VKN_FPN_WGRAD_MAX_SPLITS, w.nruns));
    w.nsplit = (int)ns;
    size_t off = 256;
    w.sc = off;
    off += 256;
    w.amax = off;
    off += bwd_align(BWD_MAX_PART * sizeof(float));
    w.part = off;
    off += bwd_align((size_t)w.nsplit * Cout * Cin * ksize * ksize * sizeof(float));
    w.total = off;
    return w;
}

}  // namespace

extern "C" {

int vkn_gn_relu_apply_f32(const float* r, const float* stats, const float* gamma, const float* beta, int groups, float* y, int B, int C,
                          int H, int W, void* stream) {
    if (!r || !stats || !gamma || !beta || !y) return VKN_E_ARG;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return VKN_E_ARG;
    if (!bwd_chan(C) || groups <= 0 || C % groups || !bwd_fits(B, C, H, W)) return VKN_E_SHAPE;
    for (const void* p : {(const void*)r, (const void*)stats, (const void*)gamma, (const void*)beta, (const void*)y})
        if (!bwd_aligned(p)) return VKN_E_ALIGN;
    const long long P = (long long)H * W, n = (long long)C * P;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_gnb_fwd, dim3(blocks, B), dim3(256), 0, static_cast<hipStream_t>(stream), r, stats, groups, C / groups, gamma,
                       beta, y, C, P);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

size_t vkn_gn_relu_bwd_workspace_bytes(int B, int C, int H, int W, int groups) {
    if (B <= 0 || H <= 0 || W <= 0 || !bwd_chan(C) || groups <= 0 || C % groups || !bwd_fits(B, C, H, W)) return 0;
    return gnb_carve(B, C, H, W, groups).total;
}

int vkn_gn_relu_bwd_f32(const float* dy, const float* r, const float* stats, const float* gamma, const float* beta, int groups, float* dr,
                        float* dgamma, float* dbeta, int B, int C, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !r || !stats || !gamma || !beta || !dr || !dgamma || !dbeta) return VKN_E_ARG;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return VKN_E_ARG;
    if (!bwd_chan(C) || groups <= 0 || C % groups || !bwd_fits(B, C, H, W) || B > 65535) return VKN_E_SHAPE;
    const GnbWs w = gnb_carve(B, C, H, W, groups);
    if (!ws || ws_bytes < w.total) return VKN_E_WORKSPACE;
    for (const void* p : {(const void*)dy, (const void*)r, (const void*)stats, (const void*)gamma, (const void*)beta, (const void*)dr,
                          (const void*)dgamma, (const void*)dbeta, (const void*)ws})
        if (!bwd_aligned(p)) return VKN_E_ALIGN;
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
    if (B <= 0 || H <= 0 || W <= 0 || !bwd_chan(Cin) || !bwd_chan(Cout) || !bwd_conv_ok(ksize, stride)) return 0;
    if (!bwd_fits(B, Cin, H, W) || !bwd_fits(B, Cout, bwd_out(H, stride), bwd_out(W, stride))) return 0;
    return wg_carve(B, Cin, H, W, Cout, ksize, stride).total;
}

int vkn_conv_wgrad_f32(const float* dr, const float* x, float* dw, int B, int Cin, int H, int W, int Cout, int ksize, int stride, void* ws,
                       size_t ws_bytes, void* stream) {
    if (!dr || !x || !dw) return VKN_E_ARG;
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return VKN_E_ARG;
    if (!vkn_conv_wgrad_workspace_bytes(B, Cin, H, W, Cout, ksize, stride)) return VKN_E_SHAPE;
    const WgWs w = wg_carve(B, Cin, H, W, Cout, ksize, stride);
    if (!ws || ws_bytes < w.total) return VKN_E_WORKSPACE;
    if (!bwd_aligned(dr) || !bwd_aligned(x) || !bwd_aligned(dw) || !bwd_aligned(ws)) return VKN_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    float* sc = reinterpret_cast<float*>(base + w.sc);
    float* amax = reinterpret_cast<float*>(base + w.amax);
    const int Ho = bwd_out(H, stride), Wo = bwd_out(W, stride);
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
    const dim3 grid(Cin / BWD_KC, (Cout + 127) / 128, w.nsplit);
    if (ksize == 3 && stride == 1) hipLaunchKernelGGL((k_conv_wgrad<3, 1>), grid, dim3(BWD_THREADS), 0, st, a);
    else if (ksize == 3) hipLaunchKernelGGL((k_conv_wgrad<3, 2>), grid, dim3(BWD_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_conv_wgrad<1, 1>), grid, dim3(BWD_THREADS), 0, st, a);
    VKN_CHECK_LAUNCH();
    const long long n = (long long)Cout * Cin * ksize * ksize;
    hipLaunchKernelGGL(k_wgrad_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.part, w.nsplit, n, dw);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

size_t vkn_conv_dgrad_workspace_bytes(int B, int Cout, int H, int W, int stride) {
    if (B <= 0 || H <= 0 || W <= 0 || !bwd_chan(Cout) || (stride != 1 && stride != 2)) return 0;
    if (!bwd_fits(B, Cout, bwd_out(H, stride), bwd_out(W, stride))) return 0;
    return 256 + 256 + bwd_align(BWD_MAX_PART * sizeof(float));
}

int vkn_conv_dgrad_f32(const float* dr, const void* wimg_t, float* dx, int B, int Cin, int H, int W, int Cout, int ksize, int stride,
                       void* ws, size_t ws_bytes, void* stream) {
    if (!dr || !wimg_t || !dx) return VKN_E_ARG;
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return VKN_E_ARG;
    const size_t need = vkn_conv_dgrad_workspace_bytes(B, Cout, H, W, stride);
    if (!need || !bwd_chan(Cin) || !bwd_conv_ok(ksize, stride) || !bwd_fits(B, Cin, H, W) || H > 65535) return VKN_E_SHAPE;
    if (!ws || ws_bytes < need) return VKN_E_WORKSPACE;
    if (!bwd_aligned(dr) || !bwd_aligned(wimg_t) || !bwd_aligned(dx) || !bwd_aligned(ws)) return VKN_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    float* sc = reinterpret_cast<float*>(base + 256);
    const int Ho = bwd_out(H, stride), Wo = bwd_out(W, stride);
    const int rc = bwd_pow2(dr, (long long)B * Cout * Ho * Wo, reinterpret_cast<float*>(base + 512), sc, st);
    if (rc != VKN_OK) return rc;
    DgArgs a{};
    a.dr = dr;
    a.wscale = static_cast<const float*>(wimg_t);
    a.wimg = reinterpret_cast<const _Float16*>(static_cast<const char*>(wimg_t) + BWD_IMG_HDR);
    a.sc = sc;
    a.dx = dx;
    a.status = reinterpret_cast<unsigned*>(base);
    a.Cin = Cin;
    a.Cout = Cout;
    a.H = H;
    a.W = W;
    a.Ho = Ho;
    a.Wo = Wo;
    const int ntx = (bwd_out(W, stride) + BWD_TILE - 1) / BWD_TILE;
    const dim3 grid(ntx * stride, H, B * ((Cin + 255) / 256));
    if (ksize == 3 && stride == 1) hipLaunchKernelGGL((k_conv_dgrad<3, 1>), grid, dim3(BWD_THREADS), 0, st, a);
    else if (ksize == 3) hipLaunchKernelGGL((k_conv_dgrad<3, 2>), grid, dim3(BWD_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_conv_dgrad<1, 1>), grid, dim3(BWD_THREADS), 0, st, a);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

}  // extern "C"
