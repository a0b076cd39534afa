// vkn_convtile.h — the conv tile engine of the FPN block, written once for its forward (vkn_fpn.hip: k_fpn_conv), its input gradient
// (vkn_fpn_bwd.hip: k_conv_dgrad) and, where the tile is the same, its weight gradient (k_conv_wgrad).  Include after vkn_common.h.
// Device functions and inline host helpers only, no kernel: two objects include it and the library links without device linking.
//
//   * the tile: a workgroup of THREADS = 4 waves owns 256 channels x one TILE = 64-pixel run; wave w owns channels 64 w .. 64 w + 63 (two
//     32-row MFMA blocks, `WaveMap`) x the run (two 32-column blocks): `f32x16 acc[2][2] = {}`, [channel block q][pixel block pb];
//   * the B operand: KC = 32 channels of a patch in LDS as f16 hi / lo planes [row][column][channel], PITCH halfs per column, written
//     by `stage` (which also keeps the |v| < 65504 flag of the f16 split's envelope);
//   * the A operand: the prepared weight image, {scale, 1 / scale} in an IMG_HDR-byte header, then the fragments
//     [tap][ci / 16][co / 32][hi, lo][lane][8] (`frag_index`): k_fpn_wsplit writes them, k_fpn_conv and k_conv_dgrad read them;
//   * `tap_product`: one tap of one staged chunk into the accumulator tile, v_mfma_f32_32x32x16_f16 with the two-term split of
//     vkn_common.h (hi*hi + hi*lo + lo*hi).  The order of the MFMAs is part of the results (fp32 accumulation): k-step, pixel block,
//     channel block, then the three terms;
//   * `gn_preact`: the GroupNorm pre-activation.  The forward's ReLU and the backward's mask are the sign of this one expression;
//   * `block_absmax` + `pow2_scale`: the power of two that brings a tensor's max |v| into [2^14, 2^15), for the weight image and for the
//     backward's operands alike.  The exponent is clamped at -100 so that 2^(15 - e) stays finite: a weight matrix whose max |w| is
//     below 2^-101 (one below 2^-112 had an INFINITE scale before the two rules became one) is scaled by 2^115.
#pragma once

namespace convtile {

constexpr int THREADS = 256;
constexpr int TILE = 64;      // pixels per workgroup (one row run)
constexpr int KC = 32;        // channels per staged chunk (two MFMA k-steps)
constexpr int PITCH = 40;     // halfs per patch column: 32 channels + 8 pad (80-byte stride, 16-byte aligned fragment reads)
constexpr int IMG_HDR = 256;  // prepared image: {scale, 1 / scale}, then the fragments from byte 256

// ---- the prepared image.  Fragment (tap, ks, cb, lo) is 64 lanes x 8 halfs; lane l holds W[co = 32 cb + (l & 31)][ci = 16 ks + 8 (l >> 5) + j]
__host__ __device__ __forceinline__ size_t frag_index(int tap, int nks, int ks, int ncb, int cb, int lo, int lane) {  // in half8 units
    return ((((size_t)tap * nks + ks) * ncb + cb) * 2 + lo) * 64 + lane;
}
inline size_t image_bytes(int Cout, int Cin, int taps) { return IMG_HDR + (size_t)taps * Cin * Cout * 2 * sizeof(_Float16); }
inline const float* image_scale(const void* image) { return static_cast<const float*>(image); }
inline const _Float16* image_frags(const void* image) { return reinterpret_cast<const _Float16*>(static_cast<const char*>(image) + IMG_HDR); }

// ---- the accumulator tile
struct WaveMap {
    int cb0;          // the wave's first 32-channel block
    bool has0, has1;  // ... exists, and so does the second
};
__device__ __forceinline__ WaveMap wave_map(int group, int wave, int ncb) {  // group: which 256 channels the workgroup owns
    const int cb0 = group * 8 + wave * 2;
    return {cb0, cb0 < ncb, cb0 + 1 < ncb};
}
// The tile is zeroed where it is declared, `f32x16 acc[2][2] = {};`.  A helper here that zeroes it through a reference compiles both kernels
// to another prologue and measured up to 1 % slower on the forward (profiles/convtile_resources.txt, profiles/convtile_ab.txt).

// ---- staging: the f16 split of one operand value, and whether it left the split's envelope
__device__ __forceinline__ void range_split(float v, unsigned& bad, _Float16& h, _Float16& l) {
    bad |= !(fabsf(v) < 65504.f);
    vkn_split_f16(v, h, l);
}
__device__ __forceinline__ void stage(float v, unsigned& bad, _Float16* lhi, _Float16* llo, int o) {
    _Float16 h, l;
    range_split(v, bad, h, l);
    lhi[o] = h;
    llo[o] = l;
}

// ---- one tap of the staged chunk c0 .. c0 + KC - 1.  `b0`: where the lane's pixel (lane & 31) of pixel block 0 stands in the planes under
// this tap, in halfs; `pbstride`: from there to pixel block 1.  A wave with one channel block (!has1) computes it twice.
__device__ __forceinline__ void tap_product(f32x16 (&acc)[2][2], const half8* wimg, int tap, int nks, int ncb, int c0, int cb0, bool has1,
                                            int lane, const _Float16* lhi, const _Float16* llo, int b0, int pbstride) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int ks = (c0 >> 4) + s;
        half8 ah[2], al[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int cb = has1 ? cb0 + q : cb0;
            ah[q] = wimg[frag_index(tap, nks, ks, ncb, cb, 0, lane)];
            al[q] = wimg[frag_index(tap, nks, ks, ncb, cb, 1, lane)];
        }
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            const int o = b0 + pb * pbstride + s * 16 + (lane >> 5) * 8;
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

// ---- GroupNorm before the max with 0
__device__ __forceinline__ float gn_preact(float v, float mean, float rstd, float gamma, float beta) { return (v - mean) * rstd * gamma + beta; }

// ---- the power of two of one tensor.  block_absmax: the maximum over a 256-thread workgroup, in every thread
__device__ __forceinline__ float block_absmax(float m) {
    __shared__ float red[256];
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    return red[0];
}
// sc = {2^(15 - e), 2^(e - 15)} with mx = f 2^e, f in [0.5, 1); {1, 1} for an all-zero or non-finite tensor (staging flags the latter)
__device__ __forceinline__ void pow2_scale(float mx, float* sc) {
    int e = 15;
    if (mx > 0.f && mx < INFINITY) frexpf(mx, &e);
    e = max(e, -100);  // 2^(15 - e) stays finite
    sc[0] = ldexpf(1.f, 15 - e);
    sc[1] = ldexpf(1.f, e - 15);
}

// ---- host side: sizes and the envelope of the block's kernels
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int conv_out(int n, int stride) { return (n - 1) / stride + 1; }  // 3x3 pad 1 and 1x1 pad 0: ceil(n / stride)
inline int runs(int Wo) { return (Wo + TILE - 1) / TILE; }
inline bool chan_chunks(int C) { return C > 0 && C % KC == 0; }  // what an image can hold ...
inline bool chan_ok(int C) { return chan_chunks(C) && C <= 512; }  // ... and what the kernels take
inline bool conv_ok(int ksize, int stride) { return (ksize == 3 && (stride == 1 || stride == 2)) || (ksize == 1 && stride == 1); }
inline bool fits_i32(int B, int C, int H, int W) { return (long long)B * C * H * W * 4 < (1ll << 31); }

}  // namespace convtile
