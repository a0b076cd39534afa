// vkn_init.hip — helpers of the kernel-initialisation pass ("pass 0"): ConvKernelHead._decode_init_proposals after the
// loc / seg convs (reference: knet/det/kernel_head.py:204-263).  The two 1x1 convs are the decode kernel with frame-shared
// kernels, the object-feature einsum is the gather kernel; what is left is elementwise.
#include <hip/hip_runtime.h>

#include "vkn_common.h"
#include "vkn_launch.h"

#include "vkn_dectile.h"

// x_feats = semantic_feats + loc_feats                                   knet/det/kernel_head.py:238-241
__global__ __launch_bounds__(256) void k_add2(const float* __restrict__ a, const float* __restrict__ b,
                                              float* __restrict__ out, size_t n4, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4 va = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a) + i);
        const f32x4 vb = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(b) + i);
        reinterpret_cast<f32x4*>(out)[i] = va + vb;
    }
    // tail (n not a multiple of 4)
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = a[i] + b[i];
}

int vkn_launch_add2(const float* a, const float* b, float* out, size_t n, hipStream_t st) {
    const bool vec = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const size_t n4 = vec ? n / 4 : 0;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_add2, dim3((unsigned)blocks), dim3(256), 0, st, a, b, out, n4, n);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

// the same with 2-byte features (VKN_X_F16 / VKN_X_BF16): out = half(float(a) + float(b)), round-to-nearest-even — eight elements per thread
template <int XH>
__global__ __launch_bounds__(256) void k_add2h(const unsigned short* __restrict__ a, const unsigned short* __restrict__ b,
                                               unsigned short* __restrict__ out, size_t n8, size_t n) {
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
    auto up = [](unsigned short v) -> float {
        if (XH == 1) return (float)__builtin_bit_cast(_Float16, v);
        return __uint_as_float((unsigned)v << 16);
    };
    auto down = [](float v) -> unsigned short {
        if (XH == 1) return __builtin_bit_cast(unsigned short, (_Float16)v);
        return __builtin_bit_cast(unsigned short, (__bf16)v);
    };
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const u16x8 va = reinterpret_cast<const u16x8*>(a)[i], vb = reinterpret_cast<const u16x8*>(b)[i];
        u16x8 vo;
#pragma unroll
        for (int e = 0; e < 8; ++e) vo[e] = down(up(va[e]) + up(vb[e]));
        reinterpret_cast<u16x8*>(out)[i] = vo;
    }
    for (size_t i = n8 * 8 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = down(up(a[i]) + up(b[i]));
}

int vkn_launch_add2_half(const void* a, const void* b, void* out, size_t n, int xdt, hipStream_t st) {
    if (xdt != 1 && xdt != 2) return VKN_E_ARG;
    const bool vec = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const size_t n8 = vec ? n / 8 : 0;
    size_t blocks = (n8 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    const unsigned short *pa = static_cast<const unsigned short*>(a), *pb = static_cast<const unsigned short*>(b);
    unsigned short* po = static_cast<unsigned short*>(out);
    if (xdt == 1) hipLaunchKernelGGL(k_add2h<1>, dim3((unsigned)blocks), dim3(256), 0, st, pa, pb, po, n8, n);
    else hipLaunchKernelGGL(k_add2h<2>, dim3((unsigned)blocks), dim3(256), 0, st, pa, pb, po, n8, n);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

// proposal_feats[b][n] = init_w[n] (+ obj[b][n])  for n < Np;  = seg_w[nth + n - Np] for the concatenated stuff kernels
//                                                                           knet/det/kernel_head.py:234-236, 252-263
__global__ __launch_bounds__(64) void k_init_finish(const float* __restrict__ init_w, const float* __restrict__ obj,
                                                    const float* __restrict__ seg_w, float* __restrict__ out, int Np, int N,
                                                    int nth, int C) {
    const int row = blockIdx.x;  // b*N + n
    const int b = row / N, n = row - b * N;
    for (int c = threadIdx.x; c < C; c += 64) {
        float v;
        if (n < Np) {
            v = init_w[(size_t)n * C + c];
            if (obj) v += obj[((size_t)b * Np + n) * C + c];
        } else {
            v = seg_w[(size_t)(nth + n - Np) * C + c];
        }
        out[(size_t)row * C + c] = v;
    }
}

int vkn_launch_init_finish(const float* init_w, const float* obj, const float* seg_w, float* out, int B, int Np, int N, int nth,
                           int C, hipStream_t st) {
    hipLaunchKernelGGL(k_init_finish, dim3(B * N), dim3(64), 0, st, init_w, obj, seg_w, out, Np, N, nth, C);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

// ---------------------------------------------------------------------------------------------- pass 0 as ONE pass over loc and sem
// k_init_pass (round 6): the two 1x1 decodes (init_kernels . loc -> the Np thing logits, conv_seg . sem -> the ncls semantic logits),
// x = loc + sem, the stuff rows of mask_preds (= seg_preds[num_thing:]) and the thresholded thing bits for the kernel-init gather —
// one read of loc, one read of sem, one write of x (knet/det/kernel_head.py:222-257).  Before: k_decode_mfma(loc) + k_decode_mfma<NB=1>(sem)
// + a 2-D copy + k_add2 (which alone moved 3.2 GB per 32 frames) + a logits gather that read x and the logits again: 231 MB per frame;
// now 118 MB + the bit-word gather's read of x (34 MB).
//
// Structure = k_decode_mfma's, the decode tile engine of vkn_dectile.h (persistent 512-thread workgroup, kernel planes in LDS, a wave owns 64-px tiles as two interleaved 32-column
// MFMA strips, feature fragments straight from global memory in MFMA B layout, 8-byte buffer loads) with a fragment PAIR per k-step:
// the same 16 channels x 2 pixels of loc and of sem.  The 128 plane rows hold init_kernels in rows [0, Np) and conv_seg in rows
// [Np, Np + ncls): a row multiplies ONE of the two sources, so n-blocks below SLO see the loc fragments only, and in the mixed n-blocks the
// A fragment of the other source's rows is zeroed per lane (the accumulator then adds exact zeros: same bits as the separate decodes).
// x = loc + sem is formed from the pair in registers and stored with the loads' addressing (256-byte segments per channel row).
// NBL = n-blocks holding thing rows, [SLO, SHI] = n-blocks holding semantic rows — compile time (no branches around accumulators).

// logits of one 64-px tile -> their tensors: row < Np: mask_preds[b][row]; semantic row j = row - Np: seg_preds[b][j] (when wanted) and,
// with cat_stuff_mask, mask_preds[b][Np + j - num_thing] for j >= num_thing                    knet/det/kernel_head.py:222, 231-234, 255-257
// Buffer stores: n-blocks of thing rows only take the row offset in the SGPR operand (an opaque copy of P keeps the 64 row offsets from
// being hoisted into 64 SGPRs, as in k_decode_mfma); in the mixed n-blocks the destination row is a per-lane byte offset, and a lane
// whose row has no destination in a tensor stores to an offset past the buffer's range — dropped by the range check, no exec branches.
// This loop stays here, beside the engine's DECTILE_STORE_ROWS: with the thing-only n-blocks on that macro (per-lane offset from P, not
// from the opaque copy) k_init_pass<4, 3, 3> came out 196 instructions longer (profiles/dectile_resources.txt).
template <int NB, int SLO>
__device__ __forceinline__ void ip_store_tile(const f32x16 (&acc)[2][NB], const InitPassArgs& A, __amdgpu_buffer_rsrc_t mrs,
                                              __amdgpu_buffer_rsrc_t srs, int p0, int li, int g, int Ntot) {
    int Pq = A.P;
    asm volatile("" : "+s"(Pq));
    const int vst = ((4 * g) * Pq + 2 * li) << 2;
    const unsigned oor = 0x7FFFFFF0u;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row0 = nb * 32 + (r & 3) + 8 * (r >> 2);   // this lane's row is row0 + 4 g
            const dectile::u32x2 v = {__float_as_uint(acc[0][nb][r]), __float_as_uint(acc[1][nb][r])};
            if (nb < SLO) {
                __builtin_amdgcn_raw_buffer_store_b64(v, mrs, vst, (row0 * Pq + p0) << 2, 0);
            } else {
                const int row = row0 + 4 * g, j = row - A.Np;
                const int mrow = row < A.Np ? row : ((A.cat && row < Ntot && j >= A.nth) ? A.Np + j - A.nth : -1);
                const unsigned vm = mrow >= 0 ? (unsigned)((mrow * Pq + p0 + 2 * li) << 2) : oor;
                __builtin_amdgcn_raw_buffer_store_b64(v, mrs, (int)vm, 0, 0);
                const unsigned vs = (j >= 0 && row < Ntot) ? (unsigned)((j * Pq + p0 + 2 * li) << 2) : oor;
                __builtin_amdgcn_raw_buffer_store_b64(v, srs, (int)vs, 0, 0);
            }
        }
}

template <int NBL, int SLO, int SHI>
__global__ __launch_bounds__(dectile::THREADS, 2) void k_init_pass(const InitPassArgs A) {
    constexpr int NB = (NBL > SHI + 1) ? NBL : SHI + 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int C = A.C, P = A.P, KS = C >> 4;
    DECTILE_LDS(NB, smem, C, LDK, ldsH, ldsL)
    float* kbs = DECTILE_LDS_BIAS(NB, ldsL, LDK);
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, li = lane & 31;
    const int Ntot = A.Np + A.ncls;

    const int p_begin = blockIdx.x * A.px_per_wg, p_end = min(P, p_begin + A.px_per_wg);
    const int ntile = (p_end > p_begin) ? (p_end - p_begin) / dectile::TILE : 0;      // P % 64 == 0, px_per_wg % 512 == 0: whole tiles
    const int total = dectile::my_tiles(ntile, wave) * KS;

    const __amdgpu_buffer_rsrc_t lrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.loc + (size_t)b * C * P), 0, C * P * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.sem + (size_t)b * C * P), 0, C * P * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(A.x_out + (size_t)b * C * P, 0, C * P * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc(A.masks + (size_t)b * A.N * P, 0, A.N * P * 4, 0x00020000);
    // (seg_preds not wanted: a zero-sized buffer — every store to it is dropped)
    const __amdgpu_buffer_rsrc_t ers = __builtin_amdgcn_make_buffer_rsrc(A.seg ? A.seg + (size_t)b * A.ncls * P : A.masks, 0,
                                                                         A.seg ? A.ncls * P * 4 : 0, 0x00020000);

    dectile::u32x2 L0[8], S0[8], L1[8], S1[8];
    int ld_ks = 0, ld_sl = 0, ld_cnt = 0, c_ks = 0, c_sl = 0;
    const int voff = ((g << 3) * P + 2 * li) << 2;
#define IP_LOAD(LR, SR)                                                                                      \
    do {                                                                                                     \
        const int soff_ = ((ld_ks << 4) * P + DECTILE_TILE_P0(p_begin, wave, ld_sl)) << 2;           \
        _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                      \
            LR[e] = __builtin_amdgcn_raw_buffer_load_b64(lrs, voff, soff_ + ((e * P) << 2), 3);              \
            SR[e] = __builtin_amdgcn_raw_buffer_load_b64(srs, voff, soff_ + ((e * P) << 2), 3);              \
        }                                                                                                    \
        DECTILE_ADVANCE_LOAD(ld_ks, ld_sl, ld_cnt, total, KS)                                                \
    } while (0)

    if (total > 0) IP_LOAD(L0, S0);   // the first pair is requested before the planes are staged (its latency runs under the staging)
    {   // planes -> LDS (rows >= Np + ncls: zero), bias of the semantic rows
        DECTILE_STAGE_PLANES(NB, ldsH, ldsL, LDK, C, A.kh, A.kl, tid, r_ < Ntot)
        if (tid < NB * 32) kbs[tid] = (A.seg_b && tid >= A.Np && tid < Ntot) ? A.seg_b[tid - A.Np] : 0.f;
        __syncthreads();
    }
    if (total == 0) return;

    f32x16 acc[2][NB];
    // rows of this lane in the mixed n-blocks: thing (multiplies loc) or semantic (multiplies sem)
    bool thing_row[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) thing_row[nb] = (nb * 32 + li) < A.Np;
    const half8 hz = {0, 0, 0, 0, 0, 0, 0, 0};

#define IP_COMPUTE(LR, SR)                                                                                         \
    do {                                                                                                           \
        if (c_ks == 0) {                                                                                           \
            DECTILE_BIAS_ACC(acc, NB, kbs, lane)                                                                   \
        }                                                                                                          \
        const int p0_ = DECTILE_TILE_P0(p_begin, wave, c_sl);                                              \
        {   /* x = loc + sem for the pair's 16 channels x 2 pixels */                                              \
            const int soff_ = ((c_ks << 4) * P + p0_) << 2;                                                        \
            _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                        \
                const dectile::u32x2 v_ = {__float_as_uint(__uint_as_float(LR[e][0]) + __uint_as_float(SR[e][0])),       \
                                     __float_as_uint(__uint_as_float(LR[e][1]) + __uint_as_float(SR[e][1]))};      \
                __builtin_amdgcn_raw_buffer_store_b64(v_, xrs, voff, soff_ + ((e * P) << 2), 0);                   \
            }                                                                                                      \
        }                                                                                                          \
        const int cb_ = (c_ks << 4) + (g << 3);                                                                    \
        half8 bh0, bl0, bh1, bl1;                                                                                  \
        DECTILE_SPLIT_PAIR(LR, bh0, bl0, bh1, bl1)                                                                                              \
        _Pragma("unroll") for (int nb = 0; nb < NBL; ++nb) {                                                       \
            const _Float16* ap_ = ldsH + (nb * 32 + li) * LDK + cb_;                                               \
            half8 ah_ = *reinterpret_cast<const half8*>(ap_);                                                      \
            half8 al_ = *reinterpret_cast<const half8*>(ap_ + NB * 32 * LDK);                                      \
            if (nb >= SLO) { ah_ = thing_row[nb] ? ah_ : hz; al_ = thing_row[nb] ? al_ : hz; }                     \
            dectile::mfma6(ah_, al_, bh0, bl0, bh1, bl1, acc[0][nb], acc[1][nb]);                                                                                \
        }                                                                                                          \
        DECTILE_SPLIT_PAIR(SR, bh0, bl0, bh1, bl1)                                                                                              \
        _Pragma("unroll") for (int nb = SLO; nb <= SHI; ++nb) {                                                    \
            const _Float16* ap_ = ldsH + (nb * 32 + li) * LDK + cb_;                                               \
            half8 ah_ = *reinterpret_cast<const half8*>(ap_);                                                      \
            half8 al_ = *reinterpret_cast<const half8*>(ap_ + NB * 32 * LDK);                                      \
            ah_ = thing_row[nb] ? hz : ah_; al_ = thing_row[nb] ? hz : al_;                                        \
            dectile::mfma6(ah_, al_, bh0, bl0, bh1, bl1, acc[0][nb], acc[1][nb]);                                                                                \
        }                                                                                                          \
        if (++c_ks == KS) {                                                                                        \
            ip_store_tile<NB, SLO>(acc, A, mrs, ers, p0_, li, g, Ntot);                                            \
            if (A.bits) dectile::emit_bits<NB>(acc, A.thr, A.bits + ((size_t)b * (P >> 5) + ((p0_ >> 6) << 1)) * A.npt, A.npt, lane); \
            c_ks = 0;                                                                                              \
            ++c_sl;                                                                                                \
        }                                                                                                          \
    } while (0)

    for (int f = 0; f < total; f += 2) {   // pairs double-buffered: the next pair's 16 loads are in flight behind this pair's 30 MFMA groups
        IP_LOAD(L1, S1);
        IP_COMPUTE(L0, S0);
        if (f + 1 >= total) break;
        IP_LOAD(L0, S0);
        IP_COMPUTE(L1, S1);
    }
#undef IP_LOAD
#undef IP_COMPUTE
}

// pass 0 in one pass (see k_init_pass): supported when every thing and semantic row fits the 128 plane rows in one of the built row maps
int vkn_init_pass_supported(int Np, int ncls, int C, int P) {
    if (Np <= 0 || ncls <= 0 || C % 16 != 0 || C > 256 || (P % 64) != 0) return 0;
    if ((size_t)C * P * 4 >= ((size_t)1 << 31)) return 0;
    const int nbl = (Np + 31) / 32, slo = Np / 32, shi = (Np + ncls - 1) / 32;
    if (nbl == 4 && slo == 3 && shi == 3) return 1;     // Np in [97, 127], Np + ncls <= 128: 100 proposals + 19 classes (the STEP configs)
    if (nbl == 1 && slo == 0 && shi == 0) return 2;     // everything in one n-block (the tiny goldens)
    return 0;
}
int vkn_launch_init_pass(const InitPassArgs& a, int B, hipStream_t st) {
    const int kind = vkn_init_pass_supported(a.Np, a.ncls, a.C, a.P);
    if (!kind) return VKN_E_SHAPE;
    InitPassArgs A = a;
    A.px_per_wg = vkn_decode_split(B, a.P, 0).px_per_wg;   // one persistent workgroup per CU over the batch when it is large enough
    const dim3 grid((a.P + A.px_per_wg - 1) / A.px_per_wg, B);
    const size_t lds = dectile::lds_bytes(kind == 1 ? 4 : 1, a.C);
    if (kind == 1) {
        VKN_ALLOW_FULL_LDS((k_init_pass<4, 3, 3>));
        hipLaunchKernelGGL((k_init_pass<4, 3, 3>), grid, dim3(dectile::THREADS), lds, st, A);
    } else {
        VKN_ALLOW_FULL_LDS((k_init_pass<1, 0, 0>));
        hipLaunchKernelGGL((k_init_pass<1, 0, 0>), grid, dim3(dectile::THREADS), lds, st, A);
    }
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}
