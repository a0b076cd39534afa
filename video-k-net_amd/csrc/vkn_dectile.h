// vkn_dectile.h — the decode tile engine: the x-streaming MFMA decode written once for the mask decode (vkn_decode.hip: k_decode_mfma)
// and for pass 0 (vkn_init.hip: k_init_pass).  Include after vkn_common.h.  Device functions, macros and inline host helpers, no kernel.
//
//   * the tile: a persistent workgroup of THREADS = 8 waves; a wave owns TILE = 64-pixel tiles = two interleaved 32-column MFMA strips
//     (even / odd pixels), `f32x16 acc[2][NB]` = [strip][n-block of 32 rows]; tile `slot` of a wave starts at `DECTILE_TILE_P0`;
//   * the A operand: NB * 32 kernel rows in dynamic LDS as two f16 planes (hi / lo split of the fp32 values) of ldk(C) halfs per row,
//     then their fp32 bias (`DECTILE_LDS`, `DECTILE_LDS_BIAS`); `DECTILE_STAGE_PLANES` fills the planes, `DECTILE_BIAS_ACC` starts the accumulators from the bias;
//   * the B operand: fragments straight from global memory, a lane's pixel pair x 8 channels as eight dword pairs; `DECTILE_SPLIT_PAIR` is their
//     hi / lo split, `mfma6` the three-term product (hi*hi, hi*lo, lo*hi) on the two strips, alternating so that dependent MFMAs are
//     never back to back.  Per accumulator that order is part of the results;
//   * the cursor: five ints, which fragment of the wave's (tile, k-step) sequence is loaded next (`DECTILE_ADVANCE_LOAD`) and consumed next;
//   * the epilogues: `DECTILE_STORE_ROWS` (a whole tile's 32 rows of one tensor, 8-byte buffer stores) and `emit_bits` (the bit words that
//     vkn_gather.hip consumes).
//
// Most pieces are macros on the kernels' own locals, not functions on structs: both kernels sit at their register limit (pass 0 at 256 VGPRs
// with spills), and only the macro forms compile to the instruction streams the kernels had with these lines written out in each of them
// (profiles/dectile_resources.txt).  Macro names are global; their locals end in `_`.
#pragma once

namespace dectile {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int THREADS = 512;
constexpr int WAVES = 8;
constexpr int TILE = 64;  // pixels per wave tile: two interleaved 32-column MFMA strips (even / odd pixels)
__host__ __device__ constexpr int ldk(int C) { return C + 8; }  // halfs per LDS row; (C+8)*2 B = odd multiple of 16 B -> b128 reads conflict-free
inline size_t lds_bytes(int NB, int C) { return (size_t)2 * NB * 32 * ldk(C) * sizeof(_Float16) + (size_t)NB * 32 * sizeof(float); }

// of a workgroup's `ntile` tiles wave `wave` owns my_tiles
__device__ __forceinline__ int my_tiles(int ntile, int wave) { return (ntile > wave) ? (ntile - wave + WAVES - 1) / WAVES : 0; }

// one n-block x 16 channels on both strips; the two accumulators alternate so dependent MFMAs are never back to back
__device__ __forceinline__ void mfma6(half8 ah, half8 al, half8 bh0, half8 bl0, half8 bh1, half8 bl1, f32x16& acc0, f32x16& acc1) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh1, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl1, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh1, acc1, 0, 0, 0);
}

// ---- bit-packed output (intermediate stages of the fused head, pass 0's thing bits): instead of the logits, emit bit(z >= thr) — all the
// next stage's gather consumes — as words[B][P/64][2][NPT]: for 64-px tile T and row n, word [T][0][n] bit i = pixel 64 T + 2 i
// (even pixels = MFMA strip 0) and word [T][1][n] bit i = pixel 64 T + 2 i + 1 (strip 1).  That is exactly what the two ballots of
// a C/D register deliver, so the epilogue is 2 v_cmp + 4 selects per register pair and four 256-B row stores per tile (a first
// version that interleaved the two ballots into pixel order on the scalar unit cost as much as the logits stores it replaced:
// one SALU serves the whole CU).  The gather's byte -> fragment table absorbs the even/odd split.
// Cuts the stage hand-off from 2 x 15.3 MB to 2 x 0.5 MB per frame.  wbase: word [T][0][first row of acc].
template <int NB>
__device__ __forceinline__ void emit_bits(const f32x16 (&acc)[2][NB], float thr, unsigned* __restrict__ wbase, int NPT, int lane) {
    constexpr int NH = (NB * 32 + 63) / 64;
    int w[2][NH];  // [even | odd pixels][row half]: lane = row & 63
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int h = 0; h < NH; ++h) w[t][h] = 0;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned long long m0 = __ballot(acc[0][nb][r] >= thr);  // even pixels: bit 32 g + li
            const unsigned long long m1 = __ballot(acc[1][nb][r] >= thr);  // odd pixels
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int row = nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;  // compile-time
                const bool mine = lane == (row & 63);                      // lane <- its row's words (values are wave-uniform)
                w[0][row >> 6] = mine ? (int)(unsigned)(m0 >> (32 * g)) : w[0][row >> 6];
                w[1][row >> 6] = mine ? (int)(unsigned)(m1 >> (32 * g)) : w[1][row >> 6];
            }
            __builtin_amdgcn_sched_barrier(0);  // keep each pair of ballots next to its selects (else 128 masks spill SGPRs)
        }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int h = 0; h < NH; ++h)
            if (h * 64 + lane < NB * 32) wbase[(size_t)t * NPT + h * 64 + lane] = (unsigned)w[t][h];
}

}  // namespace dectile

// the dynamic LDS SMEM, [hi plane][lo plane][bias]: the planes as the locals LDK, H, L, and the pointer to the bias behind them
#define DECTILE_LDS(NB, SMEM, C, LDK, H, L)                 \
    const int LDK = dectile::ldk(C);                        \
    _Float16* H = reinterpret_cast<_Float16*>(SMEM);        \
    _Float16* L = H + (NB) * 32 * LDK;
#define DECTILE_LDS_BIAS(NB, L, LDK) reinterpret_cast<float*>((L) + (NB) * 32 * (LDK))

// tile SLOT of wave WAVE starts at this pixel (as a function the pass-0 kernels came out 17 and 92 instructions longer)
#define DECTILE_TILE_P0(P_BEGIN, WAVE, SLOT) ((P_BEGIN) + ((WAVE) + dectile::WAVES * (SLOT)) * dectile::TILE)

// ---- logits of a whole tile -> rows of ONE tensor [row][P] behind a buffer: 8-byte stores, lanes 0..31 write 256 contiguous bytes of a
// row; ONE per-lane VGPR offset VST, every row / tile offset in the SGPR operand.
// The 64 row offsets row * P * 4 are loop invariants the compiler would keep in 64 SGPRs (-> 230 SGPR spills as v_writelane /
// v_readlane pairs in the tile loop); an opaque copy PQ of P makes it recompute them per store: one s_mul
#define DECTILE_ROW_OFFSETS(VST, PQ, P, G, LI)            \
    const int VST = ((4 * (G)) * (P) + 2 * (LI)) << 2;    \
    int PQ = (P);                                         \
    asm volatile("" : "+s"(PQ));

// rows [0, NB * 32) of the planes GH / GL ([row][C]) -> the LDS planes H / L (LDK halfs per row).  LIVE: an expression in the row index
// `r_`; rows where it is false are never written by the producer and are staged as zero.  Every thread TID of the workgroup takes part.
// FOUR iterations' loads (8 x 16 bytes per thread) are requested before the first LDS store: the rolled load -> store loop was one memory
// round trip per iteration — eight in a row at C = 256, most of the decode's time at one frame per launch.
#define DECTILE_STAGE_PLANES(NB, H, L, LDK, C, GH, GL, TID, LIVE)                                    \
    {                                                                                                \
        const int cpr_ = (C) >> 3;                                                                   \
        const int items_ = (NB) * 32 * cpr_;                                                         \
        for (int i0_ = (TID); i0_ < items_; i0_ += 4 * dectile::THREADS) {                           \
            half8 vh_[4], vl_[4];                                                                    \
            _Pragma("unroll") for (int u_ = 0; u_ < 4; ++u_) {                                       \
                const int i_ = i0_ + u_ * dectile::THREADS;                                          \
                const int r_ = i_ / cpr_, q_ = i_ - r_ * cpr_;                                       \
                vh_[u_] = half8{0, 0, 0, 0, 0, 0, 0, 0};                                             \
                vl_[u_] = half8{0, 0, 0, 0, 0, 0, 0, 0};                                             \
                if (i_ < items_ && (LIVE)) {                                                         \
                    vh_[u_] = *reinterpret_cast<const half8*>((GH) + (size_t)r_ * (C) + q_ * 8);     \
                    vl_[u_] = *reinterpret_cast<const half8*>((GL) + (size_t)r_ * (C) + q_ * 8);     \
                }                                                                                    \
            }                                                                                        \
            _Pragma("unroll") for (int u_ = 0; u_ < 4; ++u_) {                                       \
                const int i_ = i0_ + u_ * dectile::THREADS;                                          \
                if (i_ < items_) {                                                                   \
                    const int r_ = i_ / cpr_, q_ = i_ - r_ * cpr_;                                   \
                    *reinterpret_cast<half8*>((H) + r_ * (LDK) + q_ * 8) = vh_[u_];                  \
                    *reinterpret_cast<half8*>((L) + r_ * (LDK) + q_ * 8) = vl_[u_];                  \
                }                                                                                    \
            }                                                                                        \
        }                                                                                            \
    }

// the wave's sequence of fragments (tile slot x k-step): the cursor of the next load moves on; past the end it stays on the last
// fragment (loads are unconditional: that keeps vmcnt counting exact)
#define DECTILE_ADVANCE_LOAD(LD_KS, LD_SL, LD_CNT, TOTAL, KS)         \
    {                                                                 \
        const bool adv_ = ((LD_CNT) + 1 < (TOTAL));                   \
        const bool wrap_ = ((LD_KS) + 1 == (KS));                     \
        LD_CNT += adv_ ? 1 : 0;                                       \
        LD_SL += (adv_ && wrap_) ? 1 : 0;                             \
        LD_KS = adv_ ? (wrap_ ? 0 : (LD_KS) + 1) : (LD_KS);           \
    }

// the accumulators `f32x16 ACC[2][NB]` start from the bias of their rows, KBS[nb * 32 + vkn_cd_row(r, lane)]
#define DECTILE_BIAS_ACC(ACC, NB, KBS, LANE)                              \
    _Pragma("unroll") for (int nb_ = 0; nb_ < (NB); ++nb_)                \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {               \
            const float kb_ = (KBS)[nb_ * 32 + vkn_cd_row(r_, LANE)];     \
            ACC[0][nb_][r_] = kb_;                                        \
            ACC[1][nb_][r_] = kb_;                                        \
        }

// fp32 fragment REG (8 channels x the lane's pixel pair, `u32x2 REG[8]`) -> half8 f16 hi / lo of the even (BH0, BL0) and the odd pixel.
// NOTE: hipcc (ROCm 7.2) miscompiles `__builtin_bit_cast(T, vec[i])` on an ext_vector ELEMENT (always yields element 0,
// tools/scratch/buftest.hip) — elements are copied to scalars first and converted with __uint_as_float / __float_as_uint.
// A macro: as a forced-inline function (four half8 by reference, or a struct of them returned) k_init_pass<1, 0, 0> came out with
// 6 - 10 more VGPRs, 3 -> 2 waves per SIMD.
#define DECTILE_SPLIT_PAIR(REG, BH0, BL0, BH1, BL1)                                          \
    _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) {                                       \
        _Float16 h_, l_;                                                                     \
        const unsigned u0_ = REG[e_][0], u1_ = REG[e_][1];                                   \
        vkn_split_f16(__uint_as_float(u0_), h_, l_);                                         \
        BH0[e_] = h_;                                                                        \
        BL0[e_] = l_;                                                                        \
        vkn_split_f16(__uint_as_float(u1_), h_, l_);                                         \
        BH1[e_] = h_;                                                                        \
        BL1[e_] = l_;                                                                        \
    }

// n-block rows ROW0 .. ROW0 + 31 of the tile at pixel P0, from the n-block's two accumulators A0 / A1 (times `osc` where OSC).  No per-row
// guard: a buffer that covers exactly the tensor's rows drops the stores of the rows behind them (ragged last n-block) by its range
// check — no exec branches in the loop.  AUX: cache policy.  A macro: as a forced-inline function (accumulators by reference or by
// value) the one-n-block decode kernels came out with 12 - 18 more VGPRs, 6 -> 5 waves per SIMD.
#define DECTILE_STORE_ROWS(A0, A1, RS, VST, PQ, ROW0, P0, AUX, OSC, osc)                                                       \
    _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                                    \
        const int row_ = (ROW0) + (r_ & 3) + 8 * (r_ >> 2); /* this lane's row is row_ + 4 g */                            \
        const float a0_ = (OSC) ? (A0)[r_] * (osc) : (A0)[r_], a1_ = (OSC) ? (A1)[r_] * (osc) : (A1)[r_];                  \
        const dectile::u32x2 v_ = {__float_as_uint(a0_), __float_as_uint(a1_)};                                            \
        __builtin_amdgcn_raw_buffer_store_b64(v_, RS, VST, (row_ * (PQ) + (P0)) << 2, AUX);                                \
    }
