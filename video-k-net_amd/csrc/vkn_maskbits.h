// vkn_maskbits.h — masks as bits: the pack pass that the run-length encoder (vkn_rle.hip) and the mask-overlap meter (vkn_maskap.hip)
// share.  K masks [H][W], uint8 (nonzero = set) or fp32 (set iff v > thr), become bits[K][strips][H]: a STRIP is MASKBITS_STRIP_COLS = 64
// columns of one mask, so one row of a strip is one 64-bit word (bit c = column 64 * strip + c; the bits behind W are zero).  The pack
// reads the input ONCE, in aligned 16-byte pieces whatever W is; every later launch reads the words only: 1/8 of the u8 input, 1/32 of
// the fp32 input.  There are no cross-file device symbols in this build, so the kernel is shared as text: every source that includes
// this header compiles its own copy.
#pragma once
#include "vkn_common.h"

namespace {

constexpr int MASKBITS_STRIP_COLS = 64;      // columns of one mask that a workgroup owns: one 64-bit word per row of the strip
constexpr int MASKBITS_THREADS = 256;

template <typename T>
__device__ __forceinline__ bool rle_set(T v, float thr);
template <>
__device__ __forceinline__ bool rle_set<unsigned char>(unsigned char v, float) { return v != 0; }
template <>
__device__ __forceinline__ bool rle_set<float>(float v, float thr) { return v > thr; }

// grid (strips, K).  LPR lanes share a row of the strip: lane j takes the j-th ALIGNED 16-byte piece that the row's 64 elements touch
// (64 / EPC + 1 pieces at most) and keeps the elements that belong to the row; the row's word is the OR over its lanes.  A piece that
// would end behind the tensor is read element by element.
template <typename T, int LPR>
__global__ __launch_bounds__(MASKBITS_THREADS) void k_rle_pack(const T* __restrict__ in, float thr, unsigned long long* __restrict__ bits, int H, int W,
                                                               long long total) {
    constexpr int EPC = 16 / (int)sizeof(T), RPI = MASKBITS_THREADS / LPR;
    static_assert(MASKBITS_STRIP_COLS / EPC + 1 <= LPR && LPR <= 32, "the lanes of a row cover its pieces and stay inside half a wave");
    const int s = blockIdx.x, k = blockIdx.y;
    const int x0 = s * MASKBITS_STRIP_COLS, sw = min(MASKBITS_STRIP_COLS, W - x0);
    const int j = threadIdx.x % LPR, r = threadIdx.x / LPR;
    unsigned long long* out = bits + ((size_t)k * gridDim.x + s) * (size_t)H;
    const long long mbase = (long long)k * H * W + x0;
    for (long long yb = 0; yb < H; yb += RPI) {
        const long long y = yb + r;
        unsigned long long word = 0;
        if (y < H) {
            const long long e0 = mbase + y * W;               // the row's first element in the strip
            const long long c0 = (e0 / EPC + j) * EPC;        // this lane's piece
            if (c0 < e0 + sw) {
                union {
                    uint4 q;
                    T v[EPC];
                } u;
                if (c0 + EPC <= total) {
                    u.q = *reinterpret_cast<const uint4*>(in + c0);
                } else {
#pragma unroll
                    for (int e = 0; e < EPC; ++e) u.v[e] = c0 + e < total ? in[c0 + e] : (T)0;
                }
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const long long col = c0 + e - e0;
                    if (col >= 0 && col < sw && rle_set<T>(u.v[e], thr)) word |= 1ull << col;
                }
            }
        }
#pragma unroll
        for (int d = 1; d < LPR; d <<= 1) word |= __shfl_xor(word, d);
        if (j == 0 && y < H) out[y] = word;
    }
}

// strips of a row of W columns
inline long long maskbits_strips(int W) { return ((long long)W + MASKBITS_STRIP_COLS - 1) / MASKBITS_STRIP_COLS; }

// lanes that share a row of a strip: the pieces of 64 elements, rounded up to a power of two (8 for bytes, 32 for fp32)
template <typename T>
struct MaskbitsLpr;
template <>
struct MaskbitsLpr<unsigned char> {
    static constexpr int value = 8;
};
template <>
struct MaskbitsLpr<float> {
    static constexpr int value = 32;
};

// one launch: `in` [K][H][W] -> bits[K][strips][H].  K >= 1; false when the launch failed.
template <typename T>
inline bool maskbits_pack(const T* in, float thr, int K, int H, int W, unsigned long long* bits, hipStream_t st) {
    hipLaunchKernelGGL((k_rle_pack<T, MaskbitsLpr<T>::value>), dim3((unsigned)maskbits_strips(W), (unsigned)K), dim3(MASKBITS_THREADS), 0, st, in, thr, bits,
                       H, W, (long long)K * H * W);
    return hipGetLastError() == hipSuccess;
}

}  // namespace
