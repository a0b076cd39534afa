// vkn_wimage.hip — the ONE writer of the split weight tile images (layout, split and addressing: vkn_wimage.h): fp32 matrices -> the
// three-plane bf16 images that k_gemm_s3 / k_ffn_fused (vkn_update.hip), k_gemm_t3 / k_chain_* (vkn_chain.hip) and k_gemm_ks
// (vkn_ksplit.hip) stream, or the two-plane fp16 images of W times a power of two that the fp16 form of the persistent chain streams
// (vkn_chain_h2.hip).  One table-driven kernel: the images of MANY matrices in one launch (training rebuilds both orientations of every
// Linear weight of a stage every step, chain_train.py); a single matrix is a table of one item.
#include <hip/hip_runtime.h>

#include "../../include/vkn.h"
#include "vkn_common.h"
#include "vkn_launch.h"
#include "vkn_wimage.h"

namespace {

// item i stands for the matrix Wm [nout][k]: element (n, kk) is W[n * ldn + kk * ldk] (* scale[i][0], a DEVICE scalar, in the SCALED form)
// for kk < kvalid and 0 for kvalid <= kk < k; its tiles are workgroups tile0[i] .. tile0[i + 1] - 1
template <bool SCALED>   // (the scale pointers travel only with the scaled form: 512 bytes of kernel arguments)
struct SplitTab {
    const float* W[VKN_SPLIT_MAX_ITEMS];
    void* dst[VKN_SPLIT_MAX_ITEMS];
    long long ldn[VKN_SPLIT_MAX_ITEMS], ldk[VKN_SPLIT_MAX_ITEMS];
    int nout[VKN_SPLIT_MAX_ITEMS], k[VKN_SPLIT_MAX_ITEMS], kvalid[VKN_SPLIT_MAX_ITEMS];
    int tile0[VKN_SPLIT_MAX_ITEMS + 1];
    const float* scale[SCALED ? VKN_SPLIT_MAX_ITEMS : 1];
};

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

// A workgroup writes one tile: thread = row, its 32 k values -> NPL x four 16-byte stores, consecutive threads consecutive 16 bytes.
// Rows >= nout and k >= kvalid are written as zeros in every plane.
template <int NPL, typename E, bool SCALED>
__global__ __launch_bounds__(256) void k_split_tiles(const SplitTab<SCALED> T, int nitems) {
    const int b = blockIdx.x;
    int it = 0;
    while (it + 1 < nitems && b >= T.tile0[it + 1]) ++it;   // block-uniform
    const int tl = b - T.tile0[it];
    const int K = T.k[it], Nout = T.nout[it], kvalid = T.kvalid[it];
    const int ktiles = K >> 5;
    const int nt = tl / ktiles, kt = tl - nt * ktiles;
    const float* __restrict__ W = T.W[it];
    const long long ldn = T.ldn[it], ldk = T.ldk[it];
    const int row = threadIdx.x, n = nt * wimg::COLS + row;
    float v[32];
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) v[kk] = 0.f;
    if (n < Nout) {
        if (ldk == 1 && kt * 32 + 32 <= kvalid && (ldn & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0) {
            const f32x4* src = reinterpret_cast<const f32x4*>(W + (size_t)n * ldn + kt * 32);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x4 t = src[j];
                v[4 * j] = t[0]; v[4 * j + 1] = t[1]; v[4 * j + 2] = t[2]; v[4 * j + 3] = t[3];
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) {
                const int k = kt * 32 + kk;
                v[kk] = k < kvalid ? W[(size_t)n * ldn + (size_t)k * ldk] : 0.f;
            }
        }
        if (SCALED) {
            const float sc = T.scale[it][0];
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) v[kk] *= sc;
        }
    }
    u16x8* dst = reinterpret_cast<u16x8*>(static_cast<E*>(T.dst[it]) + ((size_t)nt * ktiles + kt) * wimg::tile_elems(NPL));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        u16x8 o[NPL];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            E t[NPL];
            wimg::split(v[8 * q + e], t);
#pragma unroll
            for (int p = 0; p < NPL; ++p) o[p][e] = __builtin_bit_cast(unsigned short, t[p]);
        }
#pragma unroll
        for (int p = 0; p < NPL; ++p) dst[wimg::elem(p, 8 * q, row) >> 3] = o[p];
    }
}

// the launch: `scales` NULL (SCALED false) or one DEVICE scalar per item.  The callers have checked the items.
template <int NPL, typename E, bool SCALED>
int split_tiles(const VknSplitItem* items, const float* const* scales, int nitems, hipStream_t stream) {
    SplitTab<SCALED> T;
    int tiles = 0;
    for (int i = 0; i < nitems; ++i) {
        const VknSplitItem& it = items[i];
        T.W[i] = it.W; T.dst[i] = it.images;
        if (SCALED) T.scale[i] = scales[i];
        T.ldn[i] = it.ldn; T.ldk[i] = it.ldk;
        T.nout[i] = it.Nout; T.k[i] = it.K; T.kvalid[i] = it.kvalid;
        T.tile0[i] = tiles;
        tiles += ((it.Nout + wimg::COLS - 1) / wimg::COLS) * (it.K / wimg::KT);
    }
    T.tile0[nitems] = tiles;
    hipLaunchKernelGGL((k_split_tiles<NPL, E, SCALED>), dim3(tiles), dim3(256), 0, stream, T, nitems);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// bytes of the tile images of a [Nout][K] weight
size_t vkn_split_w3_bytes(int Nout, int K) { return wimg::image_bytes(3, Nout, K); }
size_t vkn_split_h2_bytes(int Nout, int K) { return wimg::image_bytes(2, Nout, K); }

// fp32 W [Nout][K] -> bf16x3 tile images (K % 32 == 0, images 16-byte aligned)
int vkn_launch_split_w3(const float* W, void* Wp, int Nout, int K, hipStream_t stream) {
    if (Nout <= 0 || K <= 0 || K % 32 != 0) return VKN_E_SHAPE;
    if (!aligned16(Wp)) return VKN_E_ALIGN;
    const VknSplitItem it{W, Wp, K, 1, Nout, K, K, 0};
    return split_tiles<3, __bf16, false>(&it, nullptr, 1, stream);
}

// ... of the TRANSPOSE of a stored matrix: Wt [Nout][K] with Wt[n][k] = W[k * Nout + n] (W is [K][Nout] row-major)
int vkn_launch_split_w3_t(const float* W, void* Wp, int Nout, int K, hipStream_t stream) {
    if (Nout <= 0 || K <= 0 || K % 32 != 0) return VKN_E_SHAPE;
    if (!aligned16(Wp)) return VKN_E_ALIGN;
    const VknSplitItem it{W, Wp, 1, Nout, Nout, K, K, 0};
    return split_tiles<3, __bf16, false>(&it, nullptr, 1, stream);
}

// fp32 W [Nout][K] -> fp16 hi / lo tile images of W * *scale.  scale: DEVICE scalar, a power of two (vkn_pow2_scale_f32 of the matrix:
// its maximum at 2^9 .. 2^10, so that the low half of every weight down to 2^-12 of the maximum keeps its eleven bits)
int vkn_launch_split_h2(const float* W, void* images, int Nout, int K, const float* scale, hipStream_t stream) {
    if (!W || !images || !scale || Nout <= 0 || K <= 0 || K % 32 != 0) return VKN_E_ARG;
    if (!aligned16(images)) return VKN_E_ALIGN;
    const VknSplitItem it{W, images, K, 1, Nout, K, K, 0};
    return split_tiles<2, _Float16, true>(&it, &scale, 1, stream);
}

extern "C" {

int vkn_split_weights_batch_f32(const VknSplitItem* items, int nitems, void* stream) {
    if (!items || nitems <= 0 || nitems > VKN_SPLIT_MAX_ITEMS) return VKN_E_ARG;
    for (int i = 0; i < nitems; ++i) {
        const VknSplitItem& it = items[i];
        if (!it.W || !it.images || it.Nout <= 0 || it.K <= 0 || it.kvalid < 0 || it.kvalid > it.K) return VKN_E_ARG;
        if (it.K % 32 != 0 || !aligned16(it.images)) return VKN_E_SHAPE;
    }
    return split_tiles<3, __bf16, false>(items, nullptr, nitems, static_cast<hipStream_t>(stream));
}

size_t vkn_sizeof_split_item(void) { return sizeof(VknSplitItem); }

}  // extern "C"
