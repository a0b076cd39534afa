// vkn_wimage.h — the split weight tile image, once: the layout every GEMM of the kernel-update chain streams, the split that fills it,
// the reader's fragment address and the product group.  Include after vkn_common.h.  Constants, device functions, one host helper; the
// writer kernel is vkn_wimage.hip.
//
//   * the image of a matrix W [Nout][K] (K % 32 == 0) is [ceil(Nout/256)][K/32] TILES, k-tile minor; a tile is COLS = 256 rows of W
//     ("columns" of the GEMM's output) x KT = 32 k as [plane NPL][q 4][row 256][8]: element (plane, k, row) at
//     ((plane * 4 + (k >> 3)) * 256 + row) * 8 + (k & 7).  Rows >= Nout are zeros in every plane.  Three bf16 planes (49152 bytes) or
//     two fp16 planes (32768 bytes, of W times a power of two);
//   * the planes are the terms of `split`: v = p[0] + p[1] (+ p[2]), each the rounding of what the earlier ones left;
//   * this IS the MFMA fragment layout: the 8 k of (k-step ks, lane half g) of a 32-wide column block are one 16-byte slot, consecutive
//     rows consecutive slots.  A reader's fragment of plane 0 sits at `WIMG_FRAG_ELEM` (elements; LDS copies of a tile) or at `WIMG_FRAG_LANE_BYTES`
//     + `frag_step_bytes` (bytes; the two halves of a buffer load's address); plane p is `PLANE` elements / `frag_step_bytes(p, .)` on;
//   * `mfma6` / `mfma3` are the significant cross products of two split operands, smallest terms first.  That order is part of the
//     results.
//
// The pieces are constexpr or forced-inline functions, but for the reader's element address and the lane part of its byte address, which
// are macros (names global, WIMG_ in front): in these forms every release
// kernel that reads images compiles to the instruction stream it had with these lines written out in it (profiles/wimage_resources.txt).
#pragma once

namespace wimg {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int COLS = 256;                 // rows of W per tile
constexpr int KT = 32;                    // k per tile: four groups of 8
constexpr int PLANE = 4 * COLS * 8;       // elements of one plane of a tile
constexpr unsigned SLOTS = COLS * 16u;    // bytes of one k group of one plane: 256 fragment slots of 16 bytes
__host__ __device__ constexpr int tile_elems(int npl) { return npl * PLANE; }
__host__ __device__ constexpr unsigned tile_bytes(int npl) { return (unsigned)tile_elems(npl) * 2u; }   // bf16 and fp16: 2 bytes
// bytes of the images of an [Nout][K] matrix
inline size_t image_bytes(int npl, int Nout, int K) { return (size_t)((Nout + COLS - 1) / COLS) * (size_t)(K / KT) * tile_bytes(npl); }

// writers: element (plane, k, row) of a tile
__host__ __device__ constexpr int elem(int plane, int k, int row) { return ((plane * 4 + (k >> 3)) * COLS + row) * 8 + (k & 7); }
// readers, element form: plane 0 of (k-step ks, lane half g, column col0 + li of the tile).  A macro, and the two column terms summed
// in this order: as a function of one column, k_gemm_s3 came out with another operand order; as a function of two, k_ffn_fused with
// another prologue (profiles/wimage_resources.txt)
#define WIMG_FRAG_ELEM(ks, g, col0, li) (((((ks) << 1) + (g)) * wimg::COLS + (col0) + (li)) * 8)
// readers, byte form: the lane part and the (plane p, k-step ks) part.  The lane part is a macro: as a function, all but one k_gemm_ks
// came out with other register numbers and another instruction order around the address
#define WIMG_FRAG_LANE_BYTES(g, col) ((unsigned)((g) * 4096 + (col) * 16))
__host__ __device__ constexpr unsigned frag_step_bytes(int p, int ks) { return (unsigned)((p * 4 + 2 * ks) * 4096); }
static_assert(SLOTS == 4096u && WIMG_FRAG_ELEM(1, 1, 224, 31) == elem(0, 24, 255) && WIMG_FRAG_LANE_BYTES(1, 3) + frag_step_bytes(2, 1) == 2u * elem(2, 24, 3),
              "the reader's fragment addresses are the writer's elements");

// v = p[0] + p[1] (+ p[2]): each term the rounding of what the earlier ones left.  E = __bf16 x 3 (2^-24 relative) or _Float16 x 2
template <int NPL, typename E>
__device__ __forceinline__ void split(float v, E (&p)[NPL]) {
    float r = v;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
        p[i] = (E)r;
        if (i + 1 < NPL) r -= (float)p[i];
    }
}
__device__ __forceinline__ void split3(float v, __bf16& h, __bf16& m, __bf16& l) {
    __bf16 t[3];
    split(v, t);
    h = t[0], m = t[1], l = t[2];
}

// acc += the six significant products of (activation ah + am + al) x (weight wh + wm + wl), as (activation, weight) terms
// (h,l) (l,h) (m,m) (h,m) (m,h) (h,h): smallest first; the dropped ones are <= 2^-24 relative.  W_FIRST: the weight fragment is the
// first MFMA operand (D^T = W . A^T, a lane owns an activation row) instead of the second.
template <bool W_FIRST>
__device__ __forceinline__ void mfma6(f32x16& acc, bf16x8 ah, bf16x8 am, bf16x8 al, bf16x8 wh, bf16x8 wm, bf16x8 wl) {
#define WIMG_MFMA_(A, W) acc = W_FIRST ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(W, A, acc, 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, W, acc, 0, 0, 0)
    WIMG_MFMA_(ah, wl);
    WIMG_MFMA_(al, wh);
    WIMG_MFMA_(am, wm);
    WIMG_MFMA_(ah, wm);
    WIMG_MFMA_(am, wh);
    WIMG_MFMA_(ah, wh);
#undef WIMG_MFMA_
}
// ... and the three of the two-term fp16 split: (h,l) (l,h) (h,h); lo x lo is below fp32 resolution
template <bool W_FIRST>
__device__ __forceinline__ void mfma3(f32x16& acc, f16x8 ah, f16x8 al, f16x8 wh, f16x8 wl) {
#define WIMG_MFMA_(A, W) acc = W_FIRST ? __builtin_amdgcn_mfma_f32_32x32x16_f16(W, A, acc, 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x16_f16(A, W, acc, 0, 0, 0)
    WIMG_MFMA_(ah, wl);
    WIMG_MFMA_(al, wh);
    WIMG_MFMA_(ah, wh);
#undef WIMG_MFMA_
}

}  // namespace wimg
