// vkn_instmask.hip — instance masks as bits straight from the head's mask logits (include/vkn_instmask.h): the reference's
// `rescale_masks(...) > mask_thr` (knet/det/kernel_update_head.py:443-466) without any of its K full-resolution fp32 maps.
//
//   p = interp(interp(sigmoid(interp_up(logits[rows[k]])), size = batch_input_shape)[:h, :w], size = ori_shape);   bit = p > thr
//
// One kernel.  A workgroup owns one output tile — a strip of 64 columns x IM_TH rows — of IM_KB masks.  As k_pan_argmax
// (vkn_panoptic.hip) does, it derives the tile's input region of every level from the output back to the logits (the coordinate maps
// are monotone: a region is spanned by the first tap of the first pixel and the second tap of the last), builds the coefficient tables
// of every level ONCE in LDS (pan_coef, vkn_resample.h), and then per mask stages the logits footprint and resamples it level by level
// through LDS (pan_lerp: x then y, v0 * w0 + v1 * w1).  In the last level a wave owns an output row, lane = column: the row's word is
// one 64-lane __ballot(p > thr), stored by lane 0.  Lanes behind Wo vote 0, so the bits behind Wo are zero.  The logits are read once
// per tile (neighbouring tiles share a halo of one or two low-res rows and columns: cache hits), the bits are written once: no atomics
// on the result, no workspace traffic, the same bits on every call.
#include "../../include/vkn_instmask.h"
#include "vkn_common.h"
#include "vkn_resample.h"

namespace {

constexpr int IM_TW = 64, IM_TH = VKN_INSTMASK_TILE_ROWS, IM_KB = VKN_INSTMASK_BATCH, IM_THREADS = 256;
static_assert(IM_TW == VKN_RLE_STRIP_COLS && IM_TH % (IM_THREADS / 64) == 0, "a wave owns whole rows of a strip");

struct ImLevel {
    int in_h, in_w;   // size of the level's input image
    float sy, sx;     // output -> input coordinate scale
};
// Levels: [0] x`up` of the logits (up > 1 only), [1] -> batch_input_shape, [2] crop -> ori_shape.  `first` is 0 or 1: the level that
// reads the logits.  The sigmoid sits in front of level 1: on level 0's output, or on the staged logits when there is no level 0.
struct ImGeom {
    ImLevel lv[3];
    int first;
    int Hm, Wm, Ho, Wo;
    int cap_w[3], cap_h[3];   // LDS capacity of the INPUT region of level l, the replicated border column / row included
};

struct ImRegion {
    int rx0[3], rw[3], ry0[3], rh[3];
};
// input region of every level for one output tile (k_pan_argmax's pan_region, for this file's levels)
__device__ __forceinline__ void im_region(const ImGeom& g, int X0, int tw, int Y0, int th, ImRegion& R) {
    int ox0 = X0, ow = tw, oy0 = Y0, oh = th;
#pragma unroll
    for (int l = 2; l >= 0; --l) {
        if (l < g.first) continue;
        int a0, a1, b0, b1;
        float lam;
        pan_coef(g.lv[l].sx, ox0, g.lv[l].in_w, a0, a1, lam);
        pan_coef(g.lv[l].sx, ox0 + ow - 1, g.lv[l].in_w, b0, b1, lam);
        R.rx0[l] = a0, R.rw[l] = b1 - a0 + 1;
        pan_coef(g.lv[l].sy, oy0, g.lv[l].in_h, a0, a1, lam);
        pan_coef(g.lv[l].sy, oy0 + oh - 1, g.lv[l].in_h, b0, b1, lam);
        R.ry0[l] = a0, R.rh[l] = b1 - a0 + 1;
        ox0 = R.rx0[l], ow = R.rw[l], oy0 = R.ry0[l], oh = R.rh[l];
    }
}

__device__ __forceinline__ float im_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// grid (strips, row tiles, ceil(K / IM_KB)).  LDS (words): per level l >= first the tables x0[nw], lx[nw], y0[nh], ly[nh] of its OUTPUT
// (nw, nh: the capacity of the next level's input, or the tile), then the input buffer of every level.
__global__ __launch_bounds__(IM_THREADS) void k_instmask(const ImGeom g, const float* __restrict__ logits, int N, const int* __restrict__ rows, int K,
                                                         float thr, unsigned long long* __restrict__ bits, unsigned* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const ldsf = reinterpret_cast<float*>(smem);
    int* const ldsi = reinterpret_cast<int*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, X0 = s * IM_TW, Y0 = blockIdx.y * IM_TH;
    const int tw = min(IM_TW, g.Wo - X0), th = min(IM_TH, g.Ho - Y0);
    const int k0 = blockIdx.z * IM_KB, nk = min(IM_KB, K - k0);
    const size_t NS = gridDim.x;

    // ---- carve
    int woff = 0;
    int tx0[3], tlx[3], ty0[3], tly[3], buf[3];     // word offsets
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        if (l < g.first) continue;
        const int nw = l == 2 ? IM_TW : g.cap_w[l + 1], nh = l == 2 ? IM_TH : g.cap_h[l + 1];
        tx0[l] = woff, woff += nw;
        tlx[l] = woff, woff += nw;
        ty0[l] = woff, woff += nh;
        tly[l] = woff, woff += nh;
    }
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        if (l < g.first) continue;
        buf[l] = woff, woff += g.cap_w[l] * g.cap_h[l];
    }

    // ---- regions (registers, every thread) and coefficient tables (LDS, indices local to the level's input region)
    ImRegion R;
    im_region(g, X0, tw, Y0, th, R);
    bool bad = false;
#pragma unroll
    for (int l = 0; l < 3; ++l)
        if (l >= g.first) bad |= R.rw[l] + 1 > g.cap_w[l] || R.rh[l] + 1 > g.cap_h[l] || R.rw[l] < 1 || R.rh[l] < 1;
    if (bad) {      // a capacity defect: reported, never a write outside a buffer (uniform over the workgroup)
        if (tid == 0) atomicOr(status, VKN_INSTMASK_STATUS_FOOTPRINT);
        for (int i = tid; i < nk * th; i += IM_THREADS) bits[((size_t)(k0 + i / th) * NS + s) * (size_t)g.Ho + Y0 + i % th] = 0ull;
        return;
    }
#pragma unroll
    for (int l = 2; l >= 0; --l) {
        if (l < g.first) continue;
        const int ox0 = l == 2 ? X0 : R.rx0[l + 1], oy0 = l == 2 ? Y0 : R.ry0[l + 1];
        const int ow = l == 2 ? tw : R.rw[l + 1], oh = l == 2 ? th : R.rh[l + 1];
        for (int i = tid; i < ow; i += IM_THREADS) {
            int i0, i1;
            float lam;
            pan_coef(g.lv[l].sx, ox0 + i, g.lv[l].in_w, i0, i1, lam);
            ldsi[tx0[l] + i] = i0 - R.rx0[l], ldsf[tlx[l] + i] = lam;
        }
        for (int i = tid; i < oh; i += IM_THREADS) {
            int i0, i1;
            float lam;
            pan_coef(g.lv[l].sy, oy0 + i, g.lv[l].in_h, i0, i1, lam);
            ldsi[ty0[l] + i] = i0 - R.ry0[l], ldsf[tly[l] + i] = lam;
        }
    }

    const int f = g.first;
    const int lw = R.rw[f], lh = R.rh[f], lw1 = lw + 1, litems = lw1 * (lh + 1);
    const size_t plane = (size_t)g.Hm * g.Wm;
    for (int kk = 0; kk < nk; ++kk) {
        const int k = k0 + kk;
        const int row = rows ? rows[k] : k;
        unsigned long long* out = bits + ((size_t)k * NS + s) * (size_t)g.Ho + Y0;
        if (row < 0 || row >= N) {          // (uniform over the workgroup)
            if (tid == 0) atomicOr(status, VKN_INSTMASK_STATUS_ROW_RANGE);
            for (int i = tid; i < th; i += IM_THREADS) out[i] = 0ull;
            continue;
        }
        __syncthreads();        // the tables are written; the previous mask is done with the buffers
        // ---- the logits footprint, with the replicated column / row, -> the first level's input
        {
            const float* src = logits + (size_t)row * plane + (size_t)R.ry0[f] * g.Wm + R.rx0[f];
            for (int i = tid; i < litems; i += IM_THREADS) {
                const int yy = i / lw1, xx = i - yy * lw1;
                const float v = src[(size_t)min(yy, lh - 1) * g.Wm + min(xx, lw - 1)];
                ldsf[buf[f] + yy * g.cap_w[f] + xx] = f == 1 ? im_sigmoid(v) : v;
            }
        }
        __syncthreads();
        // ---- the levels in front of the last: level l's output is level l + 1's input region (with its replicated column / row)
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            if (l < f) continue;
            const int ow = R.rw[l + 1], oh = R.rh[l + 1], ow1 = ow + 1, op = g.cap_w[l + 1], ip = g.cap_w[l];
            for (int i = tid; i < ow1 * (oh + 1); i += IM_THREADS) {
                const int yy = i / ow1, xx = i - yy * ow1;
                const int ys = min(yy, oh - 1), xs = min(xx, ow - 1);
                const float v = pan_lerp(ldsf, buf[l], ip, ldsi[ty0[l] + ys], ldsf[tly[l] + ys], ldsi[tx0[l] + xs], ldsf[tlx[l] + xs]);
                ldsf[buf[l + 1] + yy * op + xx] = l == 0 ? im_sigmoid(v) : v;
            }
            __syncthreads();
        }
        // ---- the last level: a wave per output row, lane = column, the row's word is one ballot
        {
            const bool okx = lane < tw;
            const int xs = okx ? lane : 0;
            const int x0 = ldsi[tx0[2] + xs];
            const float lx = ldsf[tlx[2] + xs];
            for (int y = wave; y < th; y += IM_THREADS / 64) {
                const float p = pan_lerp(ldsf, buf[2], g.cap_w[2], ldsi[ty0[2] + y], ldsf[tly[2] + y], x0, lx);
                const unsigned long long word = __ballot(okx && p > thr);
                if (lane == 0) out[y] = word;
            }
        }
    }
}

// LDS capacity of a level's input region along one axis for `out_extent` output pixels (vkn_panoptic.hip's cap_of)
inline int im_cap_of(int out_extent, float scale, int in_size) {
    long long c = (long long)ceil((double)(out_extent > 0 ? out_extent - 1 : 0) * (double)scale) + 3;
    if (c > in_size) c = in_size;
    return (int)(c < 1 ? 1 : c) + 1;      // + the replicated border column / row
}

inline bool im_cfg_ok(const VknInstMaskCfg* c, int K) {
    if (c->up != 1 && c->up != 2 && c->up != 4) return false;
    if (c->Hm < 1 || c->Wm < 1 || c->Hb < 1 || c->Wb < 1 || c->h < 1 || c->w < 1 || c->Ho < 1 || c->Wo < 1) return false;
    if (c->h > c->Hb || c->w > c->Wb) return false;
    if ((long long)c->Wm * c->up > VKN_INSTMASK_MAX_SCALED_W || (long long)c->Hm * c->up >= (1ll << 24)) return false;
    if (c->Hb >= (1 << 24) || c->Wb >= (1 << 24) || c->Ho >= (1 << 24) || c->Wo >= (1 << 24)) return false;      // pixel indices exact in fp32
    if (K < 1 || K > VKN_INSTMASK_MAX_K) return false;
    const long long words = (long long)K * (((long long)c->Wo + IM_TW - 1) / IM_TW) * c->Ho;
    return words < (1ll << 28) && ((long long)c->Ho + IM_TH - 1) / IM_TH <= 65535;
}

// the geometry and the bytes of LDS of one workgroup; false when a tile's footprint does not fit
inline bool im_geom(const VknInstMaskCfg* c, ImGeom& g, size_t& lds) {
    g = ImGeom{};
    g.Hm = c->Hm, g.Wm = c->Wm, g.Ho = c->Ho, g.Wo = c->Wo;
    g.first = c->up > 1 ? 0 : 1;
    const int Ha = c->Hm * c->up, Wa = c->Wm * c->up;
    // F.interpolate(scale_factor=up): ATen maps coordinates with 1/scale_factor; size= : with in/out (both in fp32): the values that
    // vkn_launch_panoptic_joint derives
    g.lv[0] = ImLevel{c->Hm, c->Wm, (float)(1.0 / (double)c->up), (float)(1.0 / (double)c->up)};
    g.lv[1] = ImLevel{Ha, Wa, (float)Ha / (float)c->Hb, (float)Wa / (float)c->Wb};
    g.lv[2] = ImLevel{c->h, c->w, (float)c->h / (float)c->Ho, (float)c->w / (float)c->Wo};
    int ow = IM_TW, oh = IM_TH;
    size_t words = 0;
    for (int l = 2; l >= g.first; --l) {
        words += (size_t)2 * ow + (size_t)2 * oh;     // the level's tables
        g.cap_w[l] = im_cap_of(ow, g.lv[l].sx, g.lv[l].in_w);
        g.cap_h[l] = im_cap_of(oh, g.lv[l].sy, g.lv[l].in_h);
        ow = g.cap_w[l], oh = g.cap_h[l];
        words += (size_t)ow * oh;
        if (words * 4 > VKN_INSTMASK_LDS_BYTES) return false;
    }
    lds = words * 4;
    return true;
}

}  // namespace

extern "C" {

size_t vkn_sizeof_inst_mask_cfg(void) { return sizeof(VknInstMaskCfg); }
size_t vkn_sizeof_instmask_cfg(void) { return sizeof(VknInstMaskCfg); }

size_t vkn_instance_bits_workspace_bytes(const VknInstMaskCfg* cfg, int K) {
    ImGeom g;
    size_t lds;
    if (!cfg || !im_cfg_ok(cfg, K) || !im_geom(cfg, g, lds)) return 0;
    return VKN_INSTMASK_WS_BYTES;
}

int vkn_instance_bits_f32(const VknInstMaskCfg* cfg, const float* logits, int N, const int* rows, int K, float thr, long long* bits, void* ws,
                          size_t ws_bytes, void* stream) {
    if (!cfg || !logits || !bits || !ws || N < 0 || K < 0) return VKN_E_ARG;
    ImGeom g;
    size_t lds = 0;
    if (!im_cfg_ok(cfg, K) || N < 1 || (!rows && K > N) || (long long)N * cfg->Hm * cfg->Wm >= (1ll << 40) || !im_geom(cfg, g, lds)) return VKN_E_SHAPE;
    if (ws_bytes != VKN_INSTMASK_WS_BYTES) return VKN_E_WORKSPACE;
    if (!vkn_aligned(logits, 16) || !vkn_aligned(bits, 16) || !vkn_aligned(ws, 16) || (rows && !vkn_aligned(rows, 4))) return VKN_E_ALIGN;
    if (!vkn_on_device(logits) || !vkn_on_device(bits) || !vkn_on_device(ws) || (rows && !vkn_on_device(rows))) return VKN_E_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(ws, 0, VKN_INSTMASK_WS_BYTES, st) != hipSuccess) return VKN_E_LAUNCH;
    const dim3 grid((unsigned)((cfg->Wo + IM_TW - 1) / IM_TW), (unsigned)((cfg->Ho + IM_TH - 1) / IM_TH), (unsigned)((K + IM_KB - 1) / IM_KB));
    hipLaunchKernelGGL(k_instmask, grid, dim3(IM_THREADS), lds, st, g, logits, N, rows, K, thr, reinterpret_cast<unsigned long long*>(bits),
                       static_cast<unsigned*>(ws));
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

}  // extern "C"
