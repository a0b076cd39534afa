// vkn_swin_bwd.hip — the backward of the (shifted-)window attention core of the Swin backbone (include/vkn_wattn_train.h) for gfx950.
//
// Ownership is the forward's (vkn_swin.hip): a WAVE owns one head of one window of the rolled map, a lane owns a token.  Here a
// workgroup is that one wave, so the only limit on the waves of a CU is what one wave takes.  Nothing is saved by the forward: the wave
// recomputes scores, maximum and softmax from `qkv` with the forward's expressions, in two passes over ONE pair of LDS row images
// (window^2 x 32 floats each):
//   * query-owner pass: the images hold K and V.  Lane i holds q_i scale and dout_i, recomputes its score row in registers exactly as
//     the forward does, keeps p_ij and dP_ij = dout_i . v_j, forms max_i, 1 / sum_i and delta_i = sum_j P_ij dP_ij (in fp64), accumulates
//     dq_i = scale sum_j dS_ij k_j, writes it, and parks the three scalars in LDS;
//   * every lane takes ITS token's k and v rows out of the images into registers, and the images are overwritten with q scale and dout;
//   * key-owner pass: lane j holds k_j, v_j, dk_j, dv_j and walks the queries in order; q_i scale and dout_i are LDS broadcasts.  It
//     recomputes s_ij, P_ij, dP_ij and dS_ij with the same expressions (the same bits as the query owner's), accumulates dk_j and dv_j,
//     and adds dS_ij into the wave's image of the table column in LDS: for a fixed query rel(i, j) is injective in j, so the lanes of one
//     step hit distinct words, and the steps of one wave reach the LDS in order.
// Real keys write their rows of `dqkv`; pad keys hand dk, dv to lanes 0..63, which add them in token order into the wave's pad partial.
// The table image and the pad partial go to the workspace; k_wattn_bwd_merge adds the partials of all windows in fp64 in a fixed order.
// No float atomics anywhere.
//
// Safety: every global address is formed from a token position that was reduced modulo the padded extent and compared with H, W first;
// pad positions form no address into qkv / dout / dqkv.  No input VALUE reaches an address.
//
// The geometry struct, the region rule and the score expression are a COPY of vkn_swin.hip's, not a shared header: moving them requires
// the forward's outputs hashed on the device at the parent and at the head and its register count compared, and that comparison has
// not been made.  tests/test_gpu_swin_bwd.py holds the two copies together through the float64 restatement.
#include "../../include/vkn_wattn_train.h"
#include "vkn_common.h"

namespace {

constexpr int WB_D = VKN_SWIN_HEAD_DIM;
constexpr int WB_PART = VKN_WATTN_PART_FLOATS;
constexpr int WB_SLICES = VKN_WATTN_MERGE_SLICES;
static_assert(WB_PART == 2 * WB_D, "a pad partial is dk | dv of one head");

struct WattnGeom {
    int H, W, Hp, Wp, nWw, nWin, heads, shift;      // nWin: windows of one image
};

// r(s, E) of vkn_swin.h: the slice of the rolled axis that position s falls in
__device__ __forceinline__ int wb_region(int s, int E, int ws, int shift) { return s < E - ws ? 0 : (s < E - shift ? 1 : 2); }

// the forward's dot product: products in f32x4 lanes, chained over the 8 quads, then (x + y) + (z + w).  Products commute, so the
// query owner (a in registers, b in LDS) and the key owner (a in LDS, b in registers) get the same bits.
__device__ __forceinline__ float wb_dot(const f32x4* a, const f32x4* b) {
    f32x4 a4 = a[0] * b[0];
#pragma unroll
    for (int c = 1; c < WB_D / 4; ++c) a4 = a[c] * b[c] + a4;
    return (a4.x + a4.y) + (a4.z + a4.w);
}

// the steps of ONE wave on its LDS image: nothing of the compiler's moves across, and the hardware keeps a wave's LDS operations in order
__device__ __forceinline__ void wb_wave_step() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int WS>
__global__ __launch_bounds__(64) void k_wattn_bwd(const float* __restrict__ qkv, const float* __restrict__ qkv_bias,
                                                   const float* __restrict__ table, const float* __restrict__ dout, float* __restrict__ dqkv,
                                                   float* __restrict__ tab_part, float* __restrict__ pad_part, WattnGeom g, float scale) {
    constexpr int N = WS * WS, R = 2 * WS - 1, T = R * R, D = WB_D;
    __shared__ f32x4 imgA4[N * D / 4], imgB4[N * D / 4];       // K then q scale;  V then dout
    __shared__ float tab[T], dtab[T], st_mx[64], st_inv[64], st_delta[64];
    float* imgA = reinterpret_cast<float*>(imgA4);
    float* imgB = reinterpret_cast<float*>(imgB4);
    const int lane = (int)threadIdx.x, head = (int)blockIdx.y;
    const int b = (int)blockIdx.x / g.nWin, wi = (int)blockIdx.x % g.nWin, wy0 = (wi / g.nWw) * WS, wx0 = (wi % g.nWw) * WS;
    const size_t HD = (size_t)g.heads * D;
    for (int idx = lane; idx < N * (D / 4); idx += 64) {
        const int t = idx / (D / 4), c = (idx % (D / 4)) * 4;
        int py = wy0 + t / WS + g.shift, px = wx0 + t % WS + g.shift;          // the padded-map token that the roll put here
        py -= py >= g.Hp ? g.Hp : 0;
        px -= px >= g.Wp ? g.Wp : 0;
        f32x4 k = {0.f, 0.f, 0.f, 0.f}, v = k;
        if (py < g.H && px < g.W) {
            const float* p = qkv + (((size_t)b * g.H + py) * g.W + px) * (3 * HD) + (size_t)head * D + c;
            k = *reinterpret_cast<const f32x4*>(p + HD);
            v = *reinterpret_cast<const f32x4*>(p + 2 * HD);
        } else if (qkv_bias) {                                                  // a pad token: qkv(0) = the bias
            k = *reinterpret_cast<const f32x4*>(qkv_bias + HD + (size_t)head * D + c);
            v = *reinterpret_cast<const f32x4*>(qkv_bias + 2 * HD + (size_t)head * D + c);
        }
        *reinterpret_cast<f32x4*>(imgA + t * D + c) = k;
        *reinterpret_cast<f32x4*>(imgB + t * D + c) = v;
    }
    for (int i = lane; i < T; i += 64) {
        tab[i] = table[(size_t)i * g.heads + head];
        dtab[i] = 0.f;
    }
    __syncthreads();

    // ---- this lane's token
    const bool in_window = lane < N;
    const int ty = lane / WS, tx = lane % WS;
    int py = wy0 + ty + g.shift, px = wx0 + tx + g.shift;
    py -= py >= g.Hp ? g.Hp : 0;
    px -= px >= g.Wp ? g.Wp : 0;
    const bool real = in_window && py < g.H && px < g.W;
    const size_t tok = real ? ((size_t)b * g.H + py) * g.W + px : 0;          // (a pad token forms no address: `tok` is read under `real` only)
    const bool masked = g.shift > 0;
    const int reg_own = 3 * wb_region(wy0 + ty, g.Hp, WS, g.shift) + wb_region(wx0 + tx, g.Wp, WS, g.shift);

    f32x4 dO[D / 4];
#pragma unroll
    for (int c = 0; c < D / 4; ++c) dO[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // ---- query-owner pass (a pad query's output is cropped away: dout = 0, nothing to add)
    if (real) {
        f32x4 q[D / 4];
#pragma unroll
        for (int c = 0; c < D / 4; ++c) {
            q[c] = *reinterpret_cast<const f32x4*>(qkv + tok * (3 * HD) + (size_t)head * D + 4 * c) * scale;
            dO[c] = *reinterpret_cast<const f32x4*>(dout + tok * HD + (size_t)head * D + 4 * c);
        }
        const float* tq = tab + (ty + WS - 1) * R + (tx + WS - 1);              // tq[-(y_j R + x_j)] = table[rel(i, j)]
        float s[N], dP[N];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            float a = wb_dot(q, reinterpret_cast<const f32x4*>(imgA + j * D));
            a += tq[-((j / WS) * R + (j % WS))];
            const int rk = 3 * wb_region(wy0 + j / WS, g.Hp, WS, g.shift) + wb_region(wx0 + j % WS, g.Wp, WS, g.shift);
            a += (masked && rk != reg_own) ? (float)VKN_SWIN_MASK : 0.f;
            s[j] = a;
            mx = fmaxf(mx, a);
        }
        float den = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            s[j] = expf(s[j] - mx);
            den += s[j];
        }
        const float inv = 1.f / den;
        // delta_i = (sum_j p_ij dP_ij) / (sum_j p_ij), both sums in fp64 in key order, rounded once: keys that share v (the pad keys: their
        // v is the bias) then get dP_ij - delta_i = 0 exactly, as the softmax's Jacobian demands, however the weight is spread among them.
        // Accumulated in fp32, delta is off by a few ulps of dP, and every such key's dk takes that error times P_ij times q_i.
        double num = 0.0, norm = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            dP[j] = wb_dot(dO, reinterpret_cast<const f32x4*>(imgB + j * D));
            num = (double)s[j] * (double)dP[j] + num;
            norm += (double)s[j];
        }
        const float delta = (float)(num / norm);
        f32x4 dq[D / 4];
#pragma unroll
        for (int c = 0; c < D / 4; ++c) dq[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        // K is read a second time: without this line the compiler keeps the first reading of all N rows alive in registers (and spills them)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float dS = (s[j] * inv) * (dP[j] - delta);
            const f32x4* kj = reinterpret_cast<const f32x4*>(imgA + j * D);
#pragma unroll
            for (int c = 0; c < D / 4; ++c) dq[c] = dS * kj[c] + dq[c];
        }
        float* o = dqkv + tok * (3 * HD) + (size_t)head * D;
#pragma unroll
        for (int c = 0; c < D / 4; ++c) *reinterpret_cast<f32x4*>(o + 4 * c) = dq[c] * scale;
        st_mx[lane] = mx;
        st_inv[lane] = inv;
        st_delta[lane] = delta;
    }

    // ---- the images change hands: every lane takes its own k, v rows; then q scale and dout take their place
    f32x4 k[D / 4], v[D / 4], dk[D / 4], dv[D / 4];
#pragma unroll
    for (int c = 0; c < D / 4; ++c) {
        k[c] = in_window ? imgA4[lane * (D / 4) + c] : f32x4{0.f, 0.f, 0.f, 0.f};
        v[c] = in_window ? imgB4[lane * (D / 4) + c] : f32x4{0.f, 0.f, 0.f, 0.f};
        dk[c] = dv[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    if (in_window) {
#pragma unroll
        for (int c = 0; c < D / 4; ++c) {
            f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
            if (real) q4 = *reinterpret_cast<const f32x4*>(qkv + tok * (3 * HD) + (size_t)head * D + 4 * c) * scale;
            imgA4[lane * (D / 4) + c] = q4;
            imgB4[lane * (D / 4) + c] = dO[c];
        }
    }
    __syncthreads();

    // ---- key-owner pass
    if (in_window) {
        const int rel_own = (WS - 1 - ty) * R + (WS - 1 - tx);                  // rel(i, j) = y_i R + x_i + rel_own
#pragma unroll 1
        for (int i = 0; i < N; ++i) {
            const int iy = i / WS, ix = i % WS;
            int qy = wy0 + iy + g.shift, qx = wx0 + ix + g.shift;
            qy -= qy >= g.Hp ? g.Hp : 0;
            qx -= qx >= g.Wp ? g.Wp : 0;
            if (qy >= g.H || qx >= g.W) continue;                                // a pad query (uniform over the wave)
            const f32x4* qi = imgA4 + i * (D / 4);
            const f32x4* di = imgB4 + i * (D / 4);
            const int rel = iy * R + ix + rel_own;
            float a = wb_dot(qi, k);
            a += tab[rel];
            const int rq = 3 * wb_region(wy0 + iy, g.Hp, WS, g.shift) + wb_region(wx0 + ix, g.Wp, WS, g.shift);
            a += (masked && reg_own != rq) ? (float)VKN_SWIN_MASK : 0.f;
            const float inv = st_inv[i];
            const float p = expf(a - st_mx[i]);
            const float dPij = wb_dot(di, v);
            const float P = p * inv;
            const float dS = P * (dPij - st_delta[i]);
#pragma unroll
            for (int c = 0; c < D / 4; ++c) {
                dv[c] = P * di[c] + dv[c];
                dk[c] = dS * qi[c] + dk[c];
            }
            dtab[rel] += dS;
            wb_wave_step();
        }
    }
    __syncthreads();                                                             // every read of the images is done

    // ---- out: a real key's rows of dqkv; a pad key's dk | dv into the images, for the pad partial
    if (real) {
        float* o = dqkv + tok * (3 * HD) + (size_t)head * D;
#pragma unroll
        for (int c = 0; c < D / 4; ++c) {
            *reinterpret_cast<f32x4*>(o + HD + 4 * c) = dk[c];
            *reinterpret_cast<f32x4*>(o + 2 * HD + 4 * c) = dv[c];
        }
    } else if (in_window) {
#pragma unroll
        for (int c = 0; c < D / 4; ++c) {
            imgA4[lane * (D / 4) + c] = dk[c];
            imgB4[lane * (D / 4) + c] = dv[c];
        }
    }
    __syncthreads();
    const size_t wave_id = (size_t)blockIdx.x * g.heads + head;
    for (int i = lane; i < T; i += 64) tab_part[wave_id * T + i] = dtab[i];
    if (pad_part) {
        const float* img = lane < D ? imgA : imgB;
        const int c = lane & (D - 1);
        float sum = 0.f;
        for (int t = 0; t < N; ++t) {                                            // the pad keys of the window, in token order
            int ky = wy0 + t / WS + g.shift, kx = wx0 + t % WS + g.shift;
            ky -= ky >= g.Hp ? g.Hp : 0;
            kx -= kx >= g.Wp ? g.Wp : 0;
            if (ky >= g.H || kx >= g.W) sum += img[t * D + c];
        }
        pad_part[wave_id * WB_PART + lane] = sum;
    }
}

// One thread block per 64 outputs: thread (slice, e) adds the partials of the windows w = slice, slice + SLICES, ... of output e in fp64,
// then thread (0, e) adds the slices in order.  Outputs: heads T table words, then heads 64 pad-bias words, then the heads 32 zeros of
// the bias gradient's q third (the last two only with a bias).
__global__ __launch_bounds__(64 * WB_SLICES) void k_wattn_bwd_merge(const float* __restrict__ tab_part, const float* __restrict__ pad_part,
                                                                   float* __restrict__ dtable, float* __restrict__ dbias, int n_wave_sets,
                                                                   int heads, int T) {
    __shared__ double part[WB_SLICES][64];
    const int lane = (int)threadIdx.x & 63, slice = (int)threadIdx.x >> 6;
    const int n_tab = heads * T, n_pad = dbias ? heads * WB_PART : 0, n_zero = dbias ? heads * WB_D : 0;
    const int e = (int)blockIdx.x * 64 + lane;
    double sum = 0.0;
    if (e < n_tab) {
        for (int w = slice; w < n_wave_sets; w += WB_SLICES) sum += (double)tab_part[(size_t)w * n_tab + e];
    } else if (e < n_tab + n_pad) {
        for (int w = slice; w < n_wave_sets; w += WB_SLICES) sum += (double)pad_part[(size_t)w * n_pad + (e - n_tab)];
    }
    part[slice][lane] = sum;
    __syncthreads();
    if (slice != 0 || e >= n_tab + n_pad + n_zero) return;
    double total = part[0][lane];
#pragma unroll
    for (int s = 1; s < WB_SLICES; ++s) total += part[s][lane];
    if (e < n_tab) {
        dtable[(size_t)(e % T) * heads + e / T] = (float)total;                 // partials [head][rel] -> dbias_table [rel][head]
    } else if (e < n_tab + n_pad) {
        const int f = e - n_tab, head = f / WB_PART, third = 1 + (f % WB_PART) / WB_D, c = f % WB_D;
        dbias[((size_t)third * heads + head) * WB_D + c] = (float)total;
    } else {
        dbias[e - n_tab - n_pad] = 0.f;                                          // the q third: a pad query has no gradient
    }
}

// the windows of B images, or 0 when their count leaves int
long long wb_windows(int B, int H, int W, int window) {
    const long long nWh = ((long long)H + window - 1) / window, nWw = ((long long)W + window - 1) / window;
    return (long long)B * nWh * nWw;
}

long long wb_tab_bytes(long long windows, int heads, int window) {
    const long long T = (2ll * window - 1) * (2ll * window - 1);
    const long long raw = windows * heads * T * (long long)sizeof(float);
    return (raw + VKN_WATTN_WS_ALIGN - 1) / VKN_WATTN_WS_ALIGN * VKN_WATTN_WS_ALIGN;
}

long long wb_workspace(int B, int H, int W, int heads, int window) {
    const long long windows = wb_windows(B, H, W, window);
    return wb_tab_bytes(windows, heads, window) + windows * heads * WB_PART * (long long)sizeof(float);
}

}  // namespace

extern "C" int vkn_wattn_bwd_supported(int B, int H, int W, int heads, int window, int shift) {
    if (!vkn_swin_window_attn_supported(B, H, W, heads, window, shift)) return 0;
    return wb_workspace(B, H, W, heads, window) < (1ll << 31);
}

extern "C" size_t vkn_wattn_bwd_workspace_bytes(int B, int H, int W, int heads, int window) {
    if (!vkn_wattn_bwd_supported(B, H, W, heads, window, 0)) return 0;
    return (size_t)wb_workspace(B, H, W, heads, window);
}

extern "C" int vkn_wattn_bwd_f32(const float* qkv, const float* qkv_bias, const float* bias_table, const float* dout, float* dqkv,
                                 float* dqkv_bias, float* dbias_table, int B, int H, int W, int heads, int window, int shift, float scale,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!qkv || !bias_table || !dout || !dqkv || !dbias_table || B <= 0 || H <= 0 || W <= 0 || heads <= 0) return VKN_E_ARG;
    if ((qkv_bias == nullptr) != (dqkv_bias == nullptr)) return VKN_E_ARG;
    if (!vkn_wattn_bwd_supported(B, H, W, heads, window, shift)) return VKN_E_SHAPE;
    const size_t need = vkn_wattn_bwd_workspace_bytes(B, H, W, heads, window);
    if (!workspace || workspace_bytes < need) return VKN_E_WORKSPACE;
    if (!vkn_aligned(qkv, 16) || !vkn_aligned(qkv_bias, 16) || !vkn_aligned(bias_table, 16) || !vkn_aligned(dout, 16) || !vkn_aligned(dqkv, 16) ||
        !vkn_aligned(dqkv_bias, 16) || !vkn_aligned(dbias_table, 16) || !vkn_aligned(workspace, 16))
        return VKN_E_ALIGN;
    WattnGeom g;
    g.H = H, g.W = W, g.heads = heads, g.shift = shift;
    const int nWh = (H + window - 1) / window;
    g.nWw = (W + window - 1) / window;
    g.Hp = nWh * window, g.Wp = g.nWw * window, g.nWin = nWh * g.nWw;
    const long long windows = wb_windows(B, H, W, window);
    float* tab_part = static_cast<float*>(workspace);
    float* pad_part = qkv_bias ? reinterpret_cast<float*>(static_cast<char*>(workspace) + wb_tab_bytes(windows, heads, window)) : nullptr;
    const dim3 grid((unsigned)windows, (unsigned)heads), block(64);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define WATTN_LAUNCH(WS)                                                                                                                \
    case WS:                                                                                                                            \
        hipLaunchKernelGGL((k_wattn_bwd<WS>), grid, block, 0, st, qkv, qkv_bias, bias_table, dout, dqkv, tab_part, pad_part, g, scale); \
        break
    switch (window) {
        WATTN_LAUNCH(1);
        WATTN_LAUNCH(2);
        WATTN_LAUNCH(3);
        WATTN_LAUNCH(4);
        WATTN_LAUNCH(5);
        WATTN_LAUNCH(6);
        WATTN_LAUNCH(7);
        WATTN_LAUNCH(8);
    }
#undef WATTN_LAUNCH
    VKN_CHECK_LAUNCH();
    const int T = (2 * window - 1) * (2 * window - 1);
    const int outputs = heads * T + (qkv_bias ? heads * (WB_PART + WB_D) : 0);
    hipLaunchKernelGGL(k_wattn_bwd_merge, dim3((unsigned)((outputs + 63) / 64)), dim3(64 * WB_SLICES), 0, st, tab_part, pad_part, dbias_table,
                       dqkv_bias, (int)windows, heads, T);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}
