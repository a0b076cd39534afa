// vkn_swin.hip — the (shifted-)window attention core of the Swin backbone (include/vkn_swin.h) for gfx950.
//
// A workgroup owns one window of the rolled map and a group of heads; a WAVE owns one head, and shares nothing with the other waves but
// the barrier.  The wave stages K and V of its head (window^2 x 32 floats each) and the head's column of the relative-position table
// in LDS: 128-byte segments per token, read from `qkv` where it lies (a pad token from `qkv_bias`).  Lane i then holds query row i
// (pre-scaled, 32 registers) and walks the keys: every K / V read is ONE address for the whole wave (an LDS broadcast, no bank
// conflict), the window^2 scores stay in registers (the key loop is unrolled: `window` is a template parameter), the maximum, the
// exponentials and the 32 accumulators of P V follow in plain fp32 FMA, ONE reciprocal at the end.  `qkv` is read once, `out` written once.
//
// Safety: every address is formed from a token position that was reduced modulo the padded extent and compared with H, W first; pad
// positions form no global address at all.  No input VALUE reaches an address.
#include "../../include/vkn_swin.h"
#include "vkn_common.h"

namespace {

constexpr int SWIN_D = VKN_SWIN_HEAD_DIM;
constexpr int SWIN_LDS_BYTES = 65536;     // what a workgroup may take without asking for more

struct SwinGeom {
    int H, W, Hp, Wp, nWw, nWin, heads, shift;      // nWin: windows of one image
};

__host__ __device__ constexpr int swin_wave_floats(int ws) { return (2 * ws * ws * SWIN_D + (2 * ws - 1) * (2 * ws - 1) + 3) & ~3; }

// r(s, E) of the header: the slice of the rolled axis that position s falls in
__device__ __forceinline__ int swin_region(int s, int E, int ws, int shift) { return s < E - ws ? 0 : (s < E - shift ? 1 : 2); }

template <int WS>
__global__ __launch_bounds__(256) void k_swin_window_attn(const float* __restrict__ qkv, const float* __restrict__ qkv_bias,
                                                          const float* __restrict__ table, float* __restrict__ out, SwinGeom g, float scale) {
    constexpr int N = WS * WS, R = 2 * WS - 1, T = R * R, D = SWIN_D;
    extern __shared__ f32x4 swin_lds[];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int head = (int)blockIdx.y * ((int)blockDim.x >> 6) + wave;
    const bool head_live = head < g.heads;
    const int b = (int)blockIdx.x / g.nWin, wi = (int)blockIdx.x % g.nWin, wy0 = (wi / g.nWw) * WS, wx0 = (wi % g.nWw) * WS;
    float* Ks = reinterpret_cast<float*>(swin_lds) + wave * swin_wave_floats(WS);
    float* Vs = Ks + N * D;
    float* tab = Vs + N * D;
    const size_t HD = (size_t)g.heads * D;
    if (head_live) {
        for (int idx = lane; idx < N * (D / 4); idx += 64) {
            const int t = idx / (D / 4), c = (idx % (D / 4)) * 4;
            int py = wy0 + t / WS + g.shift, px = wx0 + t % WS + g.shift;      // the padded-map token that the roll put here
            py -= py >= g.Hp ? g.Hp : 0;
            px -= px >= g.Wp ? g.Wp : 0;
            f32x4 k = {0.f, 0.f, 0.f, 0.f}, v = k;
            if (py < g.H && px < g.W) {
                const float* p = qkv + (((size_t)b * g.H + py) * g.W + px) * (3 * HD) + (size_t)head * D + c;
                k = *reinterpret_cast<const f32x4*>(p + HD);
                v = *reinterpret_cast<const f32x4*>(p + 2 * HD);
            } else if (qkv_bias) {                                              // a pad token: qkv(0) = the bias
                k = *reinterpret_cast<const f32x4*>(qkv_bias + HD + (size_t)head * D + c);
                v = *reinterpret_cast<const f32x4*>(qkv_bias + 2 * HD + (size_t)head * D + c);
            }
            *reinterpret_cast<f32x4*>(Ks + t * D + c) = k;
            *reinterpret_cast<f32x4*>(Vs + t * D + c) = v;
        }
        for (int i = lane; i < T; i += 64) tab[i] = table[(size_t)i * g.heads + head];
    }
    __syncthreads();
    if (!head_live || lane >= N) return;
    const int ty = lane / WS, tx = lane % WS;
    int py = wy0 + ty + g.shift, px = wx0 + tx + g.shift;
    py -= py >= g.Hp ? g.Hp : 0;
    px -= px >= g.Wp ? g.Wp : 0;
    if (py >= g.H || px >= g.W) return;                                         // a pad query: its output is cropped away
    const size_t tok = ((size_t)b * g.H + py) * g.W + px;
    f32x4 q[D / 4];
#pragma unroll
    for (int c = 0; c < D / 4; ++c) q[c] = *reinterpret_cast<const f32x4*>(qkv + tok * (3 * HD) + (size_t)head * D + 4 * c) * scale;
    const bool masked = g.shift > 0;
    const int rq = 3 * swin_region(wy0 + ty, g.Hp, WS, g.shift) + swin_region(wx0 + tx, g.Wp, WS, g.shift);
    const float* tq = tab + (ty + WS - 1) * R + (tx + WS - 1);                  // tq[-(y_j R + x_j)] = table[rel(i, j)]
    float s[N];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const f32x4* kj = reinterpret_cast<const f32x4*>(Ks + j * D);
        f32x4 a4 = q[0] * kj[0];
#pragma unroll
        for (int c = 1; c < D / 4; ++c) a4 = q[c] * kj[c] + a4;
        float a = (a4.x + a4.y) + (a4.z + a4.w);
        a += tq[-((j / WS) * R + (j % WS))];
        const int rk = 3 * swin_region(wy0 + j / WS, g.Hp, WS, g.shift) + swin_region(wx0 + j % WS, g.Wp, WS, g.shift);
        a += (masked && rk != rq) ? (float)VKN_SWIN_MASK : 0.f;
        s[j] = a;
        mx = fmaxf(mx, a);
    }
    f32x4 acc[D / 4];
#pragma unroll
    for (int c = 0; c < D / 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float p = expf(s[j] - mx);
        den += p;
        const f32x4* vj = reinterpret_cast<const f32x4*>(Vs + j * D);
#pragma unroll
        for (int c = 0; c < D / 4; ++c) acc[c] = p * vj[c] + acc[c];
    }
    const float inv = 1.f / den;
    float* o = out + tok * HD + (size_t)head * D;
#pragma unroll
    for (int c = 0; c < D / 4; ++c) *reinterpret_cast<f32x4*>(o + 4 * c) = acc[c] * inv;
}

}  // namespace

extern "C" int vkn_swin_window_attn_supported(int B, int H, int W, int heads, int window, int shift) {
    if (B < 1 || H < 1 || W < 1 || heads < 1 || heads > VKN_SWIN_MAX_HEADS) return 0;
    if (window < 1 || window * window > VKN_SWIN_MAX_WINDOW_TOKENS || shift < 0 || shift >= window) return 0;
    const long long limit = 1ll << 31, row = 3ll * heads * SWIN_D * (long long)sizeof(float);
    const long long map = (long long)H * W;
    if (map >= limit || map * B >= limit) return 0;
    return map * B * row < limit;                                               // qkv, the largest tensor, below 2^31 bytes
}

extern "C" int vkn_swin_window_attn_f32(const float* qkv, const float* qkv_bias, const float* bias_table, float* out, int B, int H, int W,
                                        int heads, int window, int shift, float scale, void* stream) {
    if (!qkv || !bias_table || !out || B <= 0 || H <= 0 || W <= 0 || heads <= 0) return VKN_E_ARG;
    if (!vkn_swin_window_attn_supported(B, H, W, heads, window, shift)) return VKN_E_SHAPE;
    if (!vkn_aligned(qkv, 16) || !vkn_aligned(qkv_bias, 16) || !vkn_aligned(bias_table, 16) || !vkn_aligned(out, 16)) return VKN_E_ALIGN;
    SwinGeom g;
    g.H = H, g.W = W, g.heads = heads, g.shift = shift;
    const int nWh = (H + window - 1) / window;
    g.nWw = (W + window - 1) / window;
    g.Hp = nWh * window, g.Wp = g.nWw * window, g.nWin = nWh * g.nWw;
    // waves (= heads) of a workgroup: as many as the LDS admits, at most four, and a divisor of `heads` where one exists
    const int wave_bytes = swin_wave_floats(window) * (int)sizeof(float);
    const int most = SWIN_LDS_BYTES / wave_bytes < 4 ? SWIN_LDS_BYTES / wave_bytes : 4;
    int hg = most < heads ? most : heads;
    for (int d = hg; d > 1; --d)
        if (heads % d == 0) {
            hg = d;
            break;
        }
    const dim3 grid((unsigned)((long long)B * g.nWin), (unsigned)((heads + hg - 1) / hg)), block(64 * hg);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define SWIN_LAUNCH(WS)                                                                                                                 \
    case WS:                                                                                                                            \
        hipLaunchKernelGGL((k_swin_window_attn<WS>), grid, block, (size_t)hg * wave_bytes, st, qkv, qkv_bias, bias_table, out, g, scale); \
        break
    switch (window) {
        SWIN_LAUNCH(1);
        SWIN_LAUNCH(2);
        SWIN_LAUNCH(3);
        SWIN_LAUNCH(4);
        SWIN_LAUNCH(5);
        SWIN_LAUNCH(6);
        SWIN_LAUNCH(7);
        SWIN_LAUNCH(8);
    }
#undef SWIN_LAUNCH
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}
