// vkn_trackloss.hip — the tracking loss of a training step on the device: the gather of the positive rows, `track_head.match`,
// `get_track_targets` and `loss` (knet/video/knet_quansi_dense_embed_fc_joint_train.py:439-460, knet/video/track_heads.py:658-716,
// knet/video/qdtrack/losses/{multipos_cross_entropy_loss,l2_loss}.py) and autograd's backward of them.
//
//   vkn_track_loss_fwd_f32   k_tl_fwd (one workgroup of 1024 threads per image) + k_tl_mean (the mean over the images)
//   vkn_track_loss_bwd_f32   k_tl_bwd (one workgroup per image)
//
// Forward, per image: compact the rows with gt > 0 (ascending row order), row norms, D = K R^T by plain fp32 FMA (32 embedding
// columns of all rows staged in LDS per step, transposed; a 2x2 or 4x4 register tile per thread — the e-order of the sums is the
// same in both), D kept in LDS [Kk][Kr].  Then one wave per key row: the two max-shifted logsumexps, softplus and d loss / d dists;
// the L2 loss on clamp(cos - margin, 0, 1) with hard-negative mining as a k-th-largest selection: a 4 x 8-bit radix select over the
// bit patterns of the costs pred^2 >= 0 (integer LDS histograms), ties at the cut to the lowest (k, r) in row-major order through
// ballot ranks.  Every floating-point reduction is a fixed-order wave reduction or a serial loop: no floating-point atomics, the
// same inputs give the same bits, and nothing depends on N beyond the compaction.
// Backward, per image: M = g0 dL/dD + (g0 dL/dcos_track + g1 dL/dcos_aux) / (|k| |r|) in LDS, then
//   d_key = M R - K diag(a / |k|^2),  d_ref = M^T K - R diag(b / |r|^2),  a = rowsum(Gcos * cos), b = colsum(Gcos * cos)
// (the derivative of x / max(|x|, eps) folded into one pass over the raw rows).
#include "../../include/vkn_track_train.h"
#include "vkn_common.h"

namespace {

constexpr int TL_MAX = VKN_TRACK_LOSS_MAX_ROWS;   // rows per image
constexpr int TL_THREADS = 1024;
constexpr int TL_WAVES = TL_THREADS / 64;
constexpr int TL_EC = 32;                         // embedding columns staged per step of the matmul
constexpr float TL_EPS = 1e-12f;                  // F.normalize's clamp on the norm
constexpr int TL_SMALL = 8 * TL_MAX * 4 + 2 * TL_MAX * 4 + 256 * 4 + 64 * 4;   // the small LDS arrays of k_tl_fwd, bytes

inline size_t tl_pad(size_t n) { return (n + 255) & ~(size_t)255; }
// workspace: part fp32 [B][2] (per-image losses), then per image: hdr int32 [4] (Kk, Kr), krow, rrow int32 [N], nk, nr fp32 [N]
// (raw norms), cd, cc, cos fp32 [N * N] (leading dimension Kr)
__host__ __device__ inline size_t tl_img_head(int N) { return (16 + (size_t)N * 16 + 255) & ~(size_t)255; }
__host__ __device__ inline size_t tl_mat(int N) { return ((size_t)N * N * 4 + 255) & ~(size_t)255; }
__host__ __device__ inline size_t tl_img_bytes(int N) { return tl_img_head(N) + 3 * tl_mat(N); }
inline size_t tl_ws_bytes(int B, int N) { return tl_pad((size_t)B * 8) + (size_t)B * tl_img_bytes(N); }
inline size_t tl_fwd_lds(int N) { return (((size_t)N * N * 4 + 15) & ~(size_t)15) + 2 * TL_EC * TL_MAX * 4 + TL_SMALL; }
inline size_t tl_bwd_lds(int N) { return 2 * (((size_t)N * N * 4 + 15) & ~(size_t)15) + 8 * TL_MAX * 4; }

extern __shared__ __attribute__((aligned(16))) char tl_smem[];

__device__ __forceinline__ float tl_margin(const VknTrackLossCfg& c, bool t) {
    const float m = t ? c.pos_margin : c.neg_margin;
    return m > 0.f ? m : 0.f;
}
__device__ __forceinline__ float tl_clamp01(float v) { return v != v ? v : fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ unsigned tl_cost_bits(float pred) { return __float_as_uint(pred * pred); }   // pred in [0, 1]: bit order = value order

// D[k][r] = sum_e K[k][e] R[r][e] for the compacted rows, e ascending, into S (leading dimension Kr).  T x T outputs per thread.
template <int T>
__device__ __forceinline__ void tl_matmul(const float* __restrict__ key, const float* __restrict__ ref, const int* krow, const int* rrow, int Kk,
                                          int Kr, int E, float* Ks, float* Rs, float* S) {
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const bool active = ty * T < Kk && tx * T < Kr;
    float acc[T][T];
    for (int i = 0; i < T; ++i)
        for (int j = 0; j < T; ++j) acc[i][j] = 0.f;
    for (int e0 = 0; e0 < E; e0 += TL_EC) {
        // stage columns [e0, e0 + 32) of every row, transposed: Ks[e][k], Rs[e][r]; rows beyond Kk / Kr and columns beyond E are zero
        for (int idx = tid; idx < 2 * TL_MAX * (TL_EC / 4); idx += TL_THREADS) {
            const int row = idx & (2 * TL_MAX - 1), c4 = idx >> 8;
            const bool isk = row < TL_MAX;
            const int q = isk ? row : row - TL_MAX;
            const int e = e0 + c4 * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < (isk ? Kk : Kr) && e < E) v = *reinterpret_cast<const float4*>((isk ? key + (size_t)krow[q] * E : ref + (size_t)rrow[q] * E) + e);
            float* dst = (isk ? Ks : Rs) + (c4 * 4) * TL_MAX + q;
            dst[0] = v.x; dst[TL_MAX] = v.y; dst[2 * TL_MAX] = v.z; dst[3 * TL_MAX] = v.w;
        }
        __syncthreads();
        if (active) {
            const int ne = E - e0 < TL_EC ? E - e0 : TL_EC;
            for (int e = 0; e < ne; ++e) {
                float a[T], c[T];
                for (int i = 0; i < T; ++i) a[i] = Ks[e * TL_MAX + ty * T + i];
                for (int j = 0; j < T; ++j) c[j] = Rs[e * TL_MAX + tx * T + j];
                for (int i = 0; i < T; ++i)
                    for (int j = 0; j < T; ++j) acc[i][j] = fmaf(a[i], c[j], acc[i][j]);
            }
        }
        __syncthreads();
    }
    if (active)
        for (int i = 0; i < T; ++i)
            for (int j = 0; j < T; ++j)
                if (ty * T + i < Kk && tx * T + j < Kr) S[(ty * T + i) * Kr + tx * T + j] = acc[i][j];
}

__global__ __launch_bounds__(TL_THREADS) void k_tl_fwd(const float* __restrict__ key_all, const float* __restrict__ ref_all,
                                                        const long long* __restrict__ kgt, const long long* __restrict__ rgt,
                                                        const long long* __restrict__ match, const long long* __restrict__ moff,
                                                        long long n_match, int N, int E, VknTrackLossCfg cfg, int B, float* part,
                                                        char* imgws, int* __restrict__ stats, unsigned char* __restrict__ aux_kept,
                                                        int* __restrict__ status) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    char* p = tl_smem;
    float* S = reinterpret_cast<float*>(p); p += ((size_t)N * N * 4 + 15) & ~(size_t)15;
    float* Ks = reinterpret_cast<float*>(p); p += TL_EC * TL_MAX * 4;
    float* Rs = reinterpret_cast<float*>(p); p += TL_EC * TL_MAX * 4;
    int* krow = reinterpret_cast<int*>(p); p += TL_MAX * 4;    // compact key row -> original row
    int* rrow = reinterpret_cast<int*>(p); p += TL_MAX * 4;
    int* mk = reinterpret_cast<int*>(p); p += TL_MAX * 4;      // compact key row -> partner instance in the reference frame, -1: none
    int* rg = reinterpret_cast<int*>(p); p += TL_MAX * 4;      // compact reference row -> its instance
    float* nk = reinterpret_cast<float*>(p); p += TL_MAX * 4;  // raw norms
    float* nr = reinterpret_cast<float*>(p); p += TL_MAX * 4;
    int* invk = reinterpret_cast<int*>(p); p += TL_MAX * 4;    // original row -> compact row, -1: not a positive
    int* invr = reinterpret_cast<int*>(p); p += TL_MAX * 4;
    int* cnt = reinterpret_cast<int*>(p); p += TL_MAX * 4;     // per key row: positives, later: entries equal to the cut
    float* rowf = reinterpret_cast<float*>(p); p += TL_MAX * 4;
    int* hist = reinterpret_cast<int*>(p); p += 256 * 4;       // step 0: the two gt columns before compaction; then the radix histogram
    int* misc = reinterpret_cast<int*>(p);

    const float* key = key_all + (size_t)b * N * E;
    const float* ref = ref_all + (size_t)b * N * E;
    char* iw = imgws + (size_t)b * tl_img_bytes(N);
    int* w_hdr = reinterpret_cast<int*>(iw);
    float* w_cd = reinterpret_cast<float*>(iw + tl_img_head(N));
    float* w_cc = reinterpret_cast<float*>(iw + tl_img_head(N) + tl_mat(N));
    float* w_cos = reinterpret_cast<float*>(iw + tl_img_head(N) + 2 * tl_mat(N));

    // ---- 0. read and validate the gt columns, compact the positives
    {
        const long long o0 = moff[b], o1 = moff[b + 1];
        const bool okoff = o0 >= 0 && o1 >= o0 && o1 <= n_match;
        const long long G = okoff ? o1 - o0 : 0;
        bool bad = !okoff && tid == 0;
        if (tid < N) {
            long long g = kgt[(size_t)b * N + tid];
            if (g < 0 || g > G) { bad = true; g = 0; }
            long long m = -1;
            if (g > 0) {
                m = match[o0 + g - 1];
                if (m < -1 || m > 0x7ffffffeLL) { bad = true; m = -1; }
            }
            hist[tid] = g > 0 ? 1 : 0;
            Ks[tid] = __int_as_float((int)m);
        } else if (tid >= 512 && tid < 512 + N) {
            const int i = tid - 512;
            long long g = rgt[(size_t)b * N + i];
            if (g < 0 || g > 0x7fffffffLL) { bad = true; g = 0; }
            hist[TL_MAX + i] = g > 0 ? 1 : 0;
            Rs[i] = __int_as_float((int)(g - 1));
        }
        if (bad) atomicOr(status, (int)VKN_STATUS_RANGE);
    }
    __syncthreads();
    if (tid < N || (tid >= 512 && tid < 512 + N)) {
        const bool isk = tid < N;
        const int i = isk ? tid : tid - 512;
        const int* flag = hist + (isk ? 0 : TL_MAX);
        int s = 0;
        for (int j = 0; j < i; ++j) s += flag[j];
        (isk ? invk : invr)[i] = flag[i] ? s : -1;
        if (flag[i]) {
            (isk ? krow : rrow)[s] = i;
            (isk ? mk : rg)[s] = __float_as_int((isk ? Ks : Rs)[i]);
        }
        if (i == N - 1) misc[isk ? 0 : 1] = s + flag[i];
    }
    __syncthreads();
    const int Kk = misc[0], Kr = misc[1];
    // targets: positives per key row, num_pos, sum of the weights
    for (int k = tid; k < Kk; k += TL_THREADS) {
        int c = 0;
        for (int r = 0; r < Kr; ++r) c += mk[k] == rg[r];
        cnt[k] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int np = 0, ws = 0;
        for (int k = 0; k < Kk; ++k) { np += cnt[k]; ws += cnt[k] > 0; }
        misc[2] = np; misc[3] = ws;
    }
    // ---- 1. row norms: one wave per row, lanes over float4 columns, fixed-order wave sum
    for (int q = wave; q < Kk + Kr; q += TL_WAVES) {
        const float* x = q < Kk ? key + (size_t)krow[q] * E : ref + (size_t)rrow[q - Kk] * E;
        float a = 0.f;
        for (int e4 = lane; e4 < E / 4; e4 += 64) {
            const float4 v = reinterpret_cast<const float4*>(x)[e4];
            a = fmaf(v.x, v.x, a); a = fmaf(v.y, v.y, a); a = fmaf(v.z, v.z, a); a = fmaf(v.w, v.w, a);
        }
        a = vkn_wave_sum(a);
        if (lane == 0) (q < Kk ? nk[q] : nr[q - Kk]) = sqrtf(a);
    }
    __syncthreads();
    const int num_pos = misc[2], wsum = misc[3];
    // ---- 2. D = K R^T
    if (Kk <= 64 && Kr <= 64) tl_matmul<2>(key, ref, krow, rrow, Kk, Kr, E, Ks, Rs, S);
    else tl_matmul<4>(key, ref, krow, rrow, Kk, Kr, E, Ks, Rs, S);
    __syncthreads();
    // ---- 3. MultiPosCrossEntropyLoss: one wave per key row
    const bool use_temp = cfg.softmax_temp > 0.f;
    const float ce_scale = cfg.w_track / (float)wsum / (float)B;
    for (int k = wave; k < Kk; k += TL_WAVES) {
        const int m = mk[k];
        const float nkc = fmaxf(nk[k], TL_EPS);
        float mxn = -INFINITY, mxp = -INFINITY;
        for (int r = lane; r < Kr; r += 64) {
            const float d = S[k * Kr + r];
            const float c = d / (nkc * fmaxf(nr[r], TL_EPS));
            w_cos[k * Kr + r] = c;
            const float s = use_temp ? c / cfg.softmax_temp : d;
            if (m == rg[r]) mxp = fmaxf(mxp, -s); else mxn = fmaxf(mxn, s);
        }
        mxn = vkn_wave_max(mxn); mxp = vkn_wave_max(mxp);
        float sn = 0.f, sp = 0.f;
        for (int r = lane; r < Kr; r += 64) {
            const float d = S[k * Kr + r];
            const float s = use_temp ? d / (nkc * fmaxf(nr[r], TL_EPS)) / cfg.softmax_temp : d;
            if (m == rg[r]) sp += expf(-s - mxp); else sn += expf(s - mxn);
        }
        sn = vkn_wave_sum(sn); sp = vkn_wave_sum(sp);
        const float lse_n = mxn + logf(sn), lse_p = mxp + logf(sp);       // a row without negatives / positives: -inf + log(0) = -inf
        const float both = lse_n + lse_p;
        const bool fin = both - both == 0.f;                              // finite
        float loss = 0.f, sig = 0.f;
        if (fin) {
            if (both > 20.f) { loss = both; sig = 1.f; }                  // F.softplus: threshold 20
            else { const float z = expf(both); loss = log1pf(z); sig = z / (z + 1.f); }
        }
        if (lane == 0) rowf[k] = cnt[k] > 0 ? loss : 0.f;
        const float coef = (fin && cnt[k] > 0) ? ce_scale * sig : 0.f;
        for (int r = lane; r < Kr; r += 64) {
            const float d = S[k * Kr + r];
            const float s = use_temp ? d / (nkc * fmaxf(nr[r], TL_EPS)) / cfg.softmax_temp : d;
            float g = 0.f;
            if (coef != 0.f) g = (m == rg[r]) ? -coef * expf(-s - lse_p) : coef * expf(s - lse_n);
            w_cd[k * Kr + r] = g;
        }
    }
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int k = 0; k < Kk; ++k) t += rowf[k];
        part[2 * b] = cfg.w_track * (t / (float)wsum);                     // 0 / 0 = NaN: no key of this image has a partner
        if (!cfg.has_aux) part[2 * b + 1] = 0.f;
    }
    int kept_neg = 0;
    if (cfg.has_aux) {
        // ---- 4. L2Loss: S becomes pred = clamp(cos - margin, 0, 1)
        const int total = Kk * Kr, num_neg = total - num_pos;
        for (int idx = tid; idx < total; idx += TL_THREADS) {
            const int k = idx / Kr, r = idx - k * Kr;
            S[idx] = tl_clamp01(w_cos[idx] - tl_margin(cfg, mk[k] == rg[r]));
        }
        const bool mine = cfg.neg_pos_ub > 0 && (long long)num_neg > (long long)cfg.neg_pos_ub * (num_pos + 1);
        const int keep = mine ? num_pos * cfg.neg_pos_ub : num_neg;        // mine: keep < num_neg
        kept_neg = keep;
        unsigned cut = 0;      // bit pattern of the keep-th largest cost
        int need_eq = 0;       // how many entries equal to the cut stay (the first ones in row-major order)
        __syncthreads();
        if (mine && keep > 0) {
            unsigned prefix = 0;
            int remaining = keep;
            for (int shift = 24; shift >= 0; shift -= 8) {
                if (tid < 256) hist[tid] = 0;
                __syncthreads();
                for (int idx = tid; idx < total; idx += TL_THREADS) {
                    const int k = idx / Kr, r = idx - k * Kr;
                    if (mk[k] == rg[r]) continue;
                    const unsigned bits = tl_cost_bits(S[idx]);
                    if (shift == 24 || (bits >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(bits >> shift) & 255], 1);
                }
                __syncthreads();
                if (tid == 0) {
                    int cum = 0, d = 255;
                    for (; d > 0; --d) {
                        if (cum + hist[d] >= remaining) break;
                        cum += hist[d];
                    }
                    misc[4] = (int)(prefix | ((unsigned)d << shift));
                    misc[5] = remaining - cum;
                }
                __syncthreads();
                prefix = (unsigned)misc[4];
                remaining = misc[5];
            }
            cut = prefix;
            need_eq = remaining;
            // entries equal to the cut per row, then their exclusive prefix over the rows
            for (int k = wave; k < Kk; k += TL_WAVES) {
                int c = 0;
                for (int it = 0; it * 64 < Kr; ++it) {
                    const int r = it * 64 + lane;
                    const bool eq = r < Kr && mk[k] != rg[r] && tl_cost_bits(S[k * Kr + r]) == cut;
                    c += __popcll(__ballot(eq));
                }
                if (lane == 0) cnt[k] = c;
            }
            __syncthreads();
            if (tid == 0) {
                int run = 0;
                for (int k = 0; k < Kk; ++k) { const int c = cnt[k]; cnt[k] = run; run += c; }
            }
            __syncthreads();
        }
        const int nkept = num_pos + keep;
        const float l2_scale = cfg.w_aux / (float)nkept / (float)B;       // nkept == 0: inf, and inf * 0 below is the host path's NaN
        for (int k = wave; k < Kk; k += TL_WAVES) {
            const int m = mk[k];
            int base = (mine && keep > 0) ? cnt[k] : 0;
            float rs = 0.f;
            for (int it = 0; it * 64 < Kr; ++it) {
                const int r = it * 64 + lane;
                const bool valid = r < Kr;
                const int idx = k * Kr + (valid ? r : 0);
                const bool t = valid && m == rg[r];
                const float pred = S[idx];
                const unsigned bits = tl_cost_bits(pred);
                const bool eq = valid && !t && mine && keep > 0 && bits == cut;
                const unsigned long long mask = __ballot(eq);
                const int rank = base + __popcll(mask & ((1ull << lane) - 1ull));
                base += __popcll(mask);
                bool kept = valid;
                if (valid && !t && mine) kept = keep > 0 && (bits > cut || (eq && rank < need_eq));
                const float diff = pred - (t ? 1.f : 0.f);
                if (kept) rs += diff * diff;
                if (valid) {
                    const float cm = w_cos[idx] - tl_margin(cfg, t);
                    const bool inside = cm >= 0.f && cm <= 1.f;
                    w_cc[idx] = inside ? l2_scale * (kept ? 1.f : 0.f) * (2.f * diff) : 0.f;
                }
                if (valid) S[idx] = kept ? 1.f : 0.f;      // S becomes the kept mask (each lane replaces the entry it has just read)
            }
            rs = vkn_wave_sum(rs);
            if (lane == 0) rowf[k] = rs;
        }
        __syncthreads();
        if (tid == 0) {
            float t = 0.f;
            for (int k = 0; k < Kk; ++k) t += rowf[k];
            part[2 * b + 1] = cfg.w_aux * (t / (float)nkept);              // 0 / 0 = NaN, as the host path
        }
    }
    // ---- 5. what the caller and the backward read
    if (aux_kept) {
        unsigned char* plane = aux_kept + (size_t)b * N * N;
        for (int idx = tid; idx < N * N; idx += TL_THREADS) {
            const int i = idx / N, j = idx - i * N;
            const int k = invk[i], r = invr[j];
            plane[idx] = (cfg.has_aux && k >= 0 && r >= 0 && S[k * Kr + r] != 0.f) ? 1 : 0;
        }
    }
    int* w_krow = w_hdr + 4;
    int* w_rrow = w_krow + N;
    float* w_nk = reinterpret_cast<float*>(w_rrow + N);
    float* w_nr = w_nk + N;
    if (tid < N) {
        w_krow[tid] = tid < Kk ? krow[tid] : 0;
        w_rrow[tid] = tid < Kr ? rrow[tid] : 0;
        w_nk[tid] = tid < Kk ? nk[tid] : 0.f;
        w_nr[tid] = tid < Kr ? nr[tid] : 0.f;
    }
    if (tid == 0) {
        w_hdr[0] = Kk; w_hdr[1] = Kr; w_hdr[2] = 0; w_hdr[3] = 0;
        stats[4 * b] = Kk; stats[4 * b + 1] = Kr; stats[4 * b + 2] = num_pos; stats[4 * b + 3] = kept_neg;
    }
}

// losses[j] = (sum_b part[b][j]) / B: thread-strided partial sums in image order, then a fixed tree
__global__ __launch_bounds__(256) void k_tl_mean(const float* __restrict__ part, int B, float* __restrict__ losses) {
    __shared__ float s[2][256];
    const int tid = threadIdx.x;
    float a = 0.f, c = 0.f;
    for (int b = tid; b < B; b += 256) { a += part[2 * b]; c += part[2 * b + 1]; }
    s[0][tid] = a; s[1][tid] = c;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) { s[0][tid] += s[0][tid + h]; s[1][tid] += s[1][tid + h]; }
        __syncthreads();
    }
    if (tid < 2) losses[tid] = s[tid][0] / (float)B;
}

// out[row of i][e] = sum_j coef(i, j) X[row of j][e] - Y[row of i][e] * sub[i] for the compacted rows, zero for every other row.
// TR: coef(i, j) = M[j][i] (the reference side), else M[i][j].  Four rows i and one float4 of e per thread and step; j ascending.
template <bool TR>
__device__ __forceinline__ void tl_grad_rows(const float* __restrict__ X, const float* __restrict__ Y, const int* xrow, const int* yrow,
                                             const int* inv, const float* M, int ld, int ni, int nj, const float* sub, int N, int E,
                                             float* __restrict__ out) {
    const int tid = threadIdx.x, E4 = E / 4;
    for (int idx = tid; idx < N * E4; idx += TL_THREADS) {
        const int i = idx / E4;
        if (inv[i] < 0) reinterpret_cast<float4*>(out)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int groups = (ni + 3) / 4;
    for (int item = tid; item < groups * E4; item += TL_THREADS) {
        const int g = item / E4, e4 = item - g * E4, i0 = g * 4;
        const int nv = ni - i0 < 4 ? ni - i0 : 4;
        float4 acc[4];
        for (int q = 0; q < 4; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < nj; ++j) {
            const float4 x = reinterpret_cast<const float4*>(X + (size_t)xrow[j] * E)[e4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q < nv) {
                    const float m = TR ? M[j * ld + i0 + q] : M[(i0 + q) * ld + j];
                    acc[q].x = fmaf(m, x.x, acc[q].x); acc[q].y = fmaf(m, x.y, acc[q].y);
                    acc[q].z = fmaf(m, x.z, acc[q].z); acc[q].w = fmaf(m, x.w, acc[q].w);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q >= nv) break;
            const size_t o = (size_t)yrow[i0 + q] * E4 + e4;
            const float4 y = reinterpret_cast<const float4*>(Y)[o];
            const float s = sub[i0 + q];
            float4 v = acc[q];
            if (s != 0.f) { v.x = fmaf(-s, y.x, v.x); v.y = fmaf(-s, y.y, v.y); v.z = fmaf(-s, y.z, v.z); v.w = fmaf(-s, y.w, v.w); }
            reinterpret_cast<float4*>(out)[o] = v;
        }
    }
}

__global__ __launch_bounds__(TL_THREADS) void k_tl_bwd(const float* __restrict__ key_all, const float* __restrict__ ref_all,
                                                        const char* __restrict__ imgws, const float* __restrict__ gout, int N, int E,
                                                        VknTrackLossCfg cfg, float* __restrict__ dkey_all, float* __restrict__ dref_all) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    char* p = tl_smem;
    const size_t msz = ((size_t)N * N * 4 + 15) & ~(size_t)15;
    float* M = reinterpret_cast<float*>(p); p += msz;          // coefficient on the raw dot products, cosine part folded in
    float* P = reinterpret_cast<float*>(p); p += msz;          // Gcos * cos
    int* krow = reinterpret_cast<int*>(p); p += TL_MAX * 4;
    int* rrow = reinterpret_cast<int*>(p); p += TL_MAX * 4;
    float* nk = reinterpret_cast<float*>(p); p += TL_MAX * 4;
    float* nr = reinterpret_cast<float*>(p); p += TL_MAX * 4;
    float* sk = reinterpret_cast<float*>(p); p += TL_MAX * 4;
    float* sr = reinterpret_cast<float*>(p); p += TL_MAX * 4;
    int* invk = reinterpret_cast<int*>(p); p += TL_MAX * 4;
    int* invr = reinterpret_cast<int*>(p);

    const char* iw = imgws + (size_t)b * tl_img_bytes(N);
    const int* w_hdr = reinterpret_cast<const int*>(iw);
    const int* w_krow = w_hdr + 4;
    const int* w_rrow = w_krow + N;
    const float* w_nk = reinterpret_cast<const float*>(w_rrow + N);
    const float* w_nr = w_nk + N;
    const float* w_cd = reinterpret_cast<const float*>(iw + tl_img_head(N));
    const float* w_cc = reinterpret_cast<const float*>(iw + tl_img_head(N) + tl_mat(N));
    const float* w_cos = reinterpret_cast<const float*>(iw + tl_img_head(N) + 2 * tl_mat(N));
    // the workspace is the forward's; whatever it holds, nothing below leaves the buffers
    int Kk = w_hdr[0], Kr = w_hdr[1];
    Kk = Kk < 0 ? 0 : (Kk > N ? N : Kk);
    Kr = Kr < 0 ? 0 : (Kr > N ? N : Kr);
    if (tid < N) { invk[tid] = -1; invr[tid] = -1; }
    __syncthreads();
    if (tid < Kk) {
        int i = w_krow[tid];
        i = i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
        krow[tid] = i; invk[i] = tid; nk[tid] = w_nk[tid];
    }
    if (tid < Kr) {
        int i = w_rrow[tid];
        i = i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
        rrow[tid] = i; invr[i] = tid; nr[tid] = w_nr[tid];
    }
    __syncthreads();
    const float g0 = gout[0], g1 = gout[1];
    const bool use_temp = cfg.softmax_temp > 0.f;
    const int total = Kk * Kr;
    for (int idx = tid; idx < total; idx += TL_THREADS) {
        const int k = idx / Kr, r = idx - k * Kr;
        const float cd = g0 * w_cd[idx];
        float gc = use_temp ? cd / cfg.softmax_temp : 0.f;
        if (cfg.has_aux) gc += g1 * w_cc[idx];
        M[idx] = (use_temp ? 0.f : cd) + gc / (fmaxf(nk[k], TL_EPS) * fmaxf(nr[r], TL_EPS));
        P[idx] = gc * w_cos[idx];
    }
    __syncthreads();
    // the projection terms of d (x / |x|): row sums by one wave per row, column sums by one thread per column (k ascending)
    for (int k = wave; k < Kk; k += TL_WAVES) {
        float a = 0.f;
        for (int r = lane; r < Kr; r += 64) a += P[k * Kr + r];
        a = vkn_wave_sum(a);
        if (lane == 0) sk[k] = nk[k] >= TL_EPS ? a / (nk[k] * nk[k]) : 0.f;   // below the clamp the norm carries no gradient
    }
    for (int r = tid; r < Kr; r += TL_THREADS) {
        float a = 0.f;
        for (int k = 0; k < Kk; ++k) a += P[k * Kr + r];
        sr[r] = nr[r] >= TL_EPS ? a / (nr[r] * nr[r]) : 0.f;
    }
    __syncthreads();
    const float* key = key_all + (size_t)b * N * E;
    const float* ref = ref_all + (size_t)b * N * E;
    tl_grad_rows<false>(ref, key, rrow, krow, invk, M, Kr, Kk, Kr, sk, N, E, dkey_all + (size_t)b * N * E);
    tl_grad_rows<true>(key, ref, krow, rrow, invr, M, Kr, Kr, Kk, sr, N, E, dref_all + (size_t)b * N * E);
}

inline int tl_check(const VknTrackLossCfg* cfg, int B, int N, int E) {
    if (!cfg) return VKN_E_ARG;
    if (N < 1 || N > TL_MAX || E < 4 || E > 1024 || E % 4 != 0 || B < 1 || B > 65535) return VKN_E_SHAPE;
    return VKN_OK;
}

}  // namespace

extern "C" {

size_t vkn_sizeof_track_loss_cfg(void) { return sizeof(VknTrackLossCfg); }

size_t vkn_track_loss_workspace_bytes(int B, int N) {
    if (B < 1 || B > 65535 || N < 1 || N > TL_MAX) return 0;
    return tl_ws_bytes(B, N);
}

int vkn_track_loss_fwd_f32(const VknTrackLossCfg* cfg, const float* key_embeds, const float* ref_embeds, const int64_t* key_gt,
                           const int64_t* ref_gt, const int64_t* match, const int64_t* match_off, long long n_match, int B, int N, int E,
                           float* losses, int* stats, unsigned char* aux_kept, int* status, void* ws, size_t ws_bytes, void* stream) {
    if (!cfg || !key_embeds || !ref_embeds || !key_gt || !ref_gt || !match || !match_off || !losses || !stats || !status || n_match < 0)
        return VKN_E_ARG;
    const int rc = tl_check(cfg, B, N, E);
    if (rc != VKN_OK) return rc;
    const void* ptrs[] = {key_embeds, ref_embeds, key_gt, ref_gt, match, match_off, losses, stats};
    for (const void* p : ptrs)
        if (!vkn_aligned(p, 16)) return VKN_E_ALIGN;
    if (reinterpret_cast<uintptr_t>(status) & 3) return VKN_E_ALIGN;
    if (!ws || ws_bytes < tl_ws_bytes(B, N) || !vkn_aligned(ws, 16)) return VKN_E_WORKSPACE;
    for (const void* p : ptrs)
        if (!vkn_on_device(p)) return VKN_E_ARG;
    if (!vkn_on_device(status) || !vkn_on_device(ws) || (aux_kept && !vkn_on_device(aux_kept))) return VKN_E_ARG;

    hipStream_t st = static_cast<hipStream_t>(stream);
    VKN_ALLOW_FULL_LDS(k_tl_fwd);
    float* part = static_cast<float*>(ws);
    char* imgws = static_cast<char*>(ws) + tl_pad((size_t)B * 8);
    hipLaunchKernelGGL(k_tl_fwd, dim3(B), dim3(TL_THREADS), tl_fwd_lds(N), st, key_embeds, ref_embeds, reinterpret_cast<const long long*>(key_gt),
                       reinterpret_cast<const long long*>(ref_gt), reinterpret_cast<const long long*>(match),
                       reinterpret_cast<const long long*>(match_off), n_match, N, E, *cfg, B, part, imgws, stats, aux_kept, status);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_tl_mean, dim3(1), dim3(256), 0, st, part, B, losses);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

int vkn_track_loss_bwd_f32(const VknTrackLossCfg* cfg, const float* key_embeds, const float* ref_embeds, const float* gout, int B, int N,
                           int E, float* d_key, float* d_ref, const void* ws, size_t ws_bytes, void* stream) {
    if (!cfg || !key_embeds || !ref_embeds || !gout || !d_key || !d_ref) return VKN_E_ARG;
    const int rc = tl_check(cfg, B, N, E);
    if (rc != VKN_OK) return rc;
    const void* ptrs[] = {key_embeds, ref_embeds, gout, d_key, d_ref};
    for (const void* p : ptrs)
        if (!vkn_aligned(p, 16)) return VKN_E_ALIGN;
    if (!ws || ws_bytes < tl_ws_bytes(B, N) || !vkn_aligned(ws, 16)) return VKN_E_WORKSPACE;
    for (const void* p : ptrs)
        if (!vkn_on_device(p)) return VKN_E_ARG;
    if (!vkn_on_device(ws)) return VKN_E_ARG;

    hipStream_t st = static_cast<hipStream_t>(stream);
    VKN_ALLOW_FULL_LDS(k_tl_bwd);
    const char* imgws = static_cast<const char*>(ws) + tl_pad((size_t)B * 8);
    hipLaunchKernelGGL(k_tl_bwd, dim3(B), dim3(TL_THREADS), tl_bwd_lds(N), st, key_embeds, ref_embeds, imgws, gout, N, E, *cfg, d_key, d_ref);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

}  // extern "C"
