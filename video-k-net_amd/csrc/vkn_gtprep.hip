// vkn_gtprep.hip — the ground truth of a training step on the device (include/vkn_gt.h): class presence + stuff labels of the
// semantic maps, the fp32 bank of down-scaled thing and stuff masks in the training tail's row order, and gt_match_indices.
//
// All three are memory-bound byte shuffles.  The bank fill is laid out for that: a thread owns 4 neighbouring outputs of one output
// row, so a wave covers 256 consecutive outputs = 1 KiB per store instruction, and reads 4 s contiguous bytes per source row (only the
// two centre rows of every s x s cell are touched).  No per-element integer divide: output coordinates come from the 3-D grid.
#include "../../include/vkn_gt.h"
#include "vkn_common.h"

namespace {

constexpr int GT_THREADS = 256;
constexpr int GT_ROWS = GT_THREADS / 64;       // output rows per workgroup of the fill (one wave per row)
constexpr int GT_COLS = 64 * 4;                // output columns per workgroup
constexpr int GP_ROWS = 8;                     // map rows per workgroup of the presence pass

struct GtBatch { VknGtImage img[VKN_GT_MAX_IMAGES]; };
struct GtTable { int label[VKN_GT_MAX_CLASSES]; };
struct GtOffsets { int key[VKN_GT_MAX_IMAGES + 1], ref[VKN_GT_MAX_IMAGES + 1]; };

// ------------------------------------------------------------------------------------------------------------ class presence
__device__ __forceinline__ void gp_mark(unsigned* bits, int v, int& last) {
    if (v != last) {               // semantic maps are piecewise constant: most pixels repeat their left neighbour
        atomicOr(&bits[v >> 5], 1u << (v & 31));
        last = v;
    }
}

// grid (ceil(Hp / GP_ROWS), B).  Rows >= valid_h and columns >= valid_w are not read at all.
template <bool I64>
__global__ __launch_bounds__(GT_THREADS) void k_gt_presence(GtBatch batch, int Wp, unsigned* __restrict__ flags, int* __restrict__ status) {
    __shared__ unsigned bits[8];
    const VknGtImage& im = batch.img[blockIdx.y];
    const int tid = threadIdx.x;
    if (tid < 8) bits[tid] = 0u;
    __syncthreads();
    const int y0 = blockIdx.x * GP_ROWS;
    const int y1 = min(y0 + GP_ROWS, im.valid_h);
    const int vw = im.valid_w;
    int last = -1;
    bool bad = false;
    if (I64) {
        const long long* sem = static_cast<const long long*>(im.sem);
        for (int y = y0; y < y1; ++y) {
            const long long* row = sem + (size_t)y * Wp;
            for (int x = tid; x < vw; x += GT_THREADS) {
                const long long v = row[x];
                if (v < 0 || v > 255) bad = true;
                else gp_mark(bits, (int)v, last);
            }
        }
    } else {
        const unsigned char* sem = static_cast<const unsigned char*>(im.sem);
        const bool vec = (Wp & 15) == 0 && (reinterpret_cast<uintptr_t>(sem) & 15) == 0;
        for (int y = y0; y < y1; ++y) {
            const unsigned char* row = sem + (size_t)y * Wp;
            if (vec) {
                for (int x = tid * 16; x < vw; x += GT_THREADS * 16) {
                    if (x + 16 <= vw) {
                        const uint4 q = *reinterpret_cast<const uint4*>(row + x);
                        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) gp_mark(bits, (int)((w[i] >> (8 * j)) & 255u), last);
                    } else {
                        for (int i = x; i < vw; ++i) gp_mark(bits, (int)row[i], last);
                    }
                }
            } else {
                for (int x = tid; x < vw; x += GT_THREADS) gp_mark(bits, (int)row[x], last);
            }
        }
    }
    if (I64 && bad) atomicOr(status, (int)VKN_STATUS_RANGE);
    __syncthreads();
    if (tid < 8 && bits[tid]) atomicOr(&flags[blockIdx.y * 8 + tid], bits[tid]);
}

// grid (B), 256 threads: thread c owns class c.  Ascending compaction: ballots inside the wave, the four wave counts through LDS.
__global__ __launch_bounds__(GT_THREADS) void k_gt_finish(GtTable tab, const unsigned* __restrict__ flags, int* __restrict__ n_sem,
                                                          unsigned char* __restrict__ classes, long long* __restrict__ labels) {
    __shared__ int cnt[GT_THREADS / 64];
    const int b = blockIdx.x, c = threadIdx.x, wave = c >> 6, lane = c & 63;
    const int label = tab.label[c];
    const bool on = ((flags[b * 8 + (c >> 5)] >> (c & 31)) & 1u) && label >= 0;
    const unsigned long long m = __ballot(on);
    if (lane == 0) cnt[wave] = __popcll(m);
    __syncthreads();
    int pos = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += cnt[w];
    if (on) {
        classes[b * VKN_GT_MAX_CLASSES + pos] = (unsigned char)c;
        labels[b * VKN_GT_MAX_CLASSES + pos] = label;
    }
    if (c == 0) n_sem[b] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// ----------------------------------------------------------------------------------------------------------------- bank fill
// The centre pixels of 4 neighbouring s x s cells: NR x NC per cell (2 x 2; 1 x 1 at s = 1, the identity).
template <int S>
struct Geo {
    static constexpr int NR = S == 1 ? 1 : 2, NC = NR, OFF = S == 1 ? 0 : S / 2 - 1;
    static constexpr float SCALE = S == 1 ? 1.f : 0.25f;
};

// v[r][k][c] = plane[S oy + OFF + r][S (ox + k) + OFF + c], `fill` at rows >= hlim / columns >= wlim (hlim <= rows of the plane,
// wlim <= pitch).  vec: the plane is 16-byte aligned and pitch % (4 S) == 0, so the 4 S bytes at column S ox (ox % 4 == 0) are aligned.
template <int S>
__device__ __forceinline__ void gt_load_u8(const unsigned char* __restrict__ plane, int pitch, int hlim, int wlim, bool vec, int oy, int ox,
                                           int fill, int (&v)[Geo<S>::NR][4][Geo<S>::NC]) {
    using G = Geo<S>;
    const int x0 = S * ox;
#pragma unroll
    for (int r = 0; r < G::NR; ++r) {
        const int y = S * oy + G::OFF + r;
        if (y >= hlim) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < G::NC; ++c) v[r][k][c] = fill;
            continue;
        }
        const unsigned char* row = plane + (size_t)y * pitch;
        if (vec && x0 + 4 * S <= wlim) {
            unsigned w[S];                      // 4 S bytes
            if constexpr (S == 1) {
                w[0] = *reinterpret_cast<const unsigned*>(row + x0);
            } else if constexpr (S == 2) {
                const uint2 q = *reinterpret_cast<const uint2*>(row + x0);
                w[0] = q.x; w[1] = q.y;
            } else {
#pragma unroll
                for (int i = 0; i < S / 4; ++i) {
                    const uint4 q = *reinterpret_cast<const uint4*>(row + x0 + 16 * i);
                    w[4 * i] = q.x; w[4 * i + 1] = q.y; w[4 * i + 2] = q.z; w[4 * i + 3] = q.w;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < G::NC; ++c) {
                    const int byte = k * S + G::OFF + c;           // compile-time after unrolling
                    v[r][k][c] = (int)((w[byte >> 2] >> (8 * (byte & 3))) & 255u);
                }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < G::NC; ++c) {
                    const int x = x0 + k * S + G::OFF + c;
                    v[r][k][c] = x < wlim ? (int)row[x] : fill;
                }
        }
    }
}

template <int S>
__device__ __forceinline__ void gt_load_i64(const long long* __restrict__ plane, int pitch, int hlim, int wlim, int oy, int ox, int fill,
                                            int (&v)[Geo<S>::NR][4][Geo<S>::NC]) {
    using G = Geo<S>;
#pragma unroll
    for (int r = 0; r < G::NR; ++r) {
        const int y = S * oy + G::OFF + r;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < G::NC; ++c) {
                const int x = S * (ox + k) + G::OFF + c;
                int val = fill;
                if (y < hlim && x < wlim) {
                    const long long q = plane[(size_t)y * pitch + x];
                    if (q >= 0 && q <= 255) val = (int)q;
                }
                v[r][k][c] = val;
            }
    }
}

// 4 outputs at bank element `e` (columns ox .. ox + 3 of an output row of width aW): 16 bytes when the address allows
__device__ __forceinline__ void gt_store4(float* __restrict__ bank, size_t e, int ox, int aW, const float (&o)[4]) {
    if (ox + 4 <= aW && (e & 3) == 0) {
        *reinterpret_cast<float4*>(bank + e) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ox + k < aW) bank[e + k] = o[k];
    }
}

// grid (ceil(aW / GT_COLS), ceil(aH / GT_ROWS), units): a unit is one thing row, or ALL stuff rows of an image (n_sem > 0).
template <int S, bool I64>
__global__ __launch_bounds__(GT_THREADS) void k_gt_fill(GtBatch batch, int B, int Hp, int Wp, float* __restrict__ bank) {
    using G = Geo<S>;
    int u = blockIdx.z, b = 0;
    for (; b < B - 1; ++b) {                                   // wave-uniform: scalar reads of the kernel arguments
        const int n = batch.img[b].G + (batch.img[b].n_sem > 0 ? 1 : 0);
        if (u < n) break;
        u -= n;
    }
    const VknGtImage& im = batch.img[b];
    const int aH = Hp / S, aW = Wp / S;                        // once per thread
    const int oy = blockIdx.y * GT_ROWS + (threadIdx.x >> 6);
    const int ox = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    if (oy >= aH || ox >= aW) return;
    int v[G::NR][4][G::NC];
    float o[4];
    if (u < im.G) {
        const unsigned char* plane = im.masks + (size_t)u * im.Hm * im.Wm;
        const bool vec = (im.Wm % (4 * S)) == 0 && (reinterpret_cast<uintptr_t>(im.masks) & 15) == 0;
        gt_load_u8<S>(plane, im.Wm, im.Hm, im.Wm, vec, oy, ox, 0, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int sum = 0;
#pragma unroll
            for (int r = 0; r < G::NR; ++r)
#pragma unroll
                for (int c = 0; c < G::NC; ++c) sum += v[r][k][c];
            o[k] = (float)sum * G::SCALE;
        }
        gt_store4(bank, ((size_t)(im.row0 + u) * aH + oy) * aW + ox, ox, aW, o);
        return;
    }
    if (I64) {
        gt_load_i64<S>(static_cast<const long long*>(im.sem), Wp, im.valid_h, im.valid_w, oy, ox, -1, v);
    } else {
        const bool vec = (Wp % (4 * S)) == 0 && (reinterpret_cast<uintptr_t>(im.sem) & 15) == 0;
        gt_load_u8<S>(static_cast<const unsigned char*>(im.sem), Wp, im.valid_h, im.valid_w, vec, oy, ox, -1, v);
    }
    const size_t plane = (size_t)aH * aW;
    size_t e = ((size_t)im.sem_row0 * aH + oy) * aW + ox;
    for (int j = 0; j < im.n_sem; ++j, e += plane) {
        const int cls = im.classes[j];                         // uniform: a scalar load
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int n = 0;
#pragma unroll
            for (int r = 0; r < G::NR; ++r)
#pragma unroll
                for (int c = 0; c < G::NC; ++c) n += v[r][k][c] == cls ? 1 : 0;
            o[k] = (float)n * G::SCALE;
        }
        gt_store4(bank, e, ox, aW, o);
    }
}

template <int S>
void gt_launch_fill(bool i64, dim3 grid, hipStream_t st, const GtBatch& batch, int B, int Hp, int Wp, float* bank) {
    if (i64) hipLaunchKernelGGL((k_gt_fill<S, true>), grid, dim3(GT_THREADS), 0, st, batch, B, Hp, Wp, bank);
    else hipLaunchKernelGGL((k_gt_fill<S, false>), grid, dim3(GT_THREADS), 0, st, batch, B, Hp, Wp, bank);
}

// ------------------------------------------------------------------------------------------------------------ match indices
// grid (B): the image's reference ids in LDS, one key id per thread and pass, a linear scan that stops at the first hit.
__global__ __launch_bounds__(GT_THREADS) void k_gt_match(const long long* __restrict__ key_ids, const long long* __restrict__ ref_ids,
                                                         GtOffsets off, int B, long long* __restrict__ match,
                                                         long long* __restrict__ match_off) {
    __shared__ long long ref[VKN_GT_MAX_IDS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int k0 = off.key[b], nk = off.key[b + 1] - k0, r0 = off.ref[b], nr = off.ref[b + 1] - r0;
    for (int i = tid; i < nr; i += GT_THREADS) ref[i] = ref_ids[r0 + i];
    if (tid == 0) {
        match_off[b] = k0;
        if (b == B - 1) match_off[B] = off.key[B];
    }
    __syncthreads();
    for (int k = tid; k < nk; k += GT_THREADS) {
        const long long id = key_ids[k0 + k];
        int hit = -1;
        for (int r = 0; r < nr; ++r)
            if (ref[r] == id) {
                hit = r;
                break;
            }
        match[k0 + k] = hit;
    }
}

inline int gt_check_batch(const VknGtImage* imgs, int B) {
    if (!imgs || B < 0) return VKN_E_ARG;
    return VKN_OK;
}

}  // namespace

extern "C" {

size_t vkn_sizeof_gt_image(void) { return sizeof(VknGtImage); }

int vkn_gt_classes(const VknGtImage* imgs, int B, int Hp, int Wp, int sem_i64, const int* label_of_class, unsigned* flags, int* n_sem,
                   unsigned char* classes, int64_t* labels, int* status, void* stream) {
    if (gt_check_batch(imgs, B) != VKN_OK || !label_of_class || !flags || !n_sem || !classes || !labels || !status) return VKN_E_ARG;
    if (B < 1 || B > VKN_GT_MAX_IMAGES) return VKN_E_SHAPE;
    for (int b = 0; b < B; ++b)
        if (!imgs[b].sem) return VKN_E_ARG;
    if (Hp < 1 || Wp < 1 || (long long)Hp * Wp >= (1ll << 31) || Hp > GP_ROWS * 65535) return VKN_E_SHAPE;   // grid.x of the presence pass
    for (int b = 0; b < B; ++b)
        if (imgs[b].valid_h < 0 || imgs[b].valid_h > Hp || imgs[b].valid_w < 0 || imgs[b].valid_w > Wp) return VKN_E_SHAPE;
    if (!vkn_aligned(flags, 4) || !vkn_aligned(n_sem, 4) || !vkn_aligned(labels, 8) || !vkn_aligned(status, 4)) return VKN_E_ALIGN;
    for (int b = 0; b < B; ++b)
        if (sem_i64 && !vkn_aligned(imgs[b].sem, 8)) return VKN_E_ALIGN;
    const void* ptrs[] = {flags, n_sem, classes, labels, status};
    for (const void* p : ptrs)
        if (!vkn_on_device(p)) return VKN_E_ARG;
    GtBatch batch = {};
    for (int b = 0; b < B; ++b) {
        if (!vkn_on_device(imgs[b].sem)) return VKN_E_ARG;
        batch.img[b] = imgs[b];
    }
    GtTable tab;
    for (int c = 0; c < VKN_GT_MAX_CLASSES; ++c) tab.label[c] = label_of_class[c];

    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(flags, 0, (size_t)B * 8 * sizeof(unsigned), st) != hipSuccess) return VKN_E_LAUNCH;
    const dim3 grid((Hp + GP_ROWS - 1) / GP_ROWS, B);
    if (sem_i64) hipLaunchKernelGGL(k_gt_presence<true>, grid, dim3(GT_THREADS), 0, st, batch, Wp, flags, status);
    else hipLaunchKernelGGL(k_gt_presence<false>, grid, dim3(GT_THREADS), 0, st, batch, Wp, flags, status);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gt_finish, dim3(B), dim3(GT_THREADS), 0, st, tab, flags, n_sem, classes, reinterpret_cast<long long*>(labels));
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

int vkn_gt_bank_fill_f32(const VknGtImage* imgs, int B, int Hp, int Wp, int s, int sem_i64, float* bank, int G_total, void* stream) {
    if (gt_check_batch(imgs, B) != VKN_OK || !bank) return VKN_E_ARG;
    if (B < 1 || B > VKN_GT_MAX_IMAGES) return VKN_E_SHAPE;
    for (int b = 0; b < B; ++b) {
        const VknGtImage& im = imgs[b];
        if (im.G < 0 || im.n_sem < 0) return VKN_E_ARG;
        if ((im.G > 0 && !im.masks) || (im.n_sem > 0 && (!im.sem || !im.classes))) return VKN_E_ARG;
    }
    if (!(s == 1 || s == 2 || s == 4 || s == 8) || Hp < 1 || Wp < 1 || Hp % s != 0 || Wp % s != 0 || G_total < 1) return VKN_E_SHAPE;
    if ((long long)Hp * Wp >= (1ll << 31)) return VKN_E_SHAPE;
    const int aH = Hp / s, aW = Wp / s;
    if ((long long)G_total * aH * aW * 4 >= (1ll << 31)) return VKN_E_SHAPE;
    if (aH > GT_ROWS * 65535) return VKN_E_SHAPE;            // grid.y of the fill
    long long units = 0;
    for (int b = 0; b < B; ++b) {
        const VknGtImage& im = imgs[b];
        if (im.n_sem > VKN_GT_MAX_CLASSES) return VKN_E_SHAPE;
        if (im.G > 0 && (im.Hm < 1 || im.Wm < 1 || im.Hm > Hp || im.Wm > Wp)) return VKN_E_SHAPE;
        if (im.valid_h < 0 || im.valid_h > Hp || im.valid_w < 0 || im.valid_w > Wp) return VKN_E_SHAPE;
        if (im.G > 0 && (im.row0 < 0 || (long long)im.row0 + im.G > G_total)) return VKN_E_SHAPE;
        if (im.n_sem > 0 && (im.sem_row0 < 0 || (long long)im.sem_row0 + im.n_sem > G_total)) return VKN_E_SHAPE;
        units += im.G + (im.n_sem > 0 ? 1 : 0);
    }
    if (units > 65535) return VKN_E_SHAPE;
    if (!vkn_aligned(bank, 16)) return VKN_E_ALIGN;
    for (int b = 0; b < B; ++b)
        if (sem_i64 && imgs[b].n_sem > 0 && !vkn_aligned(imgs[b].sem, 8)) return VKN_E_ALIGN;
    if (!vkn_on_device(bank)) return VKN_E_ARG;
    GtBatch batch = {};
    for (int b = 0; b < B; ++b) {
        const VknGtImage& im = imgs[b];
        if ((im.G > 0 && !vkn_on_device(im.masks)) || (im.n_sem > 0 && (!vkn_on_device(im.sem) || !vkn_on_device(im.classes)))) return VKN_E_ARG;
        batch.img[b] = im;
    }
    if (units == 0) return VKN_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((aW + GT_COLS - 1) / GT_COLS, (aH + GT_ROWS - 1) / GT_ROWS, (unsigned)units);
    const bool i64 = sem_i64 != 0;
    switch (s) {
        case 1: gt_launch_fill<1>(i64, grid, st, batch, B, Hp, Wp, bank); break;
        case 2: gt_launch_fill<2>(i64, grid, st, batch, B, Hp, Wp, bank); break;
        case 4: gt_launch_fill<4>(i64, grid, st, batch, B, Hp, Wp, bank); break;
        default: gt_launch_fill<8>(i64, grid, st, batch, B, Hp, Wp, bank); break;
    }
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

int vkn_gt_match_indices(const int64_t* key_ids, const int* key_len, const int64_t* ref_ids, const int* ref_len, int B, int64_t* match,
                         int64_t* match_off, void* stream) {
    if (!key_len || !ref_len || !match_off || B < 0) return VKN_E_ARG;
    if (B < 1 || B > VKN_GT_MAX_IMAGES) return VKN_E_SHAPE;
    GtOffsets off = {};
    for (int b = 0; b < B; ++b) {
        if (key_len[b] < 0 || ref_len[b] < 0) return VKN_E_ARG;
        if (key_len[b] > VKN_GT_MAX_IDS || ref_len[b] > VKN_GT_MAX_IDS) return VKN_E_SHAPE;
        off.key[b + 1] = off.key[b] + key_len[b];
        off.ref[b + 1] = off.ref[b] + ref_len[b];
    }
    if ((off.key[B] > 0 && (!key_ids || !match)) || (off.ref[B] > 0 && !ref_ids)) return VKN_E_ARG;
    if (!vkn_aligned(key_ids, 8) || !vkn_aligned(ref_ids, 8) || !vkn_aligned(match, 8) || !vkn_aligned(match_off, 8)) return VKN_E_ALIGN;
    if (!vkn_on_device(match_off) || (off.key[B] > 0 && (!vkn_on_device(key_ids) || !vkn_on_device(match))) ||
        (off.ref[B] > 0 && !vkn_on_device(ref_ids)))
        return VKN_E_ARG;

    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_gt_match, dim3(B), dim3(GT_THREADS), 0, st, reinterpret_cast<const long long*>(key_ids),
                       reinterpret_cast<const long long*>(ref_ids), off, B, reinterpret_cast<long long*>(match),
                       reinterpret_cast<long long*>(match_off));
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

}  // extern "C"
