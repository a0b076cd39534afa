// vkn_tracktail.hip — the video detector's tracking tail on the device: what `simple_test` does between the panoptic merge and the
// two maps it returns (knet/video/knet_quansi_dense_embed_fc_joint_train.py:536-603 with the helpers :673-685, :698-736).
//
//   vkn_track_boxes_f32   the accepted thing entries of `info` in segment order (`get_things_id_for_tracking`, :673-685), the
//                         semantic filter (:546-553) and `tensor_mask2box` of `(panoptic_seg == id) * semantic_thing` (:567, :583)
//   vkn_track_maps_i32    `generate_track_id_maps` (:724-736, with the `ids + 1` of :591-592) and `get_semantic_seg` (:698-722)
//
// Both read the panoptic map once.  Per-segment results are per-frame tables indexed by segment id (<= K entries), staged in LDS:
// the box pass keeps (min, max) per compact slot in LDS through integer atomics and publishes the non-empty ones with global
// integer atomicMin / atomicMax (order-independent: the result is deterministic); the map pass is out[p] = lut[panoptic_seg[p]].
// Floating-point contraction is OFF: the bilinear interpolation of the semantic logits is the sequence of individually rounded
// fp32 operations of ATen's upsample_bilinear2d (align_corners=False).
#include "../../include/vkn_track.h"
#include "vkn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TT_MAX_K = VKN_TRACK_MAX_K;   // entries per frame (LDS tables)
constexpr int TT_TW = 64, TT_TH = 16;       // map tile of one workgroup of the box pass: 256 threads x 4 pixels of one row
constexpr int TT_EMPTY_MIN = 0x7fffffff;

inline size_t tt_pad(size_t n) { return (n + 255) & ~(size_t)255; }
// boxes workspace: slot_of [B][K + 1] (segment id -> compact slot or -1), box [B][K][4] (xmin, ymin, xmax, ymax)
inline size_t tt_boxes_ws(int B, int K) { return tt_pad((size_t)B * (K + 1) * 4) + tt_pad((size_t)B * K * 16); }
// maps workspace: lut [B][2][K + 1] (track id, semantic class) by segment id
inline size_t tt_maps_ws(int B, int K) { return tt_pad((size_t)B * 2 * (K + 1) * 4); }

// ------------------------------------------------------------------------------------------------ entries of one frame
// One workgroup per frame.  Entry i of `info` is kept when it is an accepted thing: 0 < segment id <= min(nseg, K) and joint label
// < T.  Its slot is the number of kept entries with a smaller segment id (segment ids are distinct; of a repeated id only the first
// entry is kept): ascending segment order, slots 0 .. count - 1 all written.
__global__ __launch_bounds__(256) void k_tt_entries(const int* __restrict__ info, const int* __restrict__ nseg, int K, int T,
                                                    float* __restrict__ det, long long* __restrict__ labels, int* __restrict__ rows,
                                                    int* __restrict__ segid, int* __restrict__ count, int* __restrict__ slot_of,
                                                    int* __restrict__ box) {
    __shared__ int s_sid[TT_MAX_K];   // segment id of a kept entry, 0 otherwise
    __shared__ int s_slot[TT_MAX_K + 1];   // segment id -> slot, -1: not a kept thing
    __shared__ int s_count;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int* inf = info + (size_t)b * K * VKN_PANOPTIC_INFO_FIELDS;
    int ns = nseg[b];
    ns = ns < 0 ? 0 : (ns > K ? K : ns);
    if (tid == 0) s_count = 0;
    for (int i = tid; i <= K; i += 256) s_slot[i] = -1;
    for (int i = tid; i < K; i += 256) {
        const int sid = inf[i * VKN_PANOPTIC_INFO_FIELDS + 2], lab = inf[i * VKN_PANOPTIC_INFO_FIELDS + 1];
        s_sid[i] = (sid > 0 && sid <= ns && lab >= 0 && lab < T) ? sid : 0;
    }
    for (int i = tid; i < K; i += 256) {
        const size_t r = (size_t)b * K + i;
        box[r * 4] = TT_EMPTY_MIN; box[r * 4 + 1] = TT_EMPTY_MIN; box[r * 4 + 2] = -1; box[r * 4 + 3] = -1;
    }
    __syncthreads();
    // vkn_panoptic_joint_f32 hands out every segment id once; should a malformed `info` repeat one, its first entry is the entry
    {
        bool dup[(TT_MAX_K + 255) / 256];
        int q = 0;
        for (int i = tid; i < K; i += 256, ++q) {
            const int sid = s_sid[i];
            bool d = false;
            for (int j = 0; j < i && sid > 0; ++j) d |= s_sid[j] == sid;
            dup[q] = d;
        }
        __syncthreads();
        q = 0;
        for (int i = tid; i < K; i += 256, ++q)
            if (dup[q]) s_sid[i] = 0;
    }
    __syncthreads();
    for (int i = tid; i < K; i += 256) {
        const int sid = s_sid[i];
        if (sid == 0) continue;
        int slot = 0;
        for (int j = 0; j < K; ++j) {
            const int sj = s_sid[j];
            slot += (sj > 0 && sj < sid);
        }
        const size_t r = (size_t)b * K + slot;
        det[r * 5 + 4] = __int_as_float(inf[i * VKN_PANOPTIC_INFO_FIELDS + 5]);
        labels[r] = inf[i * VKN_PANOPTIC_INFO_FIELDS + 1];
        rows[r] = inf[i * VKN_PANOPTIC_INFO_FIELDS];
        segid[r] = sid;
        s_slot[sid] = slot;
        atomicAdd(&s_count, 1);
    }
    __syncthreads();
    const int n = s_count;
    if (tid == 0) count[b] = n;
    for (int i = tid; i <= K; i += 256) slot_of[(size_t)b * (K + 1) + i] = s_slot[i];
    for (int i = n + tid; i < K; i += 256) {   // rows beyond count are zero
        const size_t r = (size_t)b * K + i;
        for (int e = 0; e < 5; ++e) det[r * 5 + e] = 0.f;
        labels[r] = 0;
        rows[r] = 0;
        segid[r] = 0;
    }
}

// ------------------------------------------------------------------------------------------------ semantic filter
struct TtSem {
    const float* logits;   // [B][Cs][hs][ws] or NULL
    int Cs, hs, ws, T;
    float sy, sx;          // ATen's area_pixel_compute_scale<float>(in, out, align_corners=False): (float)in / (float)out
};

// ATen's source index of output index d (upsample_bilinear2d, align_corners=False): max(scale * (d + 0.5) - 0.5, 0)
__device__ __forceinline__ void tt_src(int d, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
    float s = scale * ((float)d + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - (float)i0;
    l0 = 1.f - l1;
}

// semantic_thing of pixel (y, x) of frame b: arg-max channel of the interpolated logits (first maximum) < T
__device__ __forceinline__ bool tt_semantic_thing(const TtSem& s, int b, int y0, int y1, float ly0, float ly1, int x) {
    int x0, x1;
    float lx0, lx1;
    tt_src(x, s.sx, s.ws, x0, x1, lx0, lx1);
    const size_t plane = (size_t)s.hs * s.ws;
    const float* p = s.logits + (size_t)b * s.Cs * plane;
    const size_t o00 = (size_t)y0 * s.ws + x0, o01 = (size_t)y0 * s.ws + x1, o10 = (size_t)y1 * s.ws + x0, o11 = (size_t)y1 * s.ws + x1;
    float best = ly0 * (lx0 * p[o00] + lx1 * p[o01]) + ly1 * (lx0 * p[o10] + lx1 * p[o11]);
    int arg = 0;
    for (int c = 1; c < s.Cs; ++c) {
        p += plane;
        const float v = ly0 * (lx0 * p[o00] + lx1 * p[o01]) + ly1 * (lx0 * p[o10] + lx1 * p[o11]);
        if (v > best) {   // strictly greater: ties stay with the lowest channel
            best = v;
            arg = c;
        }
    }
    return arg < s.T;
}

// ------------------------------------------------------------------------------------------------ boxes
// grid (tiles x, tiles y, B), 256 threads: thread t owns 4 consecutive pixels of row (t >> 4) of the tile.
// VEC: Wo % 4 == 0, so every group of 4 is inside the row and 16-byte aligned (int4 load, one 32-bit store of the mask bytes).
template <bool VEC>
__global__ __launch_bounds__(256) void k_tt_boxes(const int* __restrict__ seg, const int* __restrict__ slot_of, TtSem sem, int K, int Ho,
                                                  int Wo, int* __restrict__ box, unsigned char* __restrict__ thing_mask) {
    __shared__ int s_slot[TT_MAX_K + 1];
    __shared__ int s_box[TT_MAX_K * 4];
    const int b = blockIdx.z, tid = threadIdx.x;
    for (int i = tid; i <= K; i += 256) s_slot[i] = slot_of[(size_t)b * (K + 1) + i];
    for (int i = tid; i < K; i += 256) {
        s_box[4 * i] = TT_EMPTY_MIN; s_box[4 * i + 1] = TT_EMPTY_MIN; s_box[4 * i + 2] = -1; s_box[4 * i + 3] = -1;
    }
    __syncthreads();
    const int y = blockIdx.y * TT_TH + (tid >> 4), x4 = blockIdx.x * TT_TW + (tid & 15) * 4;
    if (y < Ho && x4 < Wo) {
        const size_t base = ((size_t)b * Ho + y) * Wo + x4;
        int id[4] = {0, 0, 0, 0};
        const int nx = Wo - x4 < 4 ? Wo - x4 : 4;
        if (VEC) {
            const int4 v = *reinterpret_cast<const int4*>(seg + base);
            id[0] = v.x; id[1] = v.y; id[2] = v.z; id[3] = v.w;
        } else {
            for (int e = 0; e < nx; ++e) id[e] = seg[base + e];
        }
        int slot[4];
        bool any = false;
        for (int e = 0; e < 4; ++e) {
            slot[e] = (e < nx && id[e] > 0 && id[e] <= K) ? s_slot[id[e]] : -1;
            any |= slot[e] >= 0;
        }
        unsigned char m[4] = {1, 1, 1, 1};
        if (sem.logits && (any || thing_mask)) {   // the filter is evaluated for thing-segment pixels only (everywhere for thing_mask)
            int y0, y1;
            float ly0, ly1;
            tt_src(y, sem.sy, sem.hs, y0, y1, ly0, ly1);
            for (int e = 0; e < nx; ++e)
                if (slot[e] >= 0 || thing_mask) m[e] = tt_semantic_thing(sem, b, y0, y1, ly0, ly1, x4 + e) ? 1 : 0;
        }
        if (thing_mask) {
            if (VEC) {
                *reinterpret_cast<uchar4*>(thing_mask + base) = make_uchar4(m[0], m[1], m[2], m[3]);
            } else {
                for (int e = 0; e < nx; ++e) thing_mask[base + e] = m[e];
            }
        }
        // runs of one slot inside the 4 pixels share their atomics
        int cur = -1, lo = 0, hi = 0;
        for (int e = 0; e <= 4; ++e) {
            const int s = (e < 4 && m[e]) ? slot[e] : -1;
            if (s != cur) {
                if (cur >= 0) {
                    atomicMin(&s_box[4 * cur], lo); atomicMin(&s_box[4 * cur + 1], y);
                    atomicMax(&s_box[4 * cur + 2], hi); atomicMax(&s_box[4 * cur + 3], y);
                }
                cur = s;
                lo = x4 + e;
            }
            hi = x4 + e;
        }
    }
    __syncthreads();
    int* gb = box + (size_t)b * K * 4;
    for (int i = tid; i < K; i += 256)
        if (s_box[4 * i + 2] >= 0) {
            atomicMin(&gb[4 * i], s_box[4 * i]); atomicMin(&gb[4 * i + 1], s_box[4 * i + 1]);
            atomicMax(&gb[4 * i + 2], s_box[4 * i + 2]); atomicMax(&gb[4 * i + 3], s_box[4 * i + 3]);
        }
}

// det[b][slot][0..3] of the kept rows: the box as floats, unitrack's (-1, -1, 10, 10) for a segment the filter emptied
__global__ __launch_bounds__(256) void k_tt_finish(const int* __restrict__ box, const int* __restrict__ count, int K, float* __restrict__ det) {
    const int b = blockIdx.x;
    const int n = count[b];
    for (int i = threadIdx.x; i < n && i < K; i += 256) {
        const int* bb = box + ((size_t)b * K + i) * 4;
        float* d = det + ((size_t)b * K + i) * 5;
        const bool empty = bb[2] < 0;
        d[0] = empty ? -1.f : (float)bb[0]; d[1] = empty ? -1.f : (float)bb[1];
        d[2] = empty ? 10.f : (float)bb[2]; d[3] = empty ? 10.f : (float)bb[3];
    }
}

// ------------------------------------------------------------------------------------------------ maps
// One workgroup per frame: lut[0][sid] = track id + 1 of thing segment sid (0: none), lut[1][sid] = semantic class of segment sid.
__global__ __launch_bounds__(256) void k_tt_luts(const int* __restrict__ segid, const int* __restrict__ count, const long long* __restrict__ ids,
                                                 const int* __restrict__ n_ids, int max_dets, const int* __restrict__ info,
                                                 const int* __restrict__ sem_of_label, int num_labels, int K, int* __restrict__ lut) {
    const int b = blockIdx.x, tid = threadIdx.x;
    int* lt = lut + (size_t)b * 2 * (K + 1);
    int* ls = lt + (K + 1);
    for (int i = tid; i <= K; i += 256) { lt[i] = 0; ls[i] = 0; }
    __syncthreads();
    // the tracker's i-th returned row is paired with the i-th thing segment (generate_track_id_maps :732-734)
    int n = count[b];
    const int ni = n_ids[b];
    n = n < ni ? n : ni;
    n = n < max_dets ? n : max_dets;
    n = n < K ? n : K;
    for (int i = tid; i < n; i += 256) {
        const int sid = segid[(size_t)b * K + i];
        long long v = ids[(size_t)b * max_dets + i] + 1;   // :591
        if (v == -1) v = 0;                                  // :592
        if (sid > 0 && sid <= K) lt[sid] = (int)v;
    }
    const int* inf = info + (size_t)b * K * VKN_PANOPTIC_INFO_FIELDS;
    for (int i = tid; i < K; i += 256) {
        const int sid = inf[i * VKN_PANOPTIC_INFO_FIELDS + 2], lab = inf[i * VKN_PANOPTIC_INFO_FIELDS + 1];
        if (sid > 0 && sid <= K && lab >= 0 && lab < num_labels) ls[sid] = sem_of_label[lab];
    }
}

// out[p] = lut[panoptic_seg[p]] for both maps.  VEC: Ho * Wo % 4 == 0 (every frame starts 16-byte aligned).
template <bool VEC>
__global__ __launch_bounds__(256) void k_tt_maps(const int* __restrict__ seg, const int* __restrict__ lut, int K, size_t npx,
                                                 int* __restrict__ track_map, int* __restrict__ semantic_map) {
    __shared__ int s_lt[TT_MAX_K + 1], s_ls[TT_MAX_K + 1];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i <= K; i += 256) {
        s_lt[i] = lut[(size_t)b * 2 * (K + 1) + i];
        s_ls[i] = lut[(size_t)b * 2 * (K + 1) + (K + 1) + i];
    }
    __syncthreads();
    const int* s = seg + (size_t)b * npx;
    int* tm = track_map + (size_t)b * npx;
    int* sm = semantic_map + (size_t)b * npx;
    auto at = [&](int id) { return (id > 0 && id <= K) ? id : 0; };   // entry 0 of both tables is 0: void
    if (VEC) {
        const size_t nv = npx / 4;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
            const int4 v = reinterpret_cast<const int4*>(s)[i];
            const int a = at(v.x), c = at(v.y), d = at(v.z), e = at(v.w);
            reinterpret_cast<int4*>(tm)[i] = make_int4(s_lt[a], s_lt[c], s_lt[d], s_lt[e]);
            reinterpret_cast<int4*>(sm)[i] = make_int4(s_ls[a], s_ls[c], s_ls[d], s_ls[e]);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
            const int a = at(s[i]);
            tm[i] = s_lt[a];
            sm[i] = s_ls[a];
        }
    }
}

inline int tt_check_geometry(int B, int K, int Ho, int Wo) {
    if (B <= 0 || K <= 0 || Ho <= 0 || Wo <= 0) return VKN_E_ARG;
    if (K > TT_MAX_K) return VKN_E_SHAPE;
    if ((unsigned long long)Ho * (unsigned long long)Wo * 4ull >= (1ull << 31)) return VKN_E_SHAPE;
    if (B > 65535 || (Ho + TT_TH - 1) / TT_TH > 65535) return VKN_E_SHAPE;   // frames and tile rows ride on grid.y / grid.z
    return VKN_OK;
}

}  // namespace

extern "C" {

size_t vkn_track_boxes_workspace_bytes(int B, int K) {
    if (B <= 0 || K <= 0 || K > TT_MAX_K) return 0;
    return tt_boxes_ws(B, K);
}

size_t vkn_track_maps_workspace_bytes(int B, int K) {
    if (B <= 0 || K <= 0 || K > TT_MAX_K) return 0;
    return tt_maps_ws(B, K);
}

int vkn_track_boxes_f32(const int* panoptic_seg, const int* info, const int* nseg, const float* sem_logits, int Cs, int hs, int ws_w,
                        int num_thing_classes, int B, int K, int Ho, int Wo, float* det, int64_t* labels, int* rows, int* segid,
                        int* count, unsigned char* thing_mask, void* ws, size_t ws_bytes, void* stream) {
    if (!panoptic_seg || !info || !nseg || !det || !labels || !rows || !segid || !count || num_thing_classes < 0) return VKN_E_ARG;
    if (sem_logits && (Cs <= 0 || hs <= 0 || ws_w <= 0)) return VKN_E_ARG;
    const int rc = tt_check_geometry(B, K, Ho, Wo);
    if (rc != VKN_OK) return rc;
    if (sem_logits && (unsigned long long)Cs * hs * ws_w * 4ull >= (1ull << 31)) return VKN_E_SHAPE;
    const void* ptrs[] = {panoptic_seg, info, nseg, det, labels, rows, segid, count, sem_logits, thing_mask};
    for (const void* p : ptrs)
        if (p && !vkn_aligned(p, 16)) return VKN_E_ALIGN;
    if (!ws || ws_bytes < tt_boxes_ws(B, K) || !vkn_aligned(ws, 16)) return VKN_E_WORKSPACE;
    for (const void* p : ptrs)
        if (p && !vkn_on_device(p)) return VKN_E_ARG;
    if (!vkn_on_device(ws)) return VKN_E_ARG;

    hipStream_t st = static_cast<hipStream_t>(stream);
    int* slot_of = static_cast<int*>(ws);
    int* box = reinterpret_cast<int*>(static_cast<char*>(ws) + tt_pad((size_t)B * (K + 1) * 4));
    hipLaunchKernelGGL(k_tt_entries, dim3(B), dim3(256), 0, st, info, nseg, K, num_thing_classes, det, reinterpret_cast<long long*>(labels),
                       rows, segid, count, slot_of, box);
    VKN_CHECK_LAUNCH();
    TtSem sem{};
    sem.logits = sem_logits;
    sem.Cs = Cs; sem.hs = hs; sem.ws = ws_w; sem.T = num_thing_classes;
    if (sem_logits) {
        sem.sy = (float)hs / (float)Ho;
        sem.sx = (float)ws_w / (float)Wo;
    }
    const dim3 grid((Wo + TT_TW - 1) / TT_TW, (Ho + TT_TH - 1) / TT_TH, B);
    if (Wo % 4 == 0)
        hipLaunchKernelGGL(k_tt_boxes<true>, grid, dim3(256), 0, st, panoptic_seg, slot_of, sem, K, Ho, Wo, box, thing_mask);
    else
        hipLaunchKernelGGL(k_tt_boxes<false>, grid, dim3(256), 0, st, panoptic_seg, slot_of, sem, K, Ho, Wo, box, thing_mask);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_tt_finish, dim3(B), dim3(256), 0, st, box, count, K, det);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

int vkn_track_maps_i32(const int* panoptic_seg, const int* segid, const int* count, const int64_t* ids, const int* n_ids, int max_dets,
                       const int* info, const int* sem_of_label, int num_labels, int B, int K, int Ho, int Wo, int* track_map,
                       int* semantic_map, void* ws, size_t ws_bytes, void* stream) {
    if (!panoptic_seg || !segid || !count || !ids || !n_ids || !info || !sem_of_label || !track_map || !semantic_map || max_dets <= 0 ||
        num_labels <= 0)
        return VKN_E_ARG;
    const int rc = tt_check_geometry(B, K, Ho, Wo);
    if (rc != VKN_OK) return rc;
    // n_ids and sem_of_label are read as single ints (a tracker's out_count sits 8-byte aligned behind its ids): 4-byte aligned
    if ((reinterpret_cast<uintptr_t>(n_ids) & 3) || (reinterpret_cast<uintptr_t>(sem_of_label) & 3)) return VKN_E_ALIGN;
    const void* ptrs[] = {panoptic_seg, segid, count, ids, info, track_map, semantic_map};
    for (const void* p : ptrs)
        if (!vkn_aligned(p, 16)) return VKN_E_ALIGN;
    if (!ws || ws_bytes < tt_maps_ws(B, K) || !vkn_aligned(ws, 16)) return VKN_E_WORKSPACE;
    for (const void* p : ptrs)
        if (!vkn_on_device(p)) return VKN_E_ARG;
    if (!vkn_on_device(n_ids) || !vkn_on_device(sem_of_label) || !vkn_on_device(ws)) return VKN_E_ARG;

    hipStream_t st = static_cast<hipStream_t>(stream);
    int* lut = static_cast<int*>(ws);
    hipLaunchKernelGGL(k_tt_luts, dim3(B), dim3(256), 0, st, segid, count, reinterpret_cast<const long long*>(ids), n_ids, max_dets, info,
                       sem_of_label, num_labels, K, lut);
    VKN_CHECK_LAUNCH();
    const size_t npx = (size_t)Ho * Wo;
    size_t blocks = (npx / 4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    if (npx % 4 == 0)
        hipLaunchKernelGGL(k_tt_maps<true>, dim3((unsigned)blocks, B), dim3(256), 0, st, panoptic_seg, lut, K, npx, track_map, semantic_map);
    else
        hipLaunchKernelGGL(k_tt_maps<false>, dim3((unsigned)blocks, B), dim3(256), 0, st, panoptic_seg, lut, K, npx, track_map, semantic_map);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

}  // extern "C"
