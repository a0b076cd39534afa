// vkn_maskap.hip — COCO mask AP on the device (include/vkn_maskap.h): the pairwise overlap of K detections and G ground truths at full
// resolution as exact integers, and `COCOeval.evaluateImg` on those integers.
//
// Overlap.  Both sides are packed into bits by vkn_maskbits.h's k_rle_pack (the encoder's first pass): bits[n][strips][H], one 64-bit word
// per row of a strip of 64 columns, so the overlap of a detection's and a ground truth's row is popcount(d & g).  k_mask_overlap: a
// workgroup (one wave) owns a RUN of MO_RUN = 32 rows of one strip and MO_DT = 64 detections, one lane each; the lane keeps its detection's 32 words
// in a column of LDS that only it reads (held in registers, the fully unrolled tile made the scheduler hoist every LDS read and spill).
// The ground truths' words of the run are staged in LDS, MO_GC = 64 ground truths at a time, as gsh[row][gt]; a lane walks a
// register tile of MO_GT = 8 ground truths, reading their words of a row as ONE address for the whole wave (an LDS broadcast: 64 bytes in
// four 16-byte reads, no bank conflict), and adds __popcll(d & g) into eight 32-bit counters (at most 32 * 64 per run).  The counters of
// a chunk go through an LDS tile [detection][gt] and are flushed with 64-bit INTEGER atomics, ground truth fastest, so that a wave's adds
// fall on consecutive words of `inter` (one lane per table row was measured first: 1 M scattered adds, every line of the table hit by
// every workgroup, made the kernel as long as the pack).  Nonzero counters only: instance masks are local, so most (detection, ground
// truth, run) triples share no pixel, and a workgroup whose detections are all empty in the run skips the tiles.  Integer addition
// is order-free: two runs of the same input give the same bits (vkn_msda_bwd.hip relies on the same property).  Areas come from the same
// words: a detection's word is loaded by exactly one workgroup, a ground truth's by the workgroups of the first detection tile.
//
// Match.  k_ap_begin writes the K records' common fields, k_ap_match runs one wave per (category, area range) with a lane per IoU
// threshold, k_ap_end advances the record count: the hand-offs (the count that the first two read and the third writes) are kernel
// boundaries.  The work is small and sequential per threshold, like the device LSAP.
#include "../../include/vkn_maskap.h"
#include "../../include/vkn_instmask.h"   // vkn_bits_mask_overlap: the overlap with the detections already as bits
#include "vkn_common.h"
#include "vkn_maskbits.h"

namespace {

typedef unsigned long long u64;

constexpr int MO_RUN = VKN_MASKAP_ROW_RUN, MO_DT = VKN_MASKAP_DT_TILE, MO_GT = VKN_MASKAP_GT_TILE, MO_GC = VKN_MASKAP_GT_CHUNK;
static_assert(MO_DT % 64 == 0 && MO_GC % MO_GT == 0 && MO_GC == 64 && (MO_RUN * MO_GC) % MO_DT == 0 && MO_DT % MO_GC == 0 && MO_RUN % (MO_DT / MO_GC) == 0 && MO_RUN % 4 == 0,
              "a lane per detection; a staging thread keeps one ground truth");

__device__ __forceinline__ void add64(long long* p, u64 v) {
    __hip_atomic_fetch_add(reinterpret_cast<u64*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (strips * runs, ceil(K / MO_DT) or 1).  dbits [K][NS][H], gbits [G][NS][H].
__global__ __launch_bounds__(MO_DT) void k_mask_overlap(const u64* __restrict__ dbits, const u64* __restrict__ gbits, int K, int G, int H, long long NS,
                                                        long long runs, long long* __restrict__ inter, long long* __restrict__ area_dt,
                                                        long long* __restrict__ area_gt) {
    __shared__ __attribute__((aligned(16))) u64 gsh[MO_RUN][MO_GC];
    __shared__ u64 dsh[MO_RUN][MO_DT];
    __shared__ unsigned tsh[MO_DT][MO_GC + 1];                     // the chunk's counters [detection][gt]; + 1: a lane's row starts on its own bank
    const int tid = threadIdx.x;
    const long long s = blockIdx.x / runs, run = blockIdx.x % runs;
    const long long r0 = run * MO_RUN;
    const int nr = (int)min((long long)MO_RUN, (long long)H - r0);
    const int k = blockIdx.y * MO_DT + tid;
    const bool active = k < K;
    u64 any = 0;
    unsigned area = 0;
    {
        const u64* src = dbits + ((size_t)(active ? k : 0) * NS + s) * (size_t)H + r0;
        u64 w[MO_RUN];
#pragma unroll
        for (int r = 0; r < MO_RUN; ++r) w[r] = active && r < nr ? src[r] : 0ull;       // every load in flight before the first is used
#pragma unroll
        for (int r = 0; r < MO_RUN; ++r) {
            dsh[r][tid] = w[r];                                    // read back by this thread only: no barrier; rows behind the run are zero
            any |= w[r];
            area += (unsigned)__popcll(w[r]);
        }
    }
    if (area) add64(area_dt + k, area);
    const bool empty = __syncthreads_or(any != 0ull) == 0;         // no detection of the workgroup has a pixel in the run
    const int k0 = blockIdx.y * MO_DT, nk = min(MO_DT, K - k0);
    const int gl = tid % MO_GC, rw = tid / MO_GC;                  // staging: this thread's ground truth of the chunk, its first row
    for (int g0 = 0; g0 < G; g0 += MO_GC) {
        __syncthreads();
        {
            const int g = g0 + gl;
            const u64* src = gbits + ((size_t)(g < G ? g : 0) * NS + s) * (size_t)H + r0;
            unsigned ga = 0;
            constexpr int STEP = MO_DT / MO_GC, NW = MO_RUN / STEP;
            u64 w[NW];
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = g < G && rw + i * STEP < nr ? src[rw + i * STEP] : 0ull;
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                gsh[rw + i * STEP][gl] = w[i];
                ga += (unsigned)__popcll(w[i]);
            }
            if (blockIdx.y == 0 && ga) add64(area_gt + g, ga);
        }
        __syncthreads();
        if (empty) continue;
        const int ng = min(MO_GC, G - g0);
        for (int j0 = 0; j0 < ng; j0 += MO_GT) {
            unsigned acc[MO_GT];
#pragma unroll
            for (int j = 0; j < MO_GT; ++j) acc[j] = 0;
#pragma unroll 4
            for (int r = 0; r < MO_RUN; ++r) {                     // (the words of rows behind the run are zero on both sides)
                const u64 d = dsh[r][tid];
#pragma unroll
                for (int j = 0; j < MO_GT; ++j) acc[j] += (unsigned)__popcll(d & gsh[r][j0 + j]);
            }
#pragma unroll
            for (int j = 0; j < MO_GT; ++j) tsh[tid][j0 + j] = acc[j];
        }
        __syncthreads();
        // the flush, ground truth fastest: consecutive lanes add to consecutive words of `inter` (the whole block of the workgroup's
        // detections is contiguous when the chunk holds every ground truth), nonzero counters only
        for (int i = tid; i < nk * ng; i += MO_DT) {
            const int kk = i / ng, j = i - kk * ng;
            const unsigned v = tsh[kk][j];
            if (v) add64(inter + (size_t)(k0 + kk) * G + g0 + j, v);
        }
    }
}

inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

inline bool overlap_shape_ok(int K, int G, int H, int W, int elem) {
    if (K < 0 || K > VKN_MASKAP_MAX_MASKS || G < 0 || G > VKN_MASKAP_MAX_MASKS || H < 1 || W < 1) return false;
    const long long hw = (long long)H * W;
    return hw < (1ll << 31) && hw * K * elem < (1ll << 31) && hw * G < (1ll << 31);
}

struct OverlapLayout {
    size_t dbits, gbits, bytes;
    long long NS;
};
// own_dt: the workspace holds the detections as bits too (the u8 / f32 entries); false: the caller hands them in (vkn_bits_mask_overlap)
inline OverlapLayout overlap_layout(int K, int G, int H, int W, bool own_dt = true) {
    OverlapLayout l;
    l.NS = maskbits_strips(W);
    l.dbits = 0;
    l.gbits = own_dt ? up16((size_t)K * (size_t)l.NS * (size_t)H * 8) : 0;
    l.bytes = l.gbits + up16((size_t)G * (size_t)l.NS * (size_t)H * 8);
    return l;
}

// T: unsigned char / float detections that the call packs into its workspace, or u64: the detections as bits [K][NS][H]
template <typename T>
int mask_overlap(const T* dt, float thr, const unsigned char* gt, int K, int G, int H, int W, long long* inter, long long* area_dt, long long* area_gt,
                 void* ws, size_t ws_bytes, void* stream) {
    constexpr bool BITS = sizeof(T) == 8;
    if (K < 0 || G < 0 || H < 0 || W < 0) return VKN_E_ARG;
    const bool need_ws = BITS ? G > 0 : K + G > 0;      // the sides that the call packs
    if ((K > 0 && (!dt || !area_dt)) || (G > 0 && (!gt || !area_gt)) || (K > 0 && G > 0 && !inter) || (need_ws && !ws)) return VKN_E_ARG;
    if (!overlap_shape_ok(K, G, H, W, BITS ? 1 : (int)sizeof(T))) return VKN_E_SHAPE;
    const OverlapLayout l = overlap_layout(K, G, H, W, !BITS);
    if (ws_bytes != l.bytes) return VKN_E_WORKSPACE;
    const bool both = K > 0 && G > 0;
    if ((K > 0 && (!vkn_aligned(dt, 16) || !vkn_aligned(area_dt, 16))) || (G > 0 && (!vkn_aligned(gt, 16) || !vkn_aligned(area_gt, 16))) ||
        (both && !vkn_aligned(inter, 16)) || (need_ws && !vkn_aligned(ws, 16)))
        return VKN_E_ALIGN;
    if ((K > 0 && (!vkn_on_device(dt) || !vkn_on_device(area_dt))) || (G > 0 && (!vkn_on_device(gt) || !vkn_on_device(area_gt))) ||
        (both && !vkn_on_device(inter)) || (need_ws && !vkn_on_device(ws)))
        return VKN_E_ARG;
    if (K + G == 0) return VKN_OK;
    char* base = static_cast<char*>(ws);
    u64* gbits = reinterpret_cast<u64*>(base + l.gbits);      // (never read when G = 0)
    hipStream_t st = static_cast<hipStream_t>(stream);
    const u64* dbits;
    if constexpr (BITS) {
        dbits = dt;
    } else {
        u64* packed = reinterpret_cast<u64*>(base + l.dbits);
        if (K > 0 && !maskbits_pack<T>(dt, thr, K, H, W, packed, st)) return VKN_E_LAUNCH;
        dbits = packed;
    }
    if (G > 0 && !maskbits_pack<unsigned char>(gt, 0.f, G, H, W, gbits, st)) return VKN_E_LAUNCH;
    const long long runs = ((long long)H + MO_RUN - 1) / MO_RUN;
    const dim3 grid((unsigned)(l.NS * runs), (unsigned)(K > 0 ? (K + MO_DT - 1) / MO_DT : 1));
    hipLaunchKernelGGL(k_mask_overlap, grid, dim3(MO_DT), 0, st, dbits, gbits, K, G, H, l.NS, runs, inter, area_dt, area_gt);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

// ------------------------------------------------------------------------------------------------------------------------ match
constexpr int AP_MAX = VKN_MASKAP_MAX_MASKS;

struct ApArgs {
    unsigned* header;          // status, count
    long long* npig;
    int* log;
    const long long *inter, *area_dt, *area_gt;
    const float* scores;
    const int *dt_labels, *gt_labels;
    const unsigned char* gt_crowd;
    const double* gt_area;
    int* match_gt;
    int K, G, image;
};

// grid ceil(max(K, G, A * T * K) / 256): the records' common fields (rank -1, empty words), match_gt = -1, the label and score flags
__global__ __launch_bounds__(256) void k_ap_begin(const VknMaskApCfg cfg, const ApArgs a) {
    const unsigned base = a.header[1];
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
    unsigned flags = 0;
    for (long long k = i0; k < a.K; k += step) {
        const int label = a.dt_labels[k];
        const float score = a.scores[k];
        if (label < 0 || label >= cfg.num_classes) flags |= VKN_MASKAP_STATUS_LABEL_RANGE;
        if (score != score) flags |= VKN_MASKAP_STATUS_SCORE_NAN;
        const unsigned long long slot = (unsigned long long)base + (unsigned long long)k;
        if (slot < (unsigned long long)cfg.cap_records) {
            int* rec = a.log + slot * VKN_MASKAP_RECORD_INTS;
            rec[VKN_MASKAP_REC_IMAGE] = a.image;
            rec[VKN_MASKAP_REC_LABEL] = label;
            rec[VKN_MASKAP_REC_SCORE] = (int)__float_as_uint(score);
            rec[VKN_MASKAP_REC_RANK] = -1;
#pragma unroll
            for (int w = VKN_MASKAP_REC_WORDS; w < VKN_MASKAP_RECORD_INTS; ++w) rec[w] = 0;
        }
    }
    for (long long g = i0; g < a.G; g += step) {
        const int label = a.gt_labels[g];
        if (label < 0 || label >= cfg.num_classes) flags |= VKN_MASKAP_STATUS_LABEL_RANGE;
    }
    if (a.match_gt) {
        const long long n = (long long)cfg.A * cfg.T * a.K;
        for (long long i = i0; i < n; i += step) a.match_gt[i] = -1;
    }
    if (flags) atomicOr(a.header, flags);
}

// does the detection (score sj, position j) come before (score si, position i) in argsort(-score, kind='mergesort')?
__device__ __forceinline__ bool ap_before(float sj, int j, float si, int i) {
    const bool nj = sj != sj, ni = si != si;
    if (nj) return ni && j < i;
    if (ni) return true;
    return sj > si || (sj == si && j < i);
}

// grid num_classes * A, one wave: category c, area range r; lane t < T is threshold t
__global__ __launch_bounds__(64) void k_ap_match(const VknMaskApCfg cfg, const ApArgs a) {
    __shared__ int dl[AP_MAX], dord[AP_MAX], gord[AP_MAX];
    __shared__ unsigned char gig[AP_MAX], gcr[AP_MAX], gm[VKN_MASKAP_MAX_THRS][AP_MAX];
    const int lane = threadIdx.x, c = blockIdx.x / cfg.A, r = blockIdx.x % cfg.A;
    const double lo = cfg.area_lo[r], hi = cfg.area_hi[r];
    const unsigned base = a.header[1];
    const u64 below = (1ull << lane) - 1ull;
    // the category's detections in input order
    int nd = 0;
    for (int k0 = 0; k0 < a.K; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k < a.K && a.dt_labels[k] == c;
        const u64 m = __ballot(in);
        if (in) dl[nd + __popcll(m & below)] = k;
        nd += __popcll(m);
    }
    __syncthreads();
    // their order by descending score, stable
    for (int i = lane; i < nd; i += 64) {
        const int k = dl[i];
        const float si = a.scores[k];
        int rank = 0;
        for (int j = 0; j < nd; ++j) rank += j != i && ap_before(a.scores[dl[j]], j, si, i) ? 1 : 0;
        dord[rank] = k;
        const unsigned long long slot = (unsigned long long)base + (unsigned long long)k;
        if (r == 0 && rank < cfg.max_det && slot < (unsigned long long)cfg.cap_records)
            a.log[slot * VKN_MASKAP_RECORD_INTS + VKN_MASKAP_REC_RANK] = rank;
    }
    const int ndk = min(nd, cfg.max_det);
    // the category's ground truths, the ones that are not ignored first, each group in input order
    int ng = 0, npig = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int g0 = 0; g0 < a.G; g0 += 64) {
            const int g = g0 + lane;
            bool in = g < a.G && a.gt_labels[g] == c, crowd = false;
            if (in) {
                crowd = a.gt_crowd[g] != 0;
                const double ar = a.gt_area ? a.gt_area[g] : (double)a.area_gt[g];
                const bool ig = crowd || ar < lo || ar > hi;
                in = ig == (pass == 1);
            }
            const u64 m = __ballot(in);
            if (in) {
                const int at = ng + __popcll(m & below);
                gord[at] = g;
                gig[at] = (unsigned char)pass;
                gcr[at] = crowd ? 1 : 0;
            }
            ng += __popcll(m);
        }
        if (pass == 0) npig = ng;
    }
    for (int t = 0; t < cfg.T; ++t)
        for (int i = lane; i < ng; i += 64) gm[t][i] = 0;
    __syncthreads();
    if (lane == 0 && npig) add64(a.npig + (size_t)c * cfg.A + r, (u64)npig);
    const bool act = lane < cfg.T;
    const double thr = act ? cfg.iou_thrs[lane] : 0.0;
    for (int di = 0; di < ndk; ++di) {
        const int k = dord[di];
        const long long ad = a.area_dt[k];
        int m = -1;
        if (act) {
            double best = fmin(thr, 1.0 - 1e-10);
            for (int gi = 0; gi < ng; ++gi) {
                const bool crowd = gcr[gi] != 0;
                if (gm[lane][gi] && !crowd) continue;
                if (m > -1 && !gig[m] && gig[gi]) break;
                const int g = gord[gi];
                const long long I = a.inter[(size_t)k * a.G + g];
                double iou = 0.0;
                if (I != 0) {
                    const long long U = crowd ? ad : ad + a.area_gt[g] - I;
                    iou = (double)I / (double)U;
                }
                if (iou < best) continue;
                best = iou;
                m = gi;
            }
        }
        const bool matched = m > -1;
        const bool ignored = act && (matched ? gig[m] != 0 : ((double)ad < lo || (double)ad > hi));
        if (matched) {
            gm[lane][m] = 1;
            if (a.match_gt) a.match_gt[((size_t)r * cfg.T + lane) * a.K + k] = gord[m];
        }
        const u64 mw = __ballot(matched), iw = __ballot(ignored);
        const unsigned long long slot = (unsigned long long)base + (unsigned long long)k;
        if (lane == 0 && slot < (unsigned long long)cfg.cap_records) {
            int* rec = a.log + slot * VKN_MASKAP_RECORD_INTS + VKN_MASKAP_REC_WORDS + 2 * r;
            rec[0] = (int)(unsigned)mw;
            rec[1] = (int)(unsigned)iw;
        }
    }
}

__global__ void k_ap_end(const VknMaskApCfg cfg, const ApArgs a) {
    const unsigned count = a.header[1] + (unsigned)a.K;
    a.header[1] = count;
    if (count > (unsigned)cfg.cap_records) atomicOr(a.header, VKN_MASKAP_STATUS_FULL);
}

inline int ap_check_cfg(const VknMaskApCfg* cfg) {
    if (cfg->num_classes < 1 || cfg->num_classes > VKN_MASKAP_MAX_CLASSES || cfg->T < 1 || cfg->T > VKN_MASKAP_MAX_THRS || cfg->A < 1 ||
        cfg->A > VKN_MASKAP_MAX_AREAS || cfg->max_det < 1 || cfg->max_det > VKN_MASKAP_MAX_MASKS || cfg->cap_records < 1 ||
        cfg->cap_records > (1 << 24))
        return VKN_E_SHAPE;
    for (int t = 0; t < cfg->T; ++t)
        if (!(cfg->iou_thrs[t] == cfg->iou_thrs[t])) return VKN_E_SHAPE;
    for (int i = 0; i < cfg->A; ++i)
        if (!(cfg->area_lo[i] == cfg->area_lo[i]) || !(cfg->area_hi[i] == cfg->area_hi[i])) return VKN_E_SHAPE;
    return VKN_OK;
}

struct ApLayout {
    size_t off[3], bytes;
};
inline ApLayout ap_layout(const VknMaskApCfg* cfg) {
    ApLayout l;
    l.off[0] = 0;
    l.off[1] = VKN_MASKAP_HEADER_BYTES;
    l.off[2] = l.off[1] + up16((size_t)cfg->num_classes * cfg->A * 8);
    l.bytes = l.off[2] + up16((size_t)cfg->cap_records * VKN_MASKAP_RECORD_INTS * 4);
    return l;
}

}  // namespace

extern "C" {

size_t vkn_mask_overlap_workspace_bytes(int K, int G, int H, int W) {
    if (!overlap_shape_ok(K, G, H, W, 1)) return 0;
    return overlap_layout(K, G, H, W).bytes;
}

int vkn_mask_overlap_u8(const unsigned char* dt, const unsigned char* gt, int K, int G, int H, int W, long long* inter, long long* area_dt,
                        long long* area_gt, void* ws, size_t ws_bytes, void* stream) {
    return mask_overlap<unsigned char>(dt, 0.f, gt, K, G, H, W, inter, area_dt, area_gt, ws, ws_bytes, stream);
}

int vkn_mask_overlap_f32(const float* dt, float thr, const unsigned char* gt, int K, int G, int H, int W, long long* inter, long long* area_dt,
                         long long* area_gt, void* ws, size_t ws_bytes, void* stream) {
    return mask_overlap<float>(dt, thr, gt, K, G, H, W, inter, area_dt, area_gt, ws, ws_bytes, stream);
}

size_t vkn_sizeof_mask_ap_cfg(void) { return sizeof(VknMaskApCfg); }

size_t vkn_mask_ap_state_bytes(const VknMaskApCfg* cfg) {
    if (!cfg || ap_check_cfg(cfg) != VKN_OK) return 0;
    return ap_layout(cfg).bytes;
}

int vkn_mask_ap_state_layout(const VknMaskApCfg* cfg, size_t* offsets3) {
    if (!cfg || !offsets3) return VKN_E_ARG;
    const int rc = ap_check_cfg(cfg);
    if (rc != VKN_OK) return rc;
    const ApLayout l = ap_layout(cfg);
    for (int i = 0; i < 3; ++i) offsets3[i] = l.off[i];
    return VKN_OK;
}

int vkn_mask_ap_reset(const VknMaskApCfg* cfg, void* state, size_t state_bytes, void* stream) {
    if (!cfg || !state) return VKN_E_ARG;
    const int rc = ap_check_cfg(cfg);
    if (rc != VKN_OK) return rc;
    const ApLayout l = ap_layout(cfg);
    if (state_bytes != l.bytes) return VKN_E_WORKSPACE;
    if (!vkn_aligned(state, 16)) return VKN_E_ALIGN;
    if (!vkn_on_device(state)) return VKN_E_ARG;
    if (hipMemsetAsync(state, 0, l.bytes, static_cast<hipStream_t>(stream)) != hipSuccess) return VKN_E_LAUNCH;
    return VKN_OK;
}

int vkn_mask_ap_match(const VknMaskApCfg* cfg, void* state, size_t state_bytes, const long long* inter, const long long* area_dt,
                      const long long* area_gt, const float* scores, const int* dt_labels, const int* gt_labels, const unsigned char* gt_crowd,
                      const double* gt_area, int K, int G, int image_seq, int* match_gt, void* stream) {
    if (!cfg || !state || K < 0 || G < 0) return VKN_E_ARG;
    const bool both = K > 0 && G > 0;
    if ((K > 0 && (!area_dt || !scores || !dt_labels)) || (G > 0 && (!area_gt || !gt_labels || !gt_crowd)) || (both && !inter)) return VKN_E_ARG;
    const int rc = ap_check_cfg(cfg);
    if (rc != VKN_OK) return rc;
    if (K > VKN_MASKAP_MAX_MASKS || G > VKN_MASKAP_MAX_MASKS) return VKN_E_SHAPE;
    const ApLayout l = ap_layout(cfg);
    if (state_bytes != l.bytes) return VKN_E_WORKSPACE;
    if (!vkn_aligned(state, 16) || (K > 0 && (!vkn_aligned(area_dt, 16) || !vkn_aligned(scores, 4) || !vkn_aligned(dt_labels, 4))) ||
        (G > 0 && (!vkn_aligned(area_gt, 16) || !vkn_aligned(gt_labels, 4) || (gt_area && !vkn_aligned(gt_area, 8)))) ||
        (both && !vkn_aligned(inter, 16)) || (K > 0 && match_gt && !vkn_aligned(match_gt, 4)))
        return VKN_E_ALIGN;
    if (!vkn_on_device(state) || (K > 0 && (!vkn_on_device(area_dt) || !vkn_on_device(scores) || !vkn_on_device(dt_labels))) ||
        (G > 0 && (!vkn_on_device(area_gt) || !vkn_on_device(gt_labels) || !vkn_on_device(gt_crowd) || (gt_area && !vkn_on_device(gt_area)))) ||
        (both && !vkn_on_device(inter)) || (K > 0 && match_gt && !vkn_on_device(match_gt)))
        return VKN_E_ARG;
    if (K + G == 0) return VKN_OK;
    char* base = static_cast<char*>(state);
    ApArgs a;
    a.header = reinterpret_cast<unsigned*>(base + l.off[0]);
    a.npig = reinterpret_cast<long long*>(base + l.off[1]);
    a.log = reinterpret_cast<int*>(base + l.off[2]);
    a.inter = inter, a.area_dt = area_dt, a.area_gt = area_gt, a.scores = scores, a.dt_labels = dt_labels, a.gt_labels = gt_labels;
    a.gt_crowd = gt_crowd, a.gt_area = G > 0 ? gt_area : nullptr, a.match_gt = K > 0 ? match_gt : nullptr;
    a.K = K, a.G = G, a.image = image_seq;
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long items = K > G ? K : G;
    if (a.match_gt) items = (long long)cfg->A * cfg->T * K;                          // (>= K, and G needs no more than 1024 threads)
    if (items < G) items = G;
    const long long blocks = (items + 255) / 256;
    hipLaunchKernelGGL(k_ap_begin, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, *cfg, a);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ap_match, dim3((unsigned)(cfg->num_classes * cfg->A)), dim3(64), 0, st, *cfg, a);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ap_end, dim3(1), dim3(1), 0, st, *cfg, a);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

size_t vkn_bits_mask_overlap_workspace_bytes(int K, int G, int H, int W) {
    if (!overlap_shape_ok(K, G, H, W, 1)) return 0;
    return overlap_layout(K, G, H, W, false).bytes;
}

int vkn_bits_mask_overlap(const long long* dt_bits, const unsigned char* gt, int K, int G, int H, int W, long long* inter, long long* area_dt,
                          long long* area_gt, void* ws, size_t ws_bytes, void* stream) {
    return mask_overlap<u64>(reinterpret_cast<const u64*>(dt_bits), 0.f, gt, K, G, H, W, inter, area_dt, area_gt, ws, ws_bytes, stream);
}

}  // extern "C"
