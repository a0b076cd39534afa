// vkn_stq.hip — the STQ meter on the device (include/vkn_stq.h): the four integer tables of `STQuality.update_state`
// (tools/utils/STQ.py:106-188) from the four int32 maps of B frames, one launch.
//
// Traffic is 16 bytes per pixel and nothing else may scale with the pixels: a workgroup walks spans of VKN_STQ_SPAN_PX contiguous
// pixels of one frame (at most VKN_STQ_MAX_GRID workgroups, each on neighbouring spans), a lane loads four neighbouring pixels of each
// map with one 16-byte load (where that map is aligned behind the span's peel) and keeps, per kind of count, a running (key, count) in
// registers that it only hands on when the key changes.  What it hands on goes into ONE table in LDS (VKN_STQ_LDS_SLOTS slots: a 64-bit
// key that carries the 2-bit kind, a 32-bit count), first summed over the lanes of the wave that hold the same key.  When the workgroup
// has walked its spans every occupied slot becomes one update in global memory: a confusion cell is a 64-bit add into the dense matrix,
// a tube or pair a 64-bit compare-and-swap on the key slot (linear probing, at most `cap` slots) and a 64-bit add on the count, all at
// agent scope.  A key that finds no slot in LDS within STQ_LDS_PROBES takes the global path itself: correct, only slower.  The LDS
// footprint does not depend on the class count.
#include "../../include/vkn_stq.h"
#include "vkn_common.h"

namespace {

constexpr int STQ_THREADS = 256;
constexpr int STQ_LDS_PROBES = 32;                 // slots tried in LDS before a count goes to global memory directly
constexpr unsigned long long STQ_EMPTY = ~0ull;    // no tagged key is all ones: kind 3 (confusion) keys are below 2^16
enum { K_PAIR = 0, K_GT = 1, K_PRED = 2, K_CONF = 3 };
static_assert((VKN_STQ_LDS_SLOTS & (VKN_STQ_LDS_SLOTS - 1)) == 0 && VKN_STQ_SPAN_PX % (4 * STQ_THREADS) == 0, "span / table geometry");
constexpr int STQ_CNT_BITS = 6;                    // a lane counts at most SPAN_PX / THREADS body pixels + 1 head or tail pixel
static_assert(VKN_STQ_SPAN_PX / STQ_THREADS + 1 < (1 << STQ_CNT_BITS), "a lane's run count must fit STQ_CNT_BITS");

struct StqLayout {
    size_t off[8];
    size_t bytes;
    int n;
};

struct StqArgs {
    unsigned* header;                 // status, frames
    unsigned long long* conf;
    long long* keys[3];               // indexed by kind: pair, gt, pred
    unsigned long long* counts[3];
    unsigned cap_mask[3];
    unsigned full_bit[3];
    long long offset;
    int nc, n, ignore, shift, drop, map_ignore;
};

inline bool stq_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline bool stq_on_device(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // an unregistered host pointer: clear the sticky error
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}
inline bool stq_cap_ok(int cap) { return cap >= VKN_STQ_MIN_CAP && cap <= VKN_STQ_MAX_CAP && (cap & (cap - 1)) == 0; }

inline int stq_check_cfg(const VknStqCfg* c) {
    if (c->num_classes < 1 || c->num_classes > VKN_STQ_MAX_CLASSES || c->label_bit_shift < 1 || c->label_bit_shift > 30) return VKN_E_SHAPE;
    const long long lower = (long long)c->num_classes << c->label_bit_shift, upper = (long long)(c->num_classes + 1) << c->label_bit_shift;
    if (c->offset < lower || c->offset > ((1ll << 62) - 1) / upper) return VKN_E_SHAPE;      // upper * offset < 2^62
    if (!stq_cap_ok(c->cap_gt) || !stq_cap_ok(c->cap_pred) || !stq_cap_ok(c->cap_pair)) return VKN_E_SHAPE;
    return VKN_OK;
}

inline StqLayout stq_layout(const VknStqCfg* c) {
    StqLayout l;
    l.n = c->ignore_label >= c->num_classes ? c->num_classes + 1 : c->num_classes;
    size_t at = 0;
    l.off[0] = at;
    at += VKN_STQ_HEADER_BYTES;
    l.off[1] = at;
    at += ((size_t)l.n * l.n * 8 + 15) & ~(size_t)15;
    const int caps[3] = {c->cap_gt, c->cap_pred, c->cap_pair};
    for (int t = 0; t < 3; ++t) {
        l.off[2 + 2 * t] = at;
        at += (size_t)caps[t] * 8;
        l.off[3 + 2 * t] = at;
        at += (size_t)caps[t] * 8;
    }
    l.bytes = at;
    return l;
}

// ----------------------------------------------------------------------------------------------------------------------- reset
// the state as 8-byte words: the three key arrays -1, everything else 0
__global__ __launch_bounds__(256) void k_stq_reset(unsigned long long* __restrict__ state, size_t words, size_t k0, size_t k0e, size_t k1,
                                                   size_t k1e, size_t k2, size_t k2e) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
        const bool key = (i >= k0 && i < k0e) || (i >= k1 && i < k1e) || (i >= k2 && i < k2e);
        state[i] = key ? ~0ull : 0ull;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- update
__device__ __forceinline__ unsigned stq_hash(unsigned long long k) {
    k *= 0x9E3779B97F4A7C15ull;
    return (unsigned)(k >> 32) ^ (unsigned)k;
}

struct StqLds {
    unsigned long long keys[VKN_STQ_LDS_SLOTS];
    unsigned counts[VKN_STQ_LDS_SLOTS];
    StqArgs a;                        // the launch's arguments: the out-of-line helpers index its tables by kind
    unsigned flags;
    unsigned char thing[256];
};

// one (key, count) into its global table: the key slot by compare-and-swap, at most `cap` slots, then the count
__device__ void stq_global_add(const StqLds& s, int kind, unsigned long long key, unsigned cnt) {
    const StqArgs& a = s.a;
    if (kind == K_CONF) {
        __hip_atomic_fetch_add(a.conf + key, (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    long long* keys = a.keys[kind];
    const unsigned mask = a.cap_mask[kind];
    unsigned i = stq_hash(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe, i = (i + 1) & mask) {
        long long cur = __hip_atomic_load(keys + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == -1) {
            long long expect = -1;
            if (__hip_atomic_compare_exchange_strong(keys + i, &expect, (long long)key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                cur = (long long)key;
            else
                cur = expect;                        // another workgroup took the slot: perhaps with this very key
        }
        if (cur == (long long)key) {
            __hip_atomic_fetch_add(a.counts[kind] + i, (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    __hip_atomic_fetch_or(a.header, a.full_bit[kind], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // full: the count is dropped
}

// one tagged (key, count) into the workgroup's table
__device__ void stq_lds_add(StqLds& s, unsigned long long tagged, unsigned cnt) {
    unsigned i = stq_hash(tagged) & (VKN_STQ_LDS_SLOTS - 1);
    for (int probe = 0; probe < STQ_LDS_PROBES; ++probe, i = (i + 1) & (VKN_STQ_LDS_SLOTS - 1)) {
        const unsigned long long old = atomicCAS(&s.keys[i], STQ_EMPTY, tagged);
        if (old == STQ_EMPTY || old == tagged) {
            atomicAdd(&s.counts[i], cnt);
            return;
        }
    }
    stq_global_add(s, (int)(tagged & 3), tagged >> 2, cnt);
}

// Lanes that hand on a count at the same point: the lanes that hold the first such lane's key are summed (a lane's count has
// STQ_CNT_BITS bits: one ballot per bit) and that lane alone adds the sum; the others add their own.
__device__ __forceinline__ void stq_emit(StqLds& s, bool e, unsigned long long tagged, unsigned cnt) {
    if (e) {
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)tagged), hi = __builtin_amdgcn_readfirstlane((unsigned)(tagged >> 32));
        const bool match = tagged == (((unsigned long long)hi << 32) | lo);
        const unsigned long long mm = __ballot(match);
        unsigned sum = 0;
#pragma unroll
        for (int b = 0; b < STQ_CNT_BITS; ++b) sum += (unsigned)__popcll(__ballot(match && ((cnt >> b) & 1))) << b;
        const int lane = threadIdx.x & 63;
        if (match) {
            if (lane == __ffsll((long long)mm) - 1) stq_lds_add(s, tagged, sum);
        } else {
            stq_lds_add(s, tagged, cnt);
        }
    }
}

struct StqRun {
    unsigned long long key;
    unsigned cnt;
};

__device__ __forceinline__ void stq_push(StqLds& s, StqRun& r, bool valid, unsigned long long tagged) {
    const bool change = valid && r.key != tagged;
    stq_emit(s, change && r.cnt > 0, r.key, r.cnt);
    if (change) {
        r.key = tagged;
        r.cnt = 0;
    }
    r.cnt += valid ? 1u : 0u;
}

__device__ __forceinline__ void stq_pixel(StqLds& s, const StqArgs& a, StqRun (&run)[4], unsigned& flags, int gs, int gi, int ps, int pi) {
    bool live = !(a.drop && gs == a.ignore);
    const int sl = (a.map_ignore && gs == a.ignore) ? a.nc : gs, sp = (a.map_ignore && ps == a.ignore) ? a.nc : ps;
    const bool bad_class = (unsigned)sl >= (unsigned)a.n || (unsigned)sp >= (unsigned)a.n;
    const bool bad_id = ((unsigned)gi >> a.shift) != 0 || ((unsigned)pi >> a.shift) != 0;      // negative ids have the top bit set
    if (live && bad_class) flags |= VKN_STQ_STATUS_CLASS_RANGE;
    if (live && bad_id) flags |= VKN_STQ_STATUS_ID_RANGE;
    live = live && !bad_class && !bad_id;
    const int csl = live ? sl : 0, csp = live ? sp : 0;
    bool lm = live && csl < a.nc && s.thing[csl], pm = live && csp < a.nc && s.thing[csp];
    const bool crowd = lm && gi == 0;
    lm = lm && !crowd;
    pm = pm && !crowd;
    const unsigned long long yt = ((unsigned long long)(unsigned)csl << a.shift) + (unsigned)gi;
    const unsigned long long yp = ((unsigned long long)(unsigned)csp << a.shift) + (unsigned)pi;
    stq_push(s, run[K_CONF], live, ((unsigned long long)(csl * a.n + csp) << 2) | K_CONF);
    stq_push(s, run[K_PRED], pm, (yp << 2) | K_PRED);
    stq_push(s, run[K_GT], lm, (yt << 2) | K_GT);
    stq_push(s, run[K_PAIR], lm && pm, ((yt * (unsigned long long)a.offset + yp) << 2) | K_PAIR);
}

// grid: min(B * ceil(HW / VKN_STQ_SPAN_PX), VKN_STQ_MAX_GRID) workgroups; a workgroup walks `per` neighbouring spans and keeps its table in
// LDS over all of them, so the global updates — atomics on few, contended addresses — grow with the workgroups, not with the spans
__global__ __launch_bounds__(STQ_THREADS) void k_stq_update(StqArgs a, const unsigned char* __restrict__ is_thing, const int* __restrict__ gt_sem,
                                                            const int* __restrict__ gt_ins, const int* __restrict__ pred_sem,
                                                            const int* __restrict__ pred_ins, int B, int HW, int spans, int per) {
    __shared__ StqLds s;
    const int tid = threadIdx.x;
    for (int i = tid; i < VKN_STQ_LDS_SLOTS; i += STQ_THREADS) {
        s.keys[i] = STQ_EMPTY;
        s.counts[i] = 0;
    }
    s.thing[tid] = tid < a.nc ? is_thing[tid] : (unsigned char)0;
    if (tid == 0) {
        s.flags = 0;
        s.a = a;
    }
    __syncthreads();

    unsigned flags = 0;
    const int first = blockIdx.x * per, last = min(B * spans, first + per);
    for (int sn = first; sn < last; ++sn) {
        const int b = sn / spans, sp = sn - b * spans;
        const size_t base = (size_t)b * HW;
        const int p0 = sp * VKN_STQ_SPAN_PX, p1 = min(HW, p0 + VKN_STQ_SPAN_PX);
        const int* m0 = gt_sem + base;
        const int* m1 = gt_ins + base;
        const int* m2 = pred_sem + base;
        const int* m3 = pred_ins + base;
        // the peel: pixels in front of gt_sem's first 16-byte boundary inside the span; a map that is aligned differently is loaded by words
        const int mis = (int)((reinterpret_cast<uintptr_t>(m0 + p0) >> 2) & 3);
        const int head = min((4 - mis) & 3, p1 - p0);
        const int q0 = p0 + head, groups = (p1 - q0) >> 2, q1 = q0 + 4 * groups;
        const bool v1 = ((reinterpret_cast<uintptr_t>(m1 + q0)) & 15) == 0, v2 = ((reinterpret_cast<uintptr_t>(m2 + q0)) & 15) == 0,
                   v3 = ((reinterpret_cast<uintptr_t>(m3 + q0)) & 15) == 0;

        StqRun run[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) run[k] = StqRun{STQ_EMPTY, 0u};

        // head and tail pixels (fewer than 4 each), one per lane
        {
            const int p = tid < head ? p0 + tid : q1 + (tid - head);
            if (p < p1 && (tid < head || p >= q1)) stq_pixel(s, a, run, flags, m0[p], m1[p], m2[p], m3[p]);
        }
        for (int g = tid; g < groups; g += STQ_THREADS) {
            const int p = q0 + 4 * g;
            const int4 x0 = *reinterpret_cast<const int4*>(m0 + p);
            const int4 x1 = v1 ? *reinterpret_cast<const int4*>(m1 + p) : make_int4(m1[p], m1[p + 1], m1[p + 2], m1[p + 3]);
            const int4 x2 = v2 ? *reinterpret_cast<const int4*>(m2 + p) : make_int4(m2[p], m2[p + 1], m2[p + 2], m2[p + 3]);
            const int4 x3 = v3 ? *reinterpret_cast<const int4*>(m3 + p) : make_int4(m3[p], m3[p + 1], m3[p + 2], m3[p + 3]);
            stq_pixel(s, a, run, flags, x0.x, x1.x, x2.x, x3.x);
            stq_pixel(s, a, run, flags, x0.y, x1.y, x2.y, x3.y);
            stq_pixel(s, a, run, flags, x0.z, x1.z, x2.z, x3.z);
            stq_pixel(s, a, run, flags, x0.w, x1.w, x2.w, x3.w);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) stq_emit(s, run[k].cnt > 0, run[k].key, run[k].cnt);      // per span: a lane's count stays in STQ_CNT_BITS
    }
    if (flags) atomicOr(&s.flags, flags);
    __syncthreads();

    for (int i = tid; i < VKN_STQ_LDS_SLOTS; i += STQ_THREADS) {
        const unsigned long long tagged = s.keys[i];
        if (tagged != STQ_EMPTY) stq_global_add(s, (int)(tagged & 3), tagged >> 2, s.counts[i]);
    }
    if (tid == 0) {
        if (s.flags) __hip_atomic_fetch_or(a.header, s.flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (blockIdx.x == 0) __hip_atomic_fetch_add(a.header + 1, (unsigned)B, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

extern "C" {

size_t vkn_sizeof_stq_cfg(void) { return sizeof(VknStqCfg); }

size_t vkn_stq_state_bytes(const VknStqCfg* cfg) {
    if (!cfg || stq_check_cfg(cfg) != VKN_OK) return 0;
    return stq_layout(cfg).bytes;
}

int vkn_stq_state_layout(const VknStqCfg* cfg, size_t* offsets8) {
    if (!cfg || !offsets8) return VKN_E_ARG;
    const int rc = stq_check_cfg(cfg);
    if (rc != VKN_OK) return rc;
    const StqLayout l = stq_layout(cfg);
    for (int i = 0; i < 8; ++i) offsets8[i] = l.off[i];
    return VKN_OK;
}

int vkn_stq_reset(const VknStqCfg* cfg, void* state, size_t state_bytes, void* stream) {
    if (!cfg || !state) return VKN_E_ARG;
    const int rc = stq_check_cfg(cfg);
    if (rc != VKN_OK) return rc;
    const StqLayout l = stq_layout(cfg);
    if (state_bytes != l.bytes) return VKN_E_WORKSPACE;
    if (!stq_aligned(state, 16)) return VKN_E_ALIGN;
    if (!stq_on_device(state)) return VKN_E_ARG;
    const size_t words = l.bytes / 8;
    const int grid = (int)((words + 255) / 256 < 1024 ? (words + 255) / 256 : 1024);
    hipLaunchKernelGGL(k_stq_reset, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<unsigned long long*>(state), words,
                       l.off[2] / 8, l.off[3] / 8, l.off[4] / 8, l.off[5] / 8, l.off[6] / 8, l.off[7] / 8);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

int vkn_stq_update_i32(const VknStqCfg* cfg, void* state, size_t state_bytes, const unsigned char* is_thing, const int* gt_sem,
                       const int* gt_ins, const int* pred_sem, const int* pred_ins, int B, int HW, void* stream) {
    if (!cfg || !state || !is_thing || !gt_sem || !gt_ins || !pred_sem || !pred_ins || B < 0 || HW < 0) return VKN_E_ARG;
    const int rc = stq_check_cfg(cfg);
    if (rc != VKN_OK) return rc;
    if (B < 1 || HW < 1 || (long long)B * HW * 4 >= (1ll << 31)) return VKN_E_SHAPE;
    const StqLayout l = stq_layout(cfg);
    if (state_bytes != l.bytes) return VKN_E_WORKSPACE;
    if (!stq_aligned(state, 16) || !stq_aligned(gt_sem, 4) || !stq_aligned(gt_ins, 4) || !stq_aligned(pred_sem, 4) || !stq_aligned(pred_ins, 4))
        return VKN_E_ALIGN;
    if (!stq_on_device(state) || !stq_on_device(is_thing) || !stq_on_device(gt_sem) || !stq_on_device(gt_ins) || !stq_on_device(pred_sem) ||
        !stq_on_device(pred_ins))
        return VKN_E_ARG;
    char* base = static_cast<char*>(state);
    StqArgs a;
    a.header = reinterpret_cast<unsigned*>(base + l.off[0]);
    a.conf = reinterpret_cast<unsigned long long*>(base + l.off[1]);
    const int slot[3] = {6, 2, 4};                       // kind (pair, gt, pred) -> its keys' place in the layout
    const int caps[3] = {cfg->cap_pair, cfg->cap_gt, cfg->cap_pred};
    const unsigned bits[3] = {VKN_STQ_STATUS_FULL_PAIR, VKN_STQ_STATUS_FULL_GT, VKN_STQ_STATUS_FULL_PRED};
    for (int k = 0; k < 3; ++k) {
        a.keys[k] = reinterpret_cast<long long*>(base + l.off[slot[k]]);
        a.counts[k] = reinterpret_cast<unsigned long long*>(base + l.off[slot[k] + 1]);
        a.cap_mask[k] = (unsigned)caps[k] - 1;
        a.full_bit[k] = bits[k];
    }
    a.offset = cfg->offset;
    a.nc = cfg->num_classes;
    a.n = l.n;
    a.ignore = cfg->ignore_label;
    a.shift = cfg->label_bit_shift;
    a.drop = cfg->drop_ignored_gt != 0;
    a.map_ignore = cfg->ignore_label > cfg->num_classes;
    const int spans = (HW + VKN_STQ_SPAN_PX - 1) / VKN_STQ_SPAN_PX;
    const long long total = (long long)B * spans;                                   // < 2^29: B HW < 2^29
    const int per = (int)((total + VKN_STQ_MAX_GRID - 1) / VKN_STQ_MAX_GRID), grid = (int)((total + per - 1) / per);
    hipLaunchKernelGGL(k_stq_update, dim3(grid), dim3(STQ_THREADS), 0, static_cast<hipStream_t>(stream), a, is_thing, gt_sem, gt_ins, pred_sem,
                       pred_ins, B, HW, spans, per);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

}  // extern "C"
