// vkn_stq.hip — the STQ meter on the device (include/vkn_stq.h): the four integer tables of `STQuality.update_state`
// (tools/utils/STQ.py:106-188) from the four int32 maps of B frames, one launch.
//
// The pixel pass is the counting engine of vkn_mapcount.h with four kinds of count: a workgroup walks spans of VKN_STQ_SPAN_PX pixels (at
// most VKN_STQ_MAX_GRID workgroups, each on neighbouring spans, across frames) and keeps ONE table of VKN_STQ_LDS_SLOTS slots in LDS, whose
// footprint does not depend on the class count.  What leaves that table is one update in global memory: a confusion cell is a 64-bit add
// into the dense matrix, a tube or pair one insert into its open-addressing table, at agent scope.
#include "../../include/vkn_stq.h"
#include "vkn_common.h"
#include "vkn_mapcount.h"

namespace {

constexpr int STQ_THREADS = 256;
enum { K_PAIR = 0, K_GT = 1, K_PRED = 2, K_CONF = 3 };      // kind 3 (confusion) keys are below 2^16

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
// a workgroup's state, and what mapcount needs to know of the meter
struct StqLds {
    static constexpr int KINDS = 4, SLOTS = VKN_STQ_LDS_SLOTS, THREADS = STQ_THREADS, SPAN_PX = VKN_STQ_SPAN_PX;
    unsigned long long keys[SLOTS];
    unsigned counts[SLOTS];
    StqArgs a;                        // the launch's arguments: the out-of-line helpers index its tables by kind
    unsigned flags;
    unsigned char thing[256];

    static __device__ __forceinline__ unsigned hash(unsigned long long k) {
        k *= 0x9E3779B97F4A7C15ull;
        return (unsigned)(k >> 32) ^ (unsigned)k;
    }
    static __device__ __noinline__ void sink(const StqLds& s, int kind, unsigned long long key, unsigned cnt);
    static __device__ __forceinline__ void pixel(StqLds& s, const StqArgs& a, mapcount::Run (&run)[4], unsigned& flags, int gs, int gi, int ps, int pi);
};

// one (key, count) into its global table
__device__ void StqLds::sink(const StqLds& s, int kind, unsigned long long key, unsigned cnt) {
    const StqArgs& a = s.a;
    if (kind == K_CONF)
        __hip_atomic_fetch_add(a.conf + key, (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        mapcount::table_add<__HIP_MEMORY_SCOPE_AGENT, StqLds>(a.keys[kind], a.counts[kind], a.cap_mask[kind], key, cnt, a.header, a.full_bit[kind]);
}

__device__ __forceinline__ void StqLds::pixel(StqLds& s, const StqArgs& a, mapcount::Run (&run)[4], unsigned& flags, int gs, int gi, int ps, int pi) {
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
    mapcount::push(s, run[K_CONF], live, ((unsigned long long)(csl * a.n + csp) << 2) | K_CONF);
    mapcount::push(s, run[K_PRED], pm, (yp << 2) | K_PRED);
    mapcount::push(s, run[K_GT], lm, (yt << 2) | K_GT);
    mapcount::push(s, run[K_PAIR], lm && pm, ((yt * (unsigned long long)a.offset + yp) << 2) | K_PAIR);
}

// grid: min(B * ceil(HW / VKN_STQ_SPAN_PX), VKN_STQ_MAX_GRID) workgroups; a workgroup walks `per` neighbouring spans and keeps its table in
// LDS over all of them, so the global updates — atomics on few, contended addresses — grow with the workgroups, not with the spans
__global__ __launch_bounds__(STQ_THREADS) void k_stq_update(StqArgs a, const unsigned char* __restrict__ is_thing, const int* __restrict__ gt_sem,
                                                            const int* __restrict__ gt_ins, const int* __restrict__ pred_sem,
                                                            const int* __restrict__ pred_ins, int B, int HW, int spans, int per) {
    __shared__ StqLds s;
    const int tid = threadIdx.x;
    mapcount::clear(s);
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
        mapcount::walk(s, a, flags, gt_sem + base, gt_ins + base, pred_sem + base, pred_ins + base, p0, p1);
    }
    if (flags) atomicOr(&s.flags, flags);
    __syncthreads();

    mapcount::flush(s);
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
    if (!vkn_aligned(state, 16)) return VKN_E_ALIGN;
    if (!vkn_on_device(state)) return VKN_E_ARG;
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
    if (!vkn_aligned(state, 16) || !vkn_aligned(gt_sem, 4) || !vkn_aligned(gt_ins, 4) || !vkn_aligned(pred_sem, 4) || !vkn_aligned(pred_ins, 4))
        return VKN_E_ALIGN;
    if (!vkn_on_device(state) || !vkn_on_device(is_thing) || !vkn_on_device(gt_sem) || !vkn_on_device(gt_ins) || !vkn_on_device(pred_sem) ||
        !vkn_on_device(pred_ins))
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
