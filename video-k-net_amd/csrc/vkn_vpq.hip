// vkn_vpq.hip — the VPQ meter on the device (include/vkn_vpq.h): `vpq_eval` (tools/eval_dvpq_step.py:21-97) for every window of every
// window length, from the four int32 maps of B consecutive frames.
//
// A window's areas are the sums of its frames' areas, so the pixels are read ONCE: k_vpq_count counts each frame into that frame's slot
// of a ring of per-frame tables (gt areas, pred areas, pair areas) with the counting engine of vkn_mapcount.h, three kinds of count: spans
// of VKN_VPQ_SPAN_PX pixels, ONE table in LDS per workgroup, then per occupied slot one insert into the frame's open-addressing tables at
// agent scope.  A workgroup stays inside one frame, so the LDS key needs no frame tag.
// k_vpq_window never touches a pixel: one workgroup per (frame f, window length k) sums the ring slots
// of frames f - k + 1 .. f into window tables and runs the matching in three phases over those tables.  The window tables live in LDS
// when they fit its 160 KiB less 4 KiB of counters (the default capacities take 52 KiB), else in the state's scratch.  Frames of a call share the launches in
// groups of VKN_VPQ_GROUP: clear the group's ring slots, count, windows; the ring holds the max(ks) - 1 frames before a group and the
// group itself.  Stream order is the only synchronisation between the kernels.
//
// Inside k_vpq_window what one wave adds another wave reads in the next phase.  In LDS a barrier between the phases is enough.  In the
// scratch every access is an agent-scope atomic (performed at L2, never served from the CU's L1) and the barrier comes with an agent fence.
#include "../../include/vkn_vpq.h"
#include "vkn_common.h"
#include "vkn_mapcount.h"

namespace {

constexpr int VPQ_THREADS = 256;
constexpr int VPQ_WIN_THREADS = 1024;            // a window's workgroup: its work is chains of dependent table accesses, hidden by waves
constexpr size_t VPQ_WIN_STATIC_LDS = 4096;        // the window kernel's own LDS
constexpr size_t VPQ_LDS_BYTES = 160 * 1024 - VPQ_WIN_STATIC_LDS;      // window tables up to this size live in LDS
constexpr long long VPQ_MATCHED = 1ll << 62;       // on a window table's count: the segment has a true positive (areas stay below 2^34)
enum { K_PAIR = 0, K_GT = 1, K_PRED = 2 };
static_assert(VKN_VPQ_GROUP <= VKN_VPQ_MAX_GRID, "a group's frames each get a workgroup");

struct VpqLayout {
    size_t off[4];
    size_t bytes;
    size_t ring, scratch;             // byte offsets inside the state
    size_t slot_words, set_words;     // 8-byte words of one ring slot, of one window's scratch
    int R;                            // ring slots
};

// one set of tables, as 8-byte words from its base: keys (-1 = empty) and counts of pair, gt, pred (by kind), then pred's ignored overlap
struct VpqTables {
    size_t keys[3], counts[3], ign;
    unsigned cap_mask[3];
    unsigned full_bit[3];
};

struct VpqArgs {
    unsigned* header;                 // status, frames, log_used
    unsigned* base;                   // private: the sequence's frame count at the start of the call
    unsigned long long* acc;
    long long* log;
    long long* ring;
    long long* scratch;
    VpqTables t;
    size_t slot_words, set_words;
    long long offset;
    int num_cat, ign, shift, nk, ks[VKN_VPQ_MAX_KS], cap_log, R;
};

inline bool vpq_cap_ok(int cap) { return cap >= VKN_VPQ_MIN_CAP && cap <= VKN_VPQ_MAX_CAP && (cap & (cap - 1)) == 0; }

inline int vpq_check_cfg(const VknVpqCfg* c) {
    if (c->num_cat < 1 || c->num_cat > VKN_VPQ_MAX_CAT || c->ign_id < c->num_cat || c->ign_id > 255) return VKN_E_SHAPE;
    if (c->label_bit_shift < 1 || c->label_bit_shift > 30) return VKN_E_SHAPE;
    const long long lower = (long long)c->num_cat << c->label_bit_shift, upper = (long long)(c->ign_id + 1) << c->label_bit_shift;
    if (c->offset < lower || c->offset > ((1ll << 62) - 1) / upper) return VKN_E_SHAPE;      // upper * offset < 2^62
    if (c->nk < 1 || c->nk > VKN_VPQ_MAX_KS) return VKN_E_SHAPE;
    for (int i = 0; i < c->nk; ++i)
        if (c->ks[i] < 1 || c->ks[i] > VKN_VPQ_MAX_K || (i > 0 && c->ks[i] <= c->ks[i - 1])) return VKN_E_SHAPE;
    if (!vpq_cap_ok(c->cap_gt) || !vpq_cap_ok(c->cap_pred) || !vpq_cap_ok(c->cap_pair) || !vpq_cap_ok(c->cap_log)) return VKN_E_SHAPE;
    return VKN_OK;
}

inline VpqLayout vpq_layout(const VknVpqCfg* c) {
    VpqLayout l;
    size_t at = 0;
    l.off[0] = at;
    at += VKN_VPQ_HEADER_BYTES;
    l.off[1] = at;
    at += ((size_t)c->nk * 3 * c->num_cat * 8 + 15) & ~(size_t)15;
    l.off[2] = at;
    at += (size_t)c->cap_log * 32;
    l.off[3] = at;
    at += 16;                                                          // the private frame base
    l.R = c->ks[c->nk - 1] - 1 + VKN_VPQ_GROUP;
    l.slot_words = 2 * ((size_t)c->cap_gt + c->cap_pred + c->cap_pair);
    l.set_words = l.slot_words + (size_t)c->cap_pred;
    l.ring = at;
    at += (size_t)l.R * l.slot_words * 8;
    l.scratch = at;
    at += (size_t)VKN_VPQ_GROUP * c->nk * l.set_words * 8;
    l.bytes = at;
    return l;
}

inline VpqTables vpq_tables(const VknVpqCfg* c) {
    VpqTables t;
    const int caps[3] = {c->cap_pair, c->cap_gt, c->cap_pred};          // by kind
    const int order[3] = {K_GT, K_PRED, K_PAIR};                        // in memory
    const unsigned bits[3] = {VKN_VPQ_STATUS_FULL_PAIR, VKN_VPQ_STATUS_FULL_GT, VKN_VPQ_STATUS_FULL_PRED};
    size_t at = 0;
    for (int o = 0; o < 3; ++o) {
        const int k = order[o];
        t.keys[k] = at;
        at += (size_t)caps[k];
        t.counts[k] = at;
        at += (size_t)caps[k];
        t.cap_mask[k] = (unsigned)caps[k] - 1;
        t.full_bit[k] = bits[k];
    }
    t.ign = at;
    return t;
}

// a counting workgroup's state, and what mapcount needs to know of the meter
struct VpqLds {
    static constexpr int KINDS = 3, SLOTS = VKN_VPQ_LDS_SLOTS, THREADS = VPQ_THREADS, SPAN_PX = VKN_VPQ_SPAN_PX;
    unsigned long long keys[SLOTS];
    unsigned counts[SLOTS];
    VpqArgs a;                        // the launch's arguments: the out-of-line helpers index its tables by kind
    long long* slot;                  // the frame's ring slot
    unsigned flags;

    // The keys are a few small fields far apart (class << 16 | id, and gt_id * offset + pred_id): one multiplication leaves the low bits
    // of either half poor in them (2400 such pair keys had 299 distinct homes among 8192 slots, probe chains of up to 42), so every bit
    // is folded down twice around two multiplications (the 64-bit finaliser of MurmurHash3: 2087 homes, chains of up to 11).
    static __device__ __forceinline__ unsigned hash(unsigned long long k) {
        k ^= k >> 33;
        k *= 0xFF51AFD7ED558CCDull;
        k ^= k >> 33;
        k *= 0xC4CEB9FE1A85EC53ull;
        k ^= k >> 33;
        return (unsigned)k;
    }
    static __device__ __noinline__ void sink(const VpqLds& s, int kind, unsigned long long key, unsigned cnt);
    static __device__ __forceinline__ void pixel(VpqLds& s, const VpqArgs& a, mapcount::Run (&run)[3], unsigned& flags, int gs, int gi, int ps, int pi);
};

// one (key, count) into a set of tables at `base`.  SC: the scope of the atomics: agent for tables in global memory, workgroup for a
// window's tables in LDS.
template <int SC>
__device__ __forceinline__ void vpq_table_add_t(const VpqArgs& a, long long* base, int kind, unsigned long long key, unsigned long long cnt) {
    mapcount::table_add<SC, VpqLds>(base + a.t.keys[kind], reinterpret_cast<unsigned long long*>(base + a.t.counts[kind]), a.t.cap_mask[kind], key, cnt, a.header,
                                    a.t.full_bit[kind]);
}

__device__ void VpqLds::sink(const VpqLds& s, int kind, unsigned long long key, unsigned cnt) {
    vpq_table_add_t<__HIP_MEMORY_SCOPE_AGENT>(s.a, s.slot, kind, key, cnt);
}

// the slot of a key in a set of tables, -1 when it is not there (its count was dropped by a full table): mapcount::table_add's probes
template <int SC>
__device__ __forceinline__ int vpq_table_find(const VpqArgs& a, long long* base, int kind, unsigned long long key) {
    long long* keys = base + a.t.keys[kind];
    const unsigned mask = a.t.cap_mask[kind];
    unsigned i = VpqLds::hash(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe, i = (i + 1) & mask) {
        const long long cur = __hip_atomic_load(keys + i, __ATOMIC_RELAXED, SC);
        if (cur == (long long)key) return (int)i;
        if (cur == -1) return -1;
    }
    return -1;
}

// ----------------------------------------------------------------------------------------------------------------------- clear
// the ring slots of frames base + done .. + n - 1: keys -1, counts 0.  The first group of a call latches the frame base.
__global__ __launch_bounds__(256) void k_vpq_clear(VpqArgs a, int done, int n) {
    const unsigned f0 = (done == 0 ? a.header[1] : *a.base) + (unsigned)done;
    if (done == 0 && blockIdx.x == 0 && threadIdx.x == 0) *a.base = a.header[1];
    const size_t key_end[3] = {a.t.counts[K_GT], a.t.counts[K_PRED], a.t.counts[K_PAIR]};
    const size_t key_at[3] = {a.t.keys[K_GT], a.t.keys[K_PRED], a.t.keys[K_PAIR]};
    const size_t total = (size_t)n * a.slot_words;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t j = i / a.slot_words, w = i - j * a.slot_words;
        const bool key = (w >= key_at[0] && w < key_end[0]) || (w >= key_at[1] && w < key_end[1]) || (w >= key_at[2] && w < key_end[2]);
        a.ring[(size_t)((f0 + (unsigned)j) % (unsigned)a.R) * a.slot_words + w] = key ? -1ll : 0ll;
    }
}

// ----------------------------------------------------------------------------------------------------------------------- count
__device__ __forceinline__ void VpqLds::pixel(VpqLds& s, const VpqArgs& a, mapcount::Run (&run)[3], unsigned& flags, int gs, int gi, int ps, int pi) {
    const bool bad_class = (unsigned)ps >= (unsigned)a.num_cat || ((unsigned)gs >= (unsigned)a.num_cat && gs != a.ign);
    const bool bad_id = ((unsigned)gi >> a.shift) != 0 || ((unsigned)pi >> a.shift) != 0;      // negative ids have the top bit set
    if (bad_class) flags |= VKN_VPQ_STATUS_CLASS_RANGE;
    if (bad_id) flags |= VKN_VPQ_STATUS_ID_RANGE;
    const bool live = !bad_class && !bad_id;
    const unsigned long long yt = live ? ((unsigned long long)(unsigned)gs << a.shift) + (unsigned)gi : 0ull;
    const unsigned long long yp = live ? ((unsigned long long)(unsigned)ps << a.shift) + (unsigned)pi : 0ull;
    mapcount::push(s, run[K_PRED], live, (yp << 2) | K_PRED);
    mapcount::push(s, run[K_GT], live, (yt << 2) | K_GT);
    mapcount::push(s, run[K_PAIR], live, ((yt * (unsigned long long)a.offset + yp) << 2) | K_PAIR);
}

// grid: n * wpf workgroups, wpf per frame of the group; a workgroup walks `per` neighbouring spans of ITS frame and keeps its table in LDS
// over all of them.  The maps are the call's; frame j of the group is frame done + j of the call.
__global__ __launch_bounds__(VPQ_THREADS) void k_vpq_count(VpqArgs a, const int* __restrict__ gt_sem, const int* __restrict__ gt_ins,
                                                           const int* __restrict__ pred_sem, const int* __restrict__ pred_ins, int B, int HW,
                                                           int done, int n, int spans, int wpf, int per) {
    __shared__ VpqLds s;
    const int tid = threadIdx.x;
    const int j = blockIdx.x / wpf, chunk = blockIdx.x - j * wpf;
    mapcount::clear(s);
    if (tid == 0) {
        s.flags = 0;
        s.a = a;
        s.slot = a.ring + (size_t)((*a.base + (unsigned)(done + j)) % (unsigned)a.R) * a.slot_words;
    }
    __syncthreads();

    unsigned flags = 0;
    const size_t base = (size_t)(done + j) * HW;
    const int first = chunk * per, last = min(spans, first + per);
    for (int sp = first; sp < last; ++sp) {
        const int p0 = sp * VKN_VPQ_SPAN_PX, p1 = min(HW, p0 + VKN_VPQ_SPAN_PX);
        mapcount::walk(s, a, flags, gt_sem + base, gt_ins + base, pred_sem + base, pred_ins + base, p0, p1);
    }
    if (flags) atomicOr(&s.flags, flags);
    __syncthreads();

    mapcount::flush(s);
    if (tid == 0) {
        if (s.flags) __hip_atomic_fetch_or(a.header, s.flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the call's last group: nothing reads `frames` any more in this call (the windows read the latched base)
        if (blockIdx.x == 0 && done + n == B) __hip_atomic_fetch_add(a.header + 1, (unsigned)B, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------------------------------------------------- window
// grid: n * nk workgroups: frame j of the group, window length ks[i].  The window ends at the frame.  LDS: the window's tables fit the
// CU's 160 KiB and live there (workgroup-scope atomics, a barrier between the phases); otherwise they live in the state's scratch
// (agent-scope atomics, performed at L2, and an agent fence with the barrier).  Both forms run the same text.
template <int SC>
__device__ __forceinline__ long long vpq_ld(const long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, SC);
}
template <bool LDS>
__device__ __forceinline__ void vpq_phase() {
    if constexpr (!LDS) __threadfence();
    __syncthreads();
}

// what a window's workgroup keeps in LDS whichever place its tables have: the window's tp, fn, fp per class and its place in the log
struct VpqWinLds {
    unsigned cls[3][256];
    unsigned n_tp, n_written, log_base, log_room;
};
static_assert(sizeof(VpqWinLds) <= VPQ_WIN_STATIC_LDS && VKN_VPQ_MAX_CAT <= 256, "the window's static LDS");

template <bool LDS>
__global__ __launch_bounds__(VPQ_WIN_THREADS) void k_vpq_window(VpqArgs a, int done, int n) {
    extern __shared__ __attribute__((aligned(16))) char vpq_smem[];
    __shared__ VpqWinLds w;
    constexpr int SC = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
    const int tid = threadIdx.x;
    const int j = blockIdx.x / a.nk, i = blockIdx.x - j * a.nk;
    const unsigned f = *a.base + (unsigned)(done + j);
    const int k = a.ks[i];
    if (f + 1 < (unsigned)k) return;                                     // the sequence has no k frames yet (eval_dvpq_step.py:187)
    long long* S;
    if constexpr (LDS)
        S = reinterpret_cast<long long*>(vpq_smem);
    else
        S = a.scratch + (size_t)blockIdx.x * a.set_words;
    const VpqTables& t = a.t;
    const int cap[3] = {(int)t.cap_mask[0] + 1, (int)t.cap_mask[1] + 1, (int)t.cap_mask[2] + 1};

    // phase 0: empty window tables
    for (int x = tid; x < 3 * 256; x += VPQ_WIN_THREADS) w.cls[x >> 8][x & 255] = 0;
    if (tid == 0) w.n_tp = w.n_written = w.log_base = w.log_room = 0;
    for (int kind = 0; kind < 3; ++kind)
        for (int x = tid; x < cap[kind]; x += VPQ_WIN_THREADS) {
            __hip_atomic_store(S + t.keys[kind] + x, -1ll, __ATOMIC_RELAXED, SC);
            __hip_atomic_store(S + t.counts[kind] + x, 0ll, __ATOMIC_RELAXED, SC);
        }
    for (int x = tid; x < cap[K_PRED]; x += VPQ_WIN_THREADS) __hip_atomic_store(S + t.ign + x, 0ll, __ATOMIC_RELAXED, SC);
    vpq_phase<LDS>();

    // phase 1: the window's areas are the sums of its frames' areas (written by k_vpq_count, an earlier launch).  A lane takes slot x of
    // every frame of the window: the loads of all frames are in flight together, before the first insertion waits for one of them
    size_t frame_at[VKN_VPQ_MAX_K];
#pragma unroll
    for (int b = 0; b < VKN_VPQ_MAX_K; ++b) frame_at[b] = (size_t)((f - (unsigned)min(b, k - 1)) % (unsigned)a.R) * a.slot_words;
    for (int kind = 0; kind < 3; ++kind)
        for (int x = tid; x < cap[kind]; x += VPQ_WIN_THREADS) {
            long long key[VKN_VPQ_MAX_K], cnt[VKN_VPQ_MAX_K];
#pragma unroll
            for (int b = 0; b < VKN_VPQ_MAX_K; ++b) {
                key[b] = b < k ? a.ring[frame_at[b] + t.keys[kind] + x] : -1ll;
                cnt[b] = b < k ? a.ring[frame_at[b] + t.counts[kind] + x] : 0ll;
            }
#pragma unroll
            for (int b = 0; b < VKN_VPQ_MAX_K; ++b)
                if (key[b] != -1) vpq_table_add_t<SC>(a, S, kind, (unsigned long long)key[b], (unsigned long long)cnt[b]);
        }
    vpq_phase<LDS>();

    // phase 2: every intersection (eval_dvpq_step.py:63-79); an ignored gt id hands its overlap to the prediction (:53-58)
    const unsigned long long void_id = (unsigned long long)a.ign << a.shift;
    for (int x = tid; x < cap[K_PAIR]; x += VPQ_WIN_THREADS) {
        const long long key = vpq_ld<SC>(S + t.keys[K_PAIR] + x);
        if (key == -1) continue;
        const long long ia = vpq_ld<SC>(S + t.counts[K_PAIR] + x);
        const unsigned long long gt_id = (unsigned long long)key / (unsigned long long)a.offset, pred_id = (unsigned long long)key % (unsigned long long)a.offset;
        const int gcat = (int)(gt_id >> a.shift), pcat = (int)(pred_id >> a.shift);
        if (gcat != a.ign && gcat != pcat) continue;
        const int pslot = vpq_table_find<SC>(a, S, K_PRED, pred_id);
        if (pslot < 0) continue;                                         // dropped by a full table: already flagged
        if (gcat == a.ign) {
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(S + t.ign) + pslot, (unsigned long long)ia, __ATOMIC_RELAXED, SC);
            continue;
        }
        const int gslot = vpq_table_find<SC>(a, S, K_GT, gt_id);
        if (gslot < 0) continue;
        const int vslot = vpq_table_find<SC>(a, S, K_PAIR, void_id * (unsigned long long)a.offset + pred_id);
        const long long vo = vslot < 0 ? 0 : vpq_ld<SC>(S + t.counts[K_PAIR] + vslot);
        const long long ga = vpq_ld<SC>(S + t.counts[K_GT] + gslot) & (VPQ_MATCHED - 1), pa = vpq_ld<SC>(S + t.counts[K_PRED] + pslot) & (VPQ_MATCHED - 1);
        const long long uni = ga + pa - ia - vo;
        if (2 * ia > uni) {                                              // int / union > 0.5 (:74-75)
            atomicAdd(&w.cls[0][gcat], 1u);
            atomicAdd(&w.n_tp, 1u);
            __hip_atomic_fetch_or(S + t.counts[K_GT] + gslot, VPQ_MATCHED, __ATOMIC_RELAXED, SC);
            __hip_atomic_fetch_or(S + t.counts[K_PRED] + pslot, VPQ_MATCHED, __ATOMIC_RELAXED, SC);
            // the pair's count becomes its record: int below, union - int + 1 (never 0) above; nobody else reads this slot (a void
            // overlap is read from a pair whose gt class is ign_id, and that is never a true positive)
            __hip_atomic_store(S + t.counts[K_PAIR] + x, ia | ((uni - ia + 1) << 32), __ATOMIC_RELAXED, SC);
        }
    }
    vpq_phase<LDS>();
    // one reservation in the log for all of the window's records; what does not fit is dropped and flagged, and log_used stays the
    // number of records written
    if (tid == 0 && w.n_tp) {
        const unsigned at = __hip_atomic_fetch_add(a.header + 2, w.n_tp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned room = at >= (unsigned)a.cap_log ? 0u : min(w.n_tp, (unsigned)a.cap_log - at);
        if (room < w.n_tp) {
            __hip_atomic_fetch_sub(a.header + 2, w.n_tp - room, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_or(a.header, VKN_VPQ_STATUS_FULL_LOG, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        w.log_base = at;
        w.log_room = room;
    }
    __syncthreads();

    // phase 3: the records, and what found no partner (eval_dvpq_step.py:81-95)
    if (w.n_tp)
        for (int x = tid; x < cap[K_PAIR]; x += VPQ_WIN_THREADS) {
            const unsigned long long v = (unsigned long long)vpq_ld<SC>(S + t.counts[K_PAIR] + x);
            if ((v >> 32) == 0) continue;                                // areas of one window are below 2^32: not a true positive
            const unsigned r = atomicAdd(&w.n_written, 1u);
            if (r >= w.log_room) continue;
            long long* rec = a.log + (size_t)(w.log_base + r) * 4;
            const long long ia = (long long)(v & 0xFFFFFFFFull);
            rec[0] = ((long long)i << 48) | (long long)(f + 1 - (unsigned)k);
            rec[1] = vpq_ld<SC>(S + t.keys[K_PAIR] + x);
            rec[2] = ia;
            rec[3] = ia + (long long)(v >> 32) - 1;
        }
    for (int x = tid; x < cap[K_GT]; x += VPQ_WIN_THREADS) {
        const long long key = vpq_ld<SC>(S + t.keys[K_GT] + x);
        if (key == -1) continue;
        const int cat = (int)((unsigned long long)key >> a.shift);
        if ((vpq_ld<SC>(S + t.counts[K_GT] + x) & VPQ_MATCHED) || cat == a.ign) continue;
        atomicAdd(&w.cls[1][cat], 1u);
    }
    for (int x = tid; x < cap[K_PRED]; x += VPQ_WIN_THREADS) {
        const long long key = vpq_ld<SC>(S + t.keys[K_PRED] + x);
        if (key == -1) continue;
        const long long area = vpq_ld<SC>(S + t.counts[K_PRED] + x);
        if ((area & VPQ_MATCHED) || 2 * vpq_ld<SC>(S + t.ign + x) > area) continue;
        atomicAdd(&w.cls[2][(int)((unsigned long long)key >> a.shift)], 1u);
    }
    __syncthreads();
    // the window's tp, fn, fp per class: one add per class that has any
    for (int x = tid; x < 3 * a.num_cat; x += VPQ_WIN_THREADS) {
        const int r = x / a.num_cat, c = x - r * a.num_cat;
        if (w.cls[r][c]) __hip_atomic_fetch_add(a.acc + ((size_t)i * 3 + r) * a.num_cat + c, (unsigned long long)w.cls[r][c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

extern "C" {

size_t vkn_sizeof_vpq_cfg(void) { return sizeof(VknVpqCfg); }

size_t vkn_vpq_state_bytes(const VknVpqCfg* cfg) {
    if (!cfg || vpq_check_cfg(cfg) != VKN_OK) return 0;
    return vpq_layout(cfg).bytes;
}

int vkn_vpq_state_layout(const VknVpqCfg* cfg, size_t* offsets4) {
    if (!cfg || !offsets4) return VKN_E_ARG;
    const int rc = vpq_check_cfg(cfg);
    if (rc != VKN_OK) return rc;
    const VpqLayout l = vpq_layout(cfg);
    for (int i = 0; i < 4; ++i) offsets4[i] = l.off[i];
    return VKN_OK;
}

int vkn_vpq_reset(const VknVpqCfg* cfg, void* state, size_t state_bytes, void* stream) {
    if (!cfg || !state) return VKN_E_ARG;
    const int rc = vpq_check_cfg(cfg);
    if (rc != VKN_OK) return rc;
    const VpqLayout l = vpq_layout(cfg);
    if (state_bytes != l.bytes) return VKN_E_WORKSPACE;
    if (!vkn_aligned(state, 16)) return VKN_E_ALIGN;
    if (!vkn_on_device(state)) return VKN_E_ARG;
    // all zero: the ring slots and the windows' scratch are emptied by the kernels that use them
    if (hipMemsetAsync(state, 0, l.bytes, static_cast<hipStream_t>(stream)) != hipSuccess) return VKN_E_LAUNCH;
    return VKN_OK;
}

int vkn_vpq_update_i32(const VknVpqCfg* cfg, void* state, size_t state_bytes, const int* gt_sem, const int* gt_ins, const int* pred_sem,
                       const int* pred_ins, int B, int HW, void* stream) {
    if (!cfg || !state || !gt_sem || !gt_ins || !pred_sem || !pred_ins || B < 0 || HW < 0) return VKN_E_ARG;
    const int rc = vpq_check_cfg(cfg);
    if (rc != VKN_OK) return rc;
    if (B < 1 || HW < 1 || (long long)B * HW * 4 >= (1ll << 31)) return VKN_E_SHAPE;
    const VpqLayout l = vpq_layout(cfg);
    if (state_bytes != l.bytes) return VKN_E_WORKSPACE;
    if (!vkn_aligned(state, 16) || !vkn_aligned(gt_sem, 4) || !vkn_aligned(gt_ins, 4) || !vkn_aligned(pred_sem, 4) || !vkn_aligned(pred_ins, 4))
        return VKN_E_ALIGN;
    if (!vkn_on_device(state) || !vkn_on_device(gt_sem) || !vkn_on_device(gt_ins) || !vkn_on_device(pred_sem) || !vkn_on_device(pred_ins))
        return VKN_E_ARG;
    char* base = static_cast<char*>(state);
    VpqArgs a;
    a.header = reinterpret_cast<unsigned*>(base + l.off[0]);
    a.acc = reinterpret_cast<unsigned long long*>(base + l.off[1]);
    a.log = reinterpret_cast<long long*>(base + l.off[2]);
    a.base = reinterpret_cast<unsigned*>(base + l.off[3]);
    a.ring = reinterpret_cast<long long*>(base + l.ring);
    a.scratch = reinterpret_cast<long long*>(base + l.scratch);
    a.t = vpq_tables(cfg);
    a.slot_words = l.slot_words;
    a.set_words = l.set_words;
    a.offset = cfg->offset;
    a.num_cat = cfg->num_cat;
    a.ign = cfg->ign_id;
    a.shift = cfg->label_bit_shift;
    a.nk = cfg->nk;
    for (int i = 0; i < VKN_VPQ_MAX_KS; ++i) a.ks[i] = i < cfg->nk ? cfg->ks[i] : 0;
    a.cap_log = cfg->cap_log;
    a.R = l.R;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int spans = (HW + VKN_VPQ_SPAN_PX - 1) / VKN_VPQ_SPAN_PX;
    for (int done = 0; done < B; done += VKN_VPQ_GROUP) {
        const int n = B - done < VKN_VPQ_GROUP ? B - done : VKN_VPQ_GROUP;
        const size_t words = (size_t)n * l.slot_words;
        const int cgrid = (int)((words + 1023) / 1024 < 1024 ? (words + 1023) / 1024 : 1024);
        hipLaunchKernelGGL(k_vpq_clear, dim3(cgrid), dim3(256), 0, st, a, done, n);
        VKN_CHECK_LAUNCH();
        const int room = VKN_VPQ_MAX_GRID / n;                                       // workgroups a frame may have
        const int per = (spans + room - 1) / room, wpf = (spans + per - 1) / per;
        hipLaunchKernelGGL(k_vpq_count, dim3(n * wpf), dim3(VPQ_THREADS), 0, st, a, gt_sem, gt_ins, pred_sem, pred_ins, B, HW, done, n, spans,
                           wpf, per);
        VKN_CHECK_LAUNCH();
        if (l.set_words * 8 <= VPQ_LDS_BYTES) {
            VKN_ALLOW_FULL_LDS(k_vpq_window<true>);
            hipLaunchKernelGGL(k_vpq_window<true>, dim3(n * cfg->nk), dim3(VPQ_WIN_THREADS), l.set_words * 8, st, a, done, n);
        } else {
            hipLaunchKernelGGL(k_vpq_window<false>, dim3(n * cfg->nk), dim3(VPQ_WIN_THREADS), 0, st, a, done, n);
        }
        VKN_CHECK_LAUNCH();
    }
    return VKN_OK;
}

}  // extern "C"
