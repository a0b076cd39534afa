// vkn_mapcount.h — the counting engine of the map meters (vkn_stq.hip, vkn_vpq.hip): how (key, count) pairs get from the pixels of four
// int32 maps into open-addressing tables in global memory.  Include after vkn_common.h.
//
// Traffic is 16 bytes per pixel and nothing else may scale with the pixels: a workgroup walks spans of SPAN_PX contiguous pixels of one
// frame, a lane loads four neighbouring pixels of each map with one 16-byte load (where that map is aligned behind the span's peel) and
// keeps, per kind of count, a running (key, count) in registers that it only hands on when the key changes.  What it hands on goes into
// ONE table in LDS (SLOTS slots: a 64-bit key that carries the 2-bit kind, a 32-bit count), first summed over the lanes of the wave that
// hold the same key.  When the workgroup has walked its spans every occupied slot goes to the meter's tables in global memory; a key that
// finds no slot in LDS within LDS_PROBES goes there itself: correct, only slower.
//
// A meter supplies ONE type P, the workgroup's state in LDS, that is also the engine's policy:
//     static constexpr int KINDS, SLOTS, THREADS, SPAN_PX;
//     unsigned long long keys[SLOTS]; unsigned counts[SLOTS];      // the 12-byte slot as two arrays
//     static unsigned hash(unsigned long long);                    // forced inline: of LDS slots and of global slots alike
//     static void sink(const P&, int kind, unsigned long long key, unsigned cnt);      // __noinline__: one count into global memory
//     static void pixel(P&, const A& args, Run (&)[KINDS], unsigned& flags, int gt_sem, int gt_ins, int pred_sem, int pred_ins);
// `pixel`, forced inline, says what a pixel means: one `push` per kind.  Keys stay below 2^62, and a meter's kind 3, if it has one, has
// small keys, so no tagged key is EMPTY.  `emit`, `push` and `walk` are forced inline, `lds_add` is left to the compiler (it inlines it)
// and `sink` is kept out of it: the kernels' registers and timing depend on this shape (profiles/mapcount_resources.txt).
#pragma once

namespace mapcount {

constexpr int LDS_PROBES = 32;                 // slots tried in LDS before a count goes to global memory directly
constexpr unsigned long long EMPTY = ~0ull;
constexpr int CNT_BITS = 6;                    // a lane counts at most SPAN_PX / THREADS body pixels + 1 head or tail pixel

struct Run {
    unsigned long long key;
    unsigned cnt;
};

// One (key, count) into a table of mask + 1 slots: the key slot by compare-and-swap (-1 = empty), linear probing over at most all slots,
// then the count.  A full table drops the count and sets `full_bit` in the state's status word.  SCOPE: of the table's atomics, agent for a
// table in global memory, workgroup for one in LDS.  The bit is raised here, behind the loop, and not by the caller on a returned flag:
// with the flag k_vpq_window took 5 more VGPRs and a B = 1 update of the VPQ meter 2 % longer (profiles/mapcount_resources.txt,
// profiles/mapcount_ab.txt).
template <int SCOPE, class Hash>
__device__ __forceinline__ void table_add(long long* keys, unsigned long long* counts, unsigned mask, unsigned long long key, unsigned long long cnt, unsigned* status,
                                          unsigned full_bit) {
    unsigned i = Hash::hash(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe, i = (i + 1) & mask) {
        long long cur = __hip_atomic_load(keys + i, __ATOMIC_RELAXED, SCOPE);
        if (cur == -1) {
            long long expect = -1;
            if (__hip_atomic_compare_exchange_strong(keys + i, &expect, (long long)key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE))
                cur = (long long)key;
            else
                cur = expect;                        // another wave took the slot: perhaps with this very key
        }
        if (cur == (long long)key) {
            __hip_atomic_fetch_add(counts + i, cnt, __ATOMIC_RELAXED, SCOPE);
            return;
        }
    }
    __hip_atomic_fetch_or(status, full_bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <class P>
__device__ __forceinline__ void clear(P& s) {
    for (int i = threadIdx.x; i < P::SLOTS; i += P::THREADS) {
        s.keys[i] = EMPTY;
        s.counts[i] = 0;
    }
}

// one tagged (key, count) into the workgroup's table
template <class P>
__device__ void lds_add(P& s, unsigned long long tagged, unsigned cnt) {
    static_assert((P::SLOTS & (P::SLOTS - 1)) == 0, "table geometry");
    unsigned i = P::hash(tagged) & (P::SLOTS - 1);
    for (int probe = 0; probe < LDS_PROBES; ++probe, i = (i + 1) & (P::SLOTS - 1)) {
        const unsigned long long old = atomicCAS(&s.keys[i], EMPTY, tagged);
        if (old == EMPTY || old == tagged) {
            atomicAdd(&s.counts[i], cnt);
            return;
        }
    }
    P::sink(s, (int)(tagged & 3), tagged >> 2, cnt);
}

// Lanes that hand on a count at the same point: the lanes that hold the first such lane's key are summed (a lane's count has CNT_BITS
// bits: one ballot per bit) and that lane alone adds the sum; the others add their own.
template <class P>
__device__ __forceinline__ void emit(P& s, bool e, unsigned long long tagged, unsigned cnt) {
    static_assert(P::SPAN_PX / P::THREADS + 1 < (1 << CNT_BITS), "a lane's run count must fit CNT_BITS");
    if (e) {
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)tagged), hi = __builtin_amdgcn_readfirstlane((unsigned)(tagged >> 32));
        const bool match = tagged == (((unsigned long long)hi << 32) | lo);
        const unsigned long long mm = __ballot(match);
        unsigned sum = 0;
#pragma unroll
        for (int b = 0; b < CNT_BITS; ++b) sum += (unsigned)__popcll(__ballot(match && ((cnt >> b) & 1))) << b;
        const int lane = threadIdx.x & 63;
        if (match) {
            if (lane == __ffsll((long long)mm) - 1) lds_add(s, tagged, sum);
        } else {
            lds_add(s, tagged, cnt);
        }
    }
}

template <class P>
__device__ __forceinline__ void push(P& s, Run& r, bool valid, unsigned long long tagged) {
    const bool change = valid && r.key != tagged;
    emit(s, change && r.cnt > 0, r.key, r.cnt);
    if (change) {
        r.key = tagged;
        r.cnt = 0;
    }
    r.cnt += valid ? 1u : 0u;
}

// the pixels [p0, p1), at most SPAN_PX, of one frame's four maps
template <class P, class A>
__device__ __forceinline__ void walk(P& s, const A& a, unsigned& flags, const int* m0, const int* m1, const int* m2, const int* m3, int p0, int p1) {
    static_assert(P::SPAN_PX % (4 * P::THREADS) == 0, "span geometry");
    const int tid = threadIdx.x;
    // the peel: pixels in front of m0's first 16-byte boundary inside the span; a map that is aligned differently is loaded by words
    const int mis = (int)((reinterpret_cast<uintptr_t>(m0 + p0) >> 2) & 3);
    const int head = min((4 - mis) & 3, p1 - p0);
    const int q0 = p0 + head, groups = (p1 - q0) >> 2, q1 = q0 + 4 * groups;
    const bool v1 = ((reinterpret_cast<uintptr_t>(m1 + q0)) & 15) == 0, v2 = ((reinterpret_cast<uintptr_t>(m2 + q0)) & 15) == 0,
               v3 = ((reinterpret_cast<uintptr_t>(m3 + q0)) & 15) == 0;

    Run run[P::KINDS];
#pragma unroll
    for (int k = 0; k < P::KINDS; ++k) run[k] = Run{EMPTY, 0u};

    // head and tail pixels (fewer than 4 each), one per lane
    {
        const int p = tid < head ? p0 + tid : q1 + (tid - head);
        if (p < p1 && (tid < head || p >= q1)) P::pixel(s, a, run, flags, m0[p], m1[p], m2[p], m3[p]);
    }
    for (int g = tid; g < groups; g += P::THREADS) {
        const int p = q0 + 4 * g;
        const int4 x0 = *reinterpret_cast<const int4*>(m0 + p);
        const int4 x1 = v1 ? *reinterpret_cast<const int4*>(m1 + p) : make_int4(m1[p], m1[p + 1], m1[p + 2], m1[p + 3]);
        const int4 x2 = v2 ? *reinterpret_cast<const int4*>(m2 + p) : make_int4(m2[p], m2[p + 1], m2[p + 2], m2[p + 3]);
        const int4 x3 = v3 ? *reinterpret_cast<const int4*>(m3 + p) : make_int4(m3[p], m3[p + 1], m3[p + 2], m3[p + 3]);
        P::pixel(s, a, run, flags, x0.x, x1.x, x2.x, x3.x);
        P::pixel(s, a, run, flags, x0.y, x1.y, x2.y, x3.y);
        P::pixel(s, a, run, flags, x0.z, x1.z, x2.z, x3.z);
        P::pixel(s, a, run, flags, x0.w, x1.w, x2.w, x3.w);
    }
#pragma unroll
    for (int k = 0; k < P::KINDS; ++k) emit(s, run[k].cnt > 0, run[k].key, run[k].cnt);      // per span: a lane's count stays in CNT_BITS
}

// every occupied slot of the workgroup's table, after a barrier behind the last walk
template <class P>
__device__ __forceinline__ void flush(const P& s) {
    for (int i = threadIdx.x; i < P::SLOTS; i += P::THREADS) {
        const unsigned long long tagged = s.keys[i];
        if (tagged != EMPTY) P::sink(s, (int)(tagged & 3), tagged >> 2, s.counts[i]);
    }
}

}  // namespace mapcount
