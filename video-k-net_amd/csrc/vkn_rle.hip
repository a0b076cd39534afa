// vkn_rle.hip — COCO run-length encoding of instance masks on the device (include/vkn_rle.h): counts, strings, area and bbox of K
// masks [H][W] in eight launches, integer arithmetic only.
//
// The input is row-major, the RLE order column-major (p = x * H + y).  A workgroup owns a STRIP of VKN_RLE_STRIP_COLS = 64 columns of one
// mask, so that one row of a strip is one 64-bit word:
//   1. k_rle_pack     (vkn_maskbits.h, shared with vkn_maskap.hip) reads the input ONCE, in aligned 16-byte pieces whatever W is, and
//                     stores the masks as bits [K][strips][H].  Every later launch reads those words only: 1/8 of the u8 input, 1/32 of
//                     the fp32 input.
//   2. k_rle_count    per strip: thread (segment w of 4, column c of 64) walks its quarter of column c downwards; a transition at (y, x)
//                     is bit c of bits[y] ^ bits[y-1], row 0 against the LAST row of column x - 1 (the word before the strip's first
//                     word is the previous strip's last row).  Per strip: the number of transitions and the positions of its last three,
//                     area, bbox.
//   3. k_rle_scan_mask / 4. k_rle_scan_all   strips within a mask, then masks: run offsets, nruns, area, bbox into the records.
//   5. k_rle_len      per strip, knowing the three transitions before each thread's first: bytes of its runs.
//   6. k_rle_scan_mask / 7. k_rle_scan_all   the same two scans over bytes.
//   8. k_rle_emit     per strip: the counts into the run pool, the strings into the byte pool, nothing at or beyond a capacity.
// Every hand-off between workgroups is a kernel boundary: no workgroup waits for another inside a launch.  What a thread needs to know of
// the transitions before its own is a small state (how many, and the positions of the last three: run i's byte code needs counts[i] and
// counts[i-2], four positions), and "append" on such states is associative, so one block scan serves transitions and bytes alike.
#include "../../include/vkn_rle.h"
#include "../../include/vkn_instmask.h"   // vkn_bits_rle_encode: this encoder on bits that the caller already holds
#include "vkn_common.h"
#include "vkn_maskbits.h"
#include <limits.h>

namespace {

constexpr int RLE_THREADS = MASKBITS_THREADS;
constexpr int RLE_SEGS = RLE_THREADS / VKN_RLE_STRIP_COLS;      // row segments of a strip: one wave each
constexpr int RLE_CHUNK = 256;                                  // rows of its segment that a wave holds in LDS at a time
static_assert(VKN_RLE_STRIP_COLS == 64 && VKN_RLE_STRIP_COLS == MASKBITS_STRIP_COLS && RLE_SEGS == 4, "a strip row is one 64-bit word, a wave walks one row segment");

// What is known of a sequence of transitions: how many, and the positions of the last three (0 where there are fewer: p[-1] = 0 is the
// format's start, and the others are read only behind three real transitions).
struct St {
    unsigned n, p1, p2, p3;
};
__device__ __forceinline__ St st_id() { return St{0u, 0u, 0u, 0u}; }
// a, then b
__device__ __forceinline__ St st_cat(const St& a, const St& b) {
    St r;
    r.n = a.n + b.n;
    if (b.n >= 3) {
        r.p1 = b.p1, r.p2 = b.p2, r.p3 = b.p3;
    } else if (b.n == 2) {
        r.p1 = b.p1, r.p2 = b.p2, r.p3 = a.p1;
    } else if (b.n == 1) {
        r.p1 = b.p1, r.p2 = a.p1, r.p3 = a.p2;
    } else {
        r.p1 = a.p1, r.p2 = a.p2, r.p3 = a.p3;
    }
    return r;
}
__device__ __forceinline__ void st_push(St& s, unsigned p) {
    s.p3 = s.p2, s.p2 = s.p1, s.p1 = p;
    ++s.n;
}
// the run that ends at position p (a transition, or H * W for the last run): its count, and x = count - counts[i-2] behind run 2
__device__ __forceinline__ long long st_delta(const St& s, unsigned p, unsigned& count) {
    count = p - s.p1;
    return s.n > 2 ? (long long)count - (long long)(s.p2 - s.p3) : (long long)count;
}

// bytes of x in the string; written to dst[at ..) below cap when dst is given
__device__ __forceinline__ unsigned rle_code(long long x, unsigned char* dst, unsigned long long at, unsigned long long cap) {
    unsigned n = 0;
    bool more;
    do {
        int c = (int)(x & 31);
        x >>= 5;
        more = (c & 16) ? (x != -1) : (x != 0);
        if (more) c |= 32;
        if (dst && at + n < cap) dst[at + n] = (unsigned char)(c + 48);
        ++n;
    } while (more);
    return n;
}

// Exclusive scan of 256 states in the order of `e` (a permutation of the threads), behind `seed`: returns seed + every entry before e;
// total = seed + all.  Every thread of the workgroup calls it.
__device__ __forceinline__ St block_scan(St* sh, int e, const St& v, const St& seed, St& total) {
    const int t = threadIdx.x;
    sh[e] = v;
    __syncthreads();
    St x = sh[t];
    for (int d = 1; d < RLE_THREADS; d <<= 1) {
        St y = st_id();
        if (t >= d) y = sh[t - d];
        __syncthreads();
        if (t >= d) x = st_cat(y, x);
        sh[t] = x;
        __syncthreads();
    }
    const St excl = e > 0 ? st_cat(seed, sh[e - 1]) : seed;
    total = st_cat(seed, sh[RLE_THREADS - 1]);
    __syncthreads();
    return excl;
}

// ------------------------------------------------------------------------------------------------------------------------ walks
struct Strip {
    const unsigned long long* B;      // bits of the strip's rows
    unsigned long long top;           // what row 0 is compared with: the last row one column to the left
    int H, x0, sw;
};
__device__ __forceinline__ Strip strip_open(const unsigned long long* __restrict__ bits, int H, int W) {
    const int s = blockIdx.x, k = blockIdx.y;
    Strip st;
    st.B = bits + ((size_t)k * gridDim.x + s) * (size_t)H;
    st.H = H;
    st.x0 = s * VKN_RLE_STRIP_COLS;
    st.sw = min(VKN_RLE_STRIP_COLS, W - st.x0);
    const unsigned long long carry = s > 0 ? st.B[-1] >> 63 : 0ull;          // the previous strip is full: its column 63, last row
    st.top = (st.B[H - 1] << 1) | carry;
    return st;
}
// thread (w, c) walks rows [w * seg, (w + 1) * seg) of column c: tr(p) at every transition and, with PIXELS, px(y, word) per 64 rows
// from y on with the column's pixels as bits.  The words come through LDS, RLE_CHUNK rows per wave at a time: a wave loads its chunk
// with 64 independent coalesced loads in flight and then reads one word per row, the same address in every lane (a broadcast).  A
// lane first gathers its column's transitions of 64 rows into one word, a few operations per row that every lane shares, and only then
// visits its own set bits: the work per transition (a byte code, stores) is paid per transition of the busiest lane, not once per row
// in which any of the 64 columns changes.  Every thread of the workgroup calls it (barriers inside), whatever its column.
template <bool PIXELS, class TR, class PX>
__device__ __forceinline__ void strip_walk(const Strip& st, unsigned long long* rows, TR&& tr, PX&& px) {
    const int c = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long seg = (st.H - 1) / RLE_SEGS + 1;
    const long long y0 = w * seg, y1 = min((long long)st.H, y0 + seg);
    const bool active = c < st.sw;
    unsigned long long* mine = rows + w * RLE_CHUNK;
    unsigned long long prev = y0 >= y1 ? 0ull : y0 ? st.B[y0 - 1] : st.top;
    const unsigned p0 = (unsigned)(st.x0 + c) * (unsigned)st.H + (unsigned)y0;     // (used by active lanes with y0 < y1 only)
    for (long long off = 0; off < seg; off += RLE_CHUNK) {                  // the same trip count in every wave
        __syncthreads();
        for (int i = c; i < RLE_CHUNK; i += 64)
            if (y0 + off + i < y1) mine[i] = st.B[y0 + off + i];
        __syncthreads();
        if (!active) continue;
        const int n = (int)min((long long)RLE_CHUNK, y1 - y0 - off);        // <= 0 behind the wave's last row
        for (int g = 0; g < n; g += 64) {
            const int m = min(64, n - g);
            unsigned long long tw = 0, pw = 0;
            for (int i = 0; i < m; ++i) {
                const unsigned long long cur = mine[g + i];
                tw |= (((cur ^ prev) >> c) & 1ull) << i;
                if (PIXELS) pw |= ((cur >> c) & 1ull) << i;
                prev = cur;
            }
            const unsigned pg = p0 + (unsigned)(off + g);
            while (tw) {
                tr(pg + (unsigned)__builtin_ctzll(tw));
                tw &= tw - 1;
            }
            if (PIXELS && pw) px((int)(y0 + off + g), pw);
        }
    }
}
// the order of the RLE inside a strip: column by column, a column's segments downwards
__device__ __forceinline__ int strip_entry() { return (threadIdx.x & 63) * RLE_SEGS + (threadIdx.x >> 6); }
__device__ __forceinline__ St strip_count(const Strip& st, unsigned long long* rows) {
    St v = st_id();
    strip_walk<false>(st, rows, [&](unsigned p) { st_push(v, p); }, [](int, unsigned long long) {});
    return v;
}

struct RleStat {
    int area, x0, x1, y0, y1, pad[3];
};

// grid (strips, K)
__global__ __launch_bounds__(RLE_THREADS) void k_rle_count(const unsigned long long* __restrict__ bits, St* __restrict__ sum, RleStat* __restrict__ stat,
                                                           int H, int W) {
    __shared__ St sh[RLE_THREADS];
    __shared__ unsigned long long rows[RLE_SEGS * RLE_CHUNK];
    __shared__ int s_area, s_x0, s_x1, s_y0, s_y1;
    if (threadIdx.x == 0) s_area = 0, s_x0 = INT_MAX, s_x1 = -1, s_y0 = INT_MAX, s_y1 = -1;
    const Strip st = strip_open(bits, H, W);
    St v = st_id();
    int area = 0, y0 = INT_MAX, y1 = -1;
    strip_walk<true>(st, rows, [&](unsigned p) { st_push(v, p); },
                     [&](int y, unsigned long long word) {
                         area += __builtin_popcountll(word);
                         y0 = min(y0, y + (int)__builtin_ctzll(word));
                         y1 = max(y1, y + 63 - (int)__builtin_clzll(word));
                     });
    St total;
    block_scan(sh, strip_entry(), v, st_id(), total);            // (its barriers order s_* too)
    if (area) {
        const int x = st.x0 + (threadIdx.x & 63);
        atomicAdd(&s_area, area);
        atomicMin(&s_x0, x);
        atomicMax(&s_x1, x);
        atomicMin(&s_y0, y0);
        atomicMax(&s_y1, y1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t idx = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        sum[idx] = total;
        stat[idx] = RleStat{s_area, s_x0, s_x1, s_y0, s_y1, {0, 0, 0}};
    }
}

// grid K.  MODE 0: strips' transition states -> the state before each strip, the mask's transitions, area and bbox into its record.
// MODE 1: strips' bytes -> byte offset of each strip inside the mask, the mask's bytes.
template <int MODE>
__global__ __launch_bounds__(RLE_THREADS) void k_rle_scan_mask(const St* __restrict__ sum, St* __restrict__ state, const RleStat* __restrict__ stat,
                                                               const unsigned* __restrict__ sbytes, unsigned* __restrict__ sboff,
                                                               unsigned* __restrict__ tot, int* __restrict__ records, long long NS) {
    __shared__ St sh[RLE_THREADS];
    __shared__ int s_area, s_x0, s_x1, s_y0, s_y1;
    const int k = blockIdx.x, t = threadIdx.x;
    if (t == 0) s_area = 0, s_x0 = INT_MAX, s_x1 = -1, s_y0 = INT_MAX, s_y1 = -1;
    St carry = st_id();
    int area = 0, x0 = INT_MAX, x1 = -1, y0 = INT_MAX, y1 = -1;
    for (long long base = 0; base < NS; base += RLE_THREADS) {
        const long long j = base + t;
        const size_t idx = (size_t)k * NS + j;
        St v = st_id();
        if (j < NS) {
            if (MODE == 0) {
                v = sum[idx];
                const RleStat q = stat[idx];
                area += q.area;
                x0 = min(x0, q.x0), x1 = max(x1, q.x1), y0 = min(y0, q.y0), y1 = max(y1, q.y1);
            } else {
                v.n = sbytes[idx];
            }
        }
        St total;
        const St excl = block_scan(sh, t, v, carry, total);
        if (j < NS) {
            if (MODE == 0)
                state[idx] = excl;
            else
                sboff[idx] = excl.n;
        }
        carry = total;
    }
    if (MODE == 0) {
        __syncthreads();
        if (area) {
            atomicAdd(&s_area, area);
            atomicMin(&s_x0, x0);
            atomicMax(&s_x1, x1);
            atomicMin(&s_y0, y0);
            atomicMax(&s_y1, y1);
        }
        __syncthreads();
        if (t == 0) {
            int* rec = records + (size_t)k * VKN_RLE_RECORD_INTS;
            const bool any = s_area > 0;
            rec[VKN_RLE_REC_AREA] = s_area;
            rec[VKN_RLE_REC_BBOX + 0] = any ? s_x0 : 0;
            rec[VKN_RLE_REC_BBOX + 1] = any ? s_y0 : 0;
            rec[VKN_RLE_REC_BBOX + 2] = any ? s_x1 - s_x0 + 1 : 0;
            rec[VKN_RLE_REC_BBOX + 3] = any ? s_y1 - s_y0 + 1 : 0;
        }
    }
    if (t == 0) tot[2 * k + MODE] = carry.n;
}

// one workgroup.  MODE 0: nruns = transitions + 1 and run offsets; MODE 1: nbytes and byte offsets.  The pool's FULL bit.
template <int MODE>
__global__ __launch_bounds__(RLE_THREADS) void k_rle_scan_all(const unsigned* __restrict__ tot, int* __restrict__ records, int K, unsigned cap,
                                                              unsigned* __restrict__ status) {
    __shared__ St sh[RLE_THREADS];
    const int t = threadIdx.x;
    St carry = st_id();
    for (int base = 0; base < K; base += RLE_THREADS) {
        const int k = base + t;
        St v = st_id();
        if (k < K) v.n = tot[2 * k + MODE] + (MODE == 0 ? 1u : 0u);
        St total;
        const St excl = block_scan(sh, t, v, carry, total);
        if (k < K) {
            int* rec = records + (size_t)k * VKN_RLE_RECORD_INTS;
            rec[MODE == 0 ? VKN_RLE_REC_NRUNS : VKN_RLE_REC_NBYTES] = (int)v.n;
            rec[MODE == 0 ? VKN_RLE_REC_RUN_OFF : VKN_RLE_REC_BYTE_OFF] = (int)excl.n;
        }
        carry = total;
    }
    if (t == 0 && carry.n > cap) atomicOr(status, MODE == 0 ? VKN_RLE_STATUS_FULL_RUNS : VKN_RLE_STATUS_FULL_BYTES);
}

// The runs a thread ends, behind the state `s` before its first transition: every transition of its walk and, for the thread that comes
// last in the mask's order (entry 255 of the last strip: its state after the walk is the mask's), the last run, which ends at H * W.
// Returns their bytes; with `runs` / `bytes` given, writes them (mask-relative pools, nothing at or beyond a capacity).
__device__ __forceinline__ unsigned strip_runs(const Strip& st, unsigned long long* rows, St s, bool last_strip, unsigned hw, unsigned* runs, unsigned long long run_off,
                                               unsigned long long cap_runs, unsigned char* bytes, unsigned long long at,
                                               unsigned long long cap_bytes) {
    unsigned len = 0;
    auto run = [&](unsigned p) {
        unsigned count;
        const long long x = st_delta(s, p, count);
        if (runs && run_off + s.n < cap_runs) runs[run_off + s.n] = count;
        len += rle_code(x, bytes, at + len, cap_bytes);
        st_push(s, p);
    };
    strip_walk<false>(st, rows, run, [](int, unsigned long long) {});
    if (last_strip && strip_entry() == RLE_THREADS - 1) run(hw);
    return len;
}

// grid (strips, K)
__global__ __launch_bounds__(RLE_THREADS) void k_rle_len(const unsigned long long* __restrict__ bits, const St* __restrict__ state,
                                                         unsigned* __restrict__ sbytes, int H, int W) {
    __shared__ St sh[RLE_THREADS];
    __shared__ unsigned long long rows[RLE_SEGS * RLE_CHUNK];
    const Strip st = strip_open(bits, H, W);
    const size_t idx = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int e = strip_entry();
    St total;
    const St before = block_scan(sh, e, strip_count(st, rows), state[idx], total);
    St v = st_id();
    v.n = strip_runs(st, rows, before, blockIdx.x == gridDim.x - 1, (unsigned)H * (unsigned)W, nullptr, 0, 0, nullptr, 0, 0);
    block_scan(sh, e, v, st_id(), total);
    if (threadIdx.x == 0) sbytes[idx] = total.n;
}

// grid (strips, K)
__global__ __launch_bounds__(RLE_THREADS) void k_rle_emit(const unsigned long long* __restrict__ bits, const St* __restrict__ state,
                                                          const unsigned* __restrict__ sboff, const int* __restrict__ records,
                                                          unsigned* __restrict__ runs, unsigned cap_runs, unsigned char* __restrict__ bytes,
                                                          unsigned cap_bytes, int H, int W) {
    __shared__ St sh[RLE_THREADS];
    __shared__ unsigned long long rows[RLE_SEGS * RLE_CHUNK];
    const Strip st = strip_open(bits, H, W);
    const size_t idx = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int e = strip_entry();
    const bool last = blockIdx.x == gridDim.x - 1;
    const unsigned hw = (unsigned)H * (unsigned)W;
    const int* rec = records + (size_t)blockIdx.y * VKN_RLE_RECORD_INTS;
    const unsigned long long run_off = (unsigned)rec[VKN_RLE_REC_RUN_OFF], byte_off = (unsigned)rec[VKN_RLE_REC_BYTE_OFF];
    St total;
    const St before = block_scan(sh, e, strip_count(st, rows), state[idx], total);
    St v = st_id();
    v.n = strip_runs(st, rows, before, last, hw, nullptr, 0, 0, nullptr, 0, 0);
    const St at = block_scan(sh, e, v, st_id(), total);
    strip_runs(st, rows, before, last, hw, runs, run_off, cap_runs, bytes, byte_off + sboff[idx] + at.n, cap_bytes);
}

// ------------------------------------------------------------------------------------------------------------------------ host
struct RleLayout {
    size_t bits, sum, state, stat, sbytes, sboff, tot, bytes;
    long long NS;
};
inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

inline bool rle_shape_ok(int K, int H, int W, int elem) {
    if (K < 1 || K > VKN_RLE_MAX_K || H < 1 || W < 1) return false;
    const long long hw = (long long)H * W;
    return hw < (1ll << 31) && hw * K * elem < (1ll << 31);
}

// own_bits: the workspace holds the masks as bits (the u8 / f32 entries); false: the caller hands the bits in (vkn_bits_rle_encode)
inline RleLayout rle_layout(int K, int H, int W, bool own_bits = true) {
    RleLayout l;
    l.NS = ((long long)W + VKN_RLE_STRIP_COLS - 1) / VKN_RLE_STRIP_COLS;
    const size_t strips = (size_t)K * (size_t)l.NS;
    size_t at = 0;
    l.bits = at, at += own_bits ? up16(strips * (size_t)H * 8) : 0;
    l.sum = at, at += strips * sizeof(St);
    l.state = at, at += strips * sizeof(St);
    l.stat = at, at += strips * sizeof(RleStat);
    l.sbytes = at, at += up16(strips * 4);
    l.sboff = at, at += up16(strips * 4);
    l.tot = at, at += up16((size_t)K * 8);
    l.bytes = at;
    return l;
}

// the seven launches behind the pack: `bits` [K][NS][H] -> records, pools, status
int rle_run(const unsigned long long* bits, const RleLayout& l, int K, int H, int W, int* records, unsigned* runs, int cap_runs, unsigned char* bytes,
            int cap_bytes, unsigned* status, void* ws, hipStream_t st) {
    char* base = static_cast<char*>(ws);
    St* sum = reinterpret_cast<St*>(base + l.sum);
    St* state = reinterpret_cast<St*>(base + l.state);
    RleStat* stat = reinterpret_cast<RleStat*>(base + l.stat);
    unsigned* sbytes = reinterpret_cast<unsigned*>(base + l.sbytes);
    unsigned* sboff = reinterpret_cast<unsigned*>(base + l.sboff);
    unsigned* tot = reinterpret_cast<unsigned*>(base + l.tot);
    const dim3 strips((unsigned)l.NS, (unsigned)K), block(RLE_THREADS);
    hipLaunchKernelGGL(k_rle_count, strips, block, 0, st, bits, sum, stat, H, W);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_rle_scan_mask<0>, dim3(K), block, 0, st, sum, state, stat, sbytes, sboff, tot, records, l.NS);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_rle_scan_all<0>, dim3(1), block, 0, st, tot, records, K, (unsigned)cap_runs, status);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_rle_len, strips, block, 0, st, bits, state, sbytes, H, W);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_rle_scan_mask<1>, dim3(K), block, 0, st, sum, state, stat, sbytes, sboff, tot, records, l.NS);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_rle_scan_all<1>, dim3(1), block, 0, st, tot, records, K, (unsigned)cap_bytes, status);
    VKN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_rle_emit, strips, block, 0, st, bits, state, sboff, records, runs, (unsigned)cap_runs, bytes, (unsigned)cap_bytes, H, W);
    VKN_CHECK_LAUNCH();
    return VKN_OK;
}

// T: unsigned char / float masks that the call packs into its workspace, or unsigned long long: the bits themselves
template <typename T>
int rle_encode(const T* in, float thr, int K, int H, int W, int* records, unsigned* runs, int cap_runs, unsigned char* bytes, int cap_bytes,
               unsigned* status, void* ws, size_t ws_bytes, void* stream) {
    constexpr bool BITS = sizeof(T) == 8;
    if (!in || !records || !runs || !bytes || !status || !ws || K < 0 || H < 0 || W < 0 || cap_runs < 0 || cap_bytes < 0) return VKN_E_ARG;
    if (!rle_shape_ok(K, H, W, BITS ? 1 : (int)sizeof(T))) return VKN_E_SHAPE;
    const RleLayout l = rle_layout(K, H, W, !BITS);
    if (ws_bytes != l.bytes) return VKN_E_WORKSPACE;
    if (!vkn_aligned(in, 16) || !vkn_aligned(records, 16) || !vkn_aligned(runs, 16) || !vkn_aligned(bytes, 16) || !vkn_aligned(ws, 16) ||
        !vkn_aligned(status, 4))
        return VKN_E_ALIGN;
    if (!vkn_on_device(in) || !vkn_on_device(records) || !vkn_on_device(runs) || !vkn_on_device(bytes) || !vkn_on_device(status) ||
        !vkn_on_device(ws))
        return VKN_E_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if constexpr (BITS) {
        return rle_run(in, l, K, H, W, records, runs, cap_runs, bytes, cap_bytes, status, ws, st);
    } else {
        auto* bits = reinterpret_cast<unsigned long long*>(static_cast<char*>(ws) + l.bits);
        if (!maskbits_pack<T>(in, thr, K, H, W, bits, st)) return VKN_E_LAUNCH;
        return rle_run(bits, l, K, H, W, records, runs, cap_runs, bytes, cap_bytes, status, ws, st);
    }
}

}  // namespace

extern "C" {

size_t vkn_rle_workspace_bytes(int K, int H, int W) {
    if (!rle_shape_ok(K, H, W, 1)) return 0;
    return rle_layout(K, H, W).bytes;
}

int vkn_rle_encode_u8(const unsigned char* masks, int K, int H, int W, int* records, unsigned* runs, int cap_runs, unsigned char* bytes,
                      int cap_bytes, unsigned* status, void* ws, size_t ws_bytes, void* stream) {
    return rle_encode<unsigned char>(masks, 0.f, K, H, W, records, runs, cap_runs, bytes, cap_bytes, status, ws, ws_bytes, stream);
}

int vkn_rle_encode_f32(const float* logits, float thr, int K, int H, int W, int* records, unsigned* runs, int cap_runs, unsigned char* bytes,
                       int cap_bytes, unsigned* status, void* ws, size_t ws_bytes, void* stream) {
    return rle_encode<float>(logits, thr, K, H, W, records, runs, cap_runs, bytes, cap_bytes, status, ws, ws_bytes, stream);
}

size_t vkn_bits_rle_workspace_bytes(int K, int H, int W) {
    if (!rle_shape_ok(K, H, W, 1)) return 0;
    return rle_layout(K, H, W, false).bytes;
}

int vkn_bits_rle_encode(const long long* bits, int K, int H, int W, int* records, unsigned* runs, int cap_runs, unsigned char* bytes,
                        int cap_bytes, unsigned* status, void* ws, size_t ws_bytes, void* stream) {
    return rle_encode<unsigned long long>(reinterpret_cast<const unsigned long long*>(bits), 0.f, K, H, W, records, runs, cap_runs, bytes, cap_bytes,
                                          status, ws, ws_bytes, stream);
}

}  // extern "C"
