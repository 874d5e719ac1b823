// Object-level scores of two instance maps on the device (utils/instances.py; the reference has no counterpart): the sparse overlap
// table between the instances of a prediction and those of the ground truth, an IoU per overlapping pair, the one-to-one matching
// above IoU 0.5 and the counts and scores that come from it (TP / FP / FN, panoptic quality, the DSB-2018 score).  Both maps are int32
// with ids 1 .. n and 0 as background (what ptb_cc_label writes); an id <= 0 or above that side's n is background.  Every phase is a
// launch of its own:
//   1. inst_pair_kernel    a workgroup reads one chunk of 1024 consecutive positions, four per lane, and folds the 64-bit keys
//                          (pred id << 32 | truth id) before anything touches global memory: runs of equal keys inside the lane and
//                          across the wave, then all keys of the chunk in a 1024-slot LDS table (key, count, first position), then
//                          the ids of each side in two further LDS tables.  ONE update per (workgroup, distinct key) goes to the
//                          global open-addressing table (64-bit compare-and-swap on the key, integer add on the count, atomicMin on
//                          the first position), ONE 64-bit add per (workgroup, id) to the dense area arrays.
//   overlaps:
//   2. inst_mark_kernel    every occupied slot sets the bit of its pair's first position in a bitmap over the positions and counts
//                          it in the bitmap word's counter; scan (ptb_scan_device.h, launches of its own) over the counters;
//      inst_rank_kernel    row of a slot = scan value of its word + set bits below its own: the rows are in the order of the pairs'
//                          first positions.
//   match:
//   3. inst_match_kernel   every occupied slot: IoU = I / (A_p + A_t - I) as one double division of exact integers; IoU > thresholds[0]
//                          (and equal classes) -> plain stores of partner and IoU on both sides.
//   4. inst_count_kernel   per block of 1024 instances, class and threshold: matches, their IoU sum in a fixed order, present instances;
//      inst_finish_kernel  adds the blocks' partial results in block order and writes counts and scores.
//
// THE RESULT IS A FUNCTION OF THE INPUT ALONE.  The order atomics arrive in decides where a key lies in the table and nothing else:
// counts and areas are integer sums, the first position is an integer minimum, the bitmap is an OR of distinct bits (a position belongs
// to one pair), the counters are integer sums, and a row number is computed from the first position only.  With thresholds >= 0.5
// an instance has at most one partner whose IoU passes, so the stores of the match kernel never compete.  The IoU sums are added by one
// lane per (class, threshold) in block order from partial sums that a fixed tree produced.
// EVERY LOOP IS BOUNDED.  A chunk holds at most 1024 distinct keys and ids, so a probe of an LDS table ends within its 1024 slots; a
// probe of the global table is capped at the slot count, which visits every slot: it fails only when every slot holds another key,
// i.e. when the input has more distinct pairs than slots > max_pairs.  A failed insert raises a device flag and is dropped (later
// probes that see the flag give up early: the result is already marked); num_pairs = -1 iff the flag is up or the number of occupied
// slots exceeds max_pairs -- exactly when the input has more than max_pairs distinct pairs.  No workgroup waits for another one.
#include <algorithm>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_scan_device.h"

namespace ptb {

constexpr int IN_THREADS = 256;
constexpr int IN_CHUNK = 1024;                  // positions of a chunk of the pair kernel, instances of a block of the count kernel
constexpr int IN_HASH = 1024;                   // slots of the LDS tables: a chunk has at most IN_CHUNK distinct keys
constexpr long long IN_MAX_PAIRS = 1LL << 28;
constexpr int IN_MAX_T = 16;
constexpr int IN_OUTPUTS = 17;
constexpr unsigned long long IN_MIXED = ~0ull;  // a lane whose four keys differ (no key: ids are below 2^31)
constexpr unsigned long long IN_MUL = 0x9E3779B97F4A7C15ull;
static_assert(IN_CHUNK == 4 * IN_THREADS && IN_HASH == 1 << 10, "four positions per lane; the LDS hash keeps 10 bits");

#define IN_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct InstTable {
    unsigned long long* key;    // [slots]: 0 = free
    unsigned* cnt;              // [slots]: positions of the pair
    unsigned* pos;              // [slots]: its first position
    int* flag;                  // an insert failed
    unsigned slots;             // a power of two >= 2
    int shift;                  // 64 - log2(slots)
};

struct InstPairArgs {
    const int* pred;
    const int* truth;
    unsigned long long* area_p; // [np]
    unsigned long long* area_t; // [nt]
    InstTable t;
    unsigned n;
    int np, nt;
};

// ---------------------------------------------------------------------------------------------------------- phase 1
__device__ __forceinline__ int inst_lds_slot64(unsigned long long* hkey, unsigned long long key) {
    unsigned h = (unsigned)((key * IN_MUL) >> 54);
    for (int probe = 0; probe < IN_HASH; ++probe) {
        const unsigned long long old = atomicCAS(hkey + h, 0ull, key);
        if (old == 0ull || old == key) return (int)h;
        h = (h + 1) & (IN_HASH - 1);
    }
    return -1;
}

__device__ __forceinline__ int inst_lds_slot32(int* hkey, int key) {
    unsigned h = ((unsigned)key * 2654435761u) >> 22;
    for (int probe = 0; probe < IN_HASH; ++probe) {
        const int old = atomicCAS(hkey + h, 0, key);
        if (old == 0 || old == key) return (int)h;
        h = (h + 1) & (IN_HASH - 1);
    }
    return -1;
}

__device__ __forceinline__ void inst_global_add(const InstTable& t, unsigned long long key, unsigned cnt, unsigned pos) {
    unsigned h = (unsigned)((key * IN_MUL) >> t.shift);
    for (unsigned probe = 0; probe < t.slots; ++probe) {
        if ((probe & 63u) == 63u && __hip_atomic_load(t.flag, IN_RELAXED)) return;     // the table has overflown already
        unsigned long long old = __hip_atomic_load(t.key + h, IN_RELAXED);
        if (old == 0ull && __hip_atomic_compare_exchange_strong(t.key + h, &old, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            old = key;                                           // (a failed exchange leaves the slot's key in old)
        if (old == key) {
            __hip_atomic_fetch_add(t.cnt + h, cnt, IN_RELAXED);
            // the first position only decreases: a value at or below pos already makes this minimum a no-op (chunks start roughly in
            // order, so most workgroups of a large instance find it done and spare its slot one read-modify-write)
            if (__hip_atomic_load(t.pos + h, IN_RELAXED) > pos) __hip_atomic_fetch_min(t.pos + h, pos, IN_RELAXED);
            return;
        }
        h = (h + 1) & (t.slots - 1);
    }
    __hip_atomic_store(t.flag, 1, IN_RELAXED);
}

template <bool WIDE>
__global__ __launch_bounds__(IN_THREADS) void inst_pair_kernel(const InstPairArgs a) {
    __shared__ unsigned long long hkey[IN_HASH];
    __shared__ unsigned hcnt[IN_HASH], hpos[IN_HASH];
    __shared__ int akey[2][IN_HASH];
    __shared__ unsigned acnt[2][IN_HASH];
    for (int s = threadIdx.x; s < IN_HASH; s += IN_THREADS) {
        hkey[s] = 0ull; hcnt[s] = 0; hpos[s] = 0xffffffffu;
        akey[0][s] = 0; akey[1][s] = 0; acnt[0][s] = 0; acnt[1][s] = 0;
    }
    __syncthreads();
    const unsigned base = blockIdx.x * (unsigned)IN_CHUNK;
    const unsigned valid = min((unsigned)IN_CHUNK, a.n - base);
    const unsigned i = threadIdx.x * 4u;
    const int lane = threadIdx.x & 63;
    int vp[4] = {0, 0, 0, 0}, vt[4] = {0, 0, 0, 0};
    if (WIDE && i + 3 < valid) {                                 // an aligned base: base + i is a multiple of four elements
        __builtin_memcpy(vp, __builtin_assume_aligned(a.pred + base + i, 16), 16);
        __builtin_memcpy(vt, __builtin_assume_aligned(a.truth + base + i, 16), 16);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j < valid) { vp[j] = a.pred[base + i + j]; vt[j] = a.truth[base + i + j]; }
    }
    unsigned long long key[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned p = vp[j] >= 1 && vp[j] <= a.np ? (unsigned)vp[j] : 0u;
        const unsigned t = vt[j] >= 1 && vt[j] <= a.nt ? (unsigned)vt[j] : 0u;
        key[j] = ((unsigned long long)p << 32) | t;             // 0: background on both sides (and positions past the end)
    }
    // lanes whose four keys agree are folded across the wave; a lane with differing keys adds its own runs
    const bool uniform = key[0] == key[1] && key[1] == key[2] && key[2] == key[3];
    const unsigned long long ukey = uniform ? key[0] : IN_MIXED;
    const unsigned long long prev = __shfl_up(ukey, 1);
    const bool leader = lane == 0 || prev != ukey || !uniform;
    const unsigned long long m = __ballot(leader);
    const unsigned long long above = lane == 63 ? 0ull : m >> (lane + 1);
    const int len = above ? __ffsll((long long)above) : 64 - lane;
    bool bad = false;
    auto add = [&](unsigned long long k, unsigned cnt, unsigned pos) {
        const int slot = inst_lds_slot64(hkey, k);
        if (slot < 0) { bad = true; return; }
        atomicAdd(hcnt + slot, cnt);
        atomicMin(hpos + slot, pos);
    };
    if (uniform) {
        if (leader && key[0] != 0ull) add(key[0], 4u * (unsigned)len, base + i);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (key[j] == 0ull || (j > 0 && key[j] == key[j - 1])) continue;
            unsigned run = 1;
#pragma unroll
            for (int q = j + 1; q < 4; ++q) run += (run == (unsigned)(q - j) && key[q] == key[j]) ? 1u : 0u;
            add(key[j], run, base + i + j);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < IN_HASH; s += IN_THREADS) {   // one update per (workgroup, distinct key)
        const unsigned long long k = hkey[s];
        if (k == 0ull) continue;
        const int p = (int)(k >> 32), t = (int)(unsigned)k;
        const unsigned c = hcnt[s];
        if (p) {
            const int slot = inst_lds_slot32(akey[0], p);
            if (slot >= 0) atomicAdd(&acnt[0][slot], c); else bad = true;
        }
        if (t) {
            const int slot = inst_lds_slot32(akey[1], t);
            if (slot >= 0) atomicAdd(&acnt[1][slot], c); else bad = true;
        }
        if (p && t) inst_global_add(a.t, k, c, hpos[s]);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < IN_HASH; s += IN_THREADS) {   // one add per (workgroup, id)
        if (akey[0][s]) __hip_atomic_fetch_add(a.area_p + (akey[0][s] - 1), (unsigned long long)acnt[0][s], IN_RELAXED);
        if (akey[1][s]) __hip_atomic_fetch_add(a.area_t + (akey[1][s] - 1), (unsigned long long)acnt[1][s], IN_RELAXED);
    }
    if (bad) __hip_atomic_store(a.t.flag, 1, IN_RELAXED);
}

// ---------------------------------------------------------------------------------------------------------- phase 2
__global__ __launch_bounds__(IN_THREADS) void inst_mark_kernel(const InstTable t, unsigned* bitmap, unsigned* counts, unsigned n) {
    const unsigned s = blockIdx.x * IN_THREADS + threadIdx.x;
    if (s >= t.slots || t.key[s] == 0ull) return;
    const unsigned pos = t.pos[s];
    if (pos >= n) return;                                        // (cannot happen: a key is stored together with a position)
    __hip_atomic_fetch_or(bitmap + (pos >> 5), 1u << (pos & 31u), IN_RELAXED);
    __hip_atomic_fetch_add(counts + (pos >> 5), 1u, IN_RELAXED);
}

__global__ __launch_bounds__(IN_THREADS) void inst_rank_kernel(const InstTable t, const unsigned* __restrict__ bitmap, const long long* __restrict__ excl,
                                                               unsigned n, unsigned words, long long rows, long long max_pairs, int* pairs,
                                                               long long* intersection, long long* num_pairs) {
    const unsigned s = blockIdx.x * IN_THREADS + threadIdx.x;
    if (s == 0) {
        const long long total = excl[words];
        *num_pairs = (*t.flag != 0 || total > max_pairs) ? -1 : total;
    }
    if (s >= t.slots) return;
    const unsigned long long k = t.key[s];
    if (k == 0ull) return;
    const unsigned pos = t.pos[s];
    if (pos >= n) return;
    const long long r = excl[pos >> 5] + __popc(bitmap[pos >> 5] & ((1u << (pos & 31u)) - 1u));
    if (r >= rows) return;                                       // more pairs than rows: num_pairs is -1
    *reinterpret_cast<int2*>(pairs + 2 * r) = make_int2((int)(k >> 32), (int)(unsigned)k);
    intersection[r] = (long long)t.cnt[s];
}

// ---------------------------------------------------------------------------------------------------------- phase 3
struct InstMatchArgs {
    const long long* area_p;
    const long long* area_t;
    const void* class_p;        // both null: no classes
    const void* class_t;
    int* match_p;
    int* match_t;
    double* iou_p;
    double* iou_t;
    unsigned* distinct;
    double tau0;
    long long K;
    int eb_p, eb_t;
};

__device__ __forceinline__ long long inst_class(const void* c, int eb, long long i) {
    switch (eb) {
        case 1: return reinterpret_cast<const unsigned char*>(c)[i];
        case 2: return reinterpret_cast<const short*>(c)[i];
        case 4: return reinterpret_cast<const int*>(c)[i];
        default: return reinterpret_cast<const long long*>(c)[i];
    }
}

__global__ __launch_bounds__(IN_THREADS) void inst_match_kernel(const InstTable t, const InstMatchArgs a) {
    const unsigned s = blockIdx.x * IN_THREADS + threadIdx.x;
    const unsigned long long k = s < t.slots ? t.key[s] : 0ull;
    const unsigned long long occupied = __ballot(k != 0ull);
    if ((threadIdx.x & 63) == 0 && occupied) __hip_atomic_fetch_add(a.distinct, (unsigned)__popcll(occupied), IN_RELAXED);
    if (k == 0ull) return;
    const long long p = (long long)(k >> 32) - 1, q = (long long)(unsigned)k - 1;
    const long long inter = (long long)t.cnt[s];
    const long long uni = a.area_p[p] + a.area_t[q] - inter;
    if (uni <= 0) return;
    const double iou = (double)inter / (double)uni;
    if (!(iou > a.tau0)) return;
    if (a.class_p && a.class_t) {
        const long long cp = inst_class(a.class_p, a.eb_p, p), ct = inst_class(a.class_t, a.eb_t, q);
        if (cp != ct || cp < 0 || cp >= a.K) return;
    }
    // tau0 >= 0.5: no other pair of p or of q passes, so nothing else stores here
    a.match_p[p] = (int)(q + 1); a.iou_p[p] = iou;
    a.match_t[q] = (int)(p + 1); a.iou_t[q] = iou;
}

// ---------------------------------------------------------------------------------------------------------- phase 4
struct InstCountArgs {
    const long long* area_p;
    const long long* area_t;
    const double* iou_p;
    const void* class_p;
    const void* class_t;
    unsigned* part_tp;          // [gp, K, T]
    double* part_sum;           // [gp, K, T]
    unsigned* part_pp;          // [gp, K]: present predictions
    unsigned* part_pt;          // [gt, K]: present truths
    long long np, nt, K;
    unsigned gp;
    int T, eb_p, eb_t;
    double tau[IN_MAX_T];
};

__device__ __forceinline__ double inst_tau(const InstCountArgs& a, int j) {
    double v = a.tau[0];
#pragma unroll
    for (int s = 1; s < IN_MAX_T; ++s) v = s == j ? a.tau[s] : v;      // (constant indices only: the by-value struct stays in registers)
    return v;
}

__global__ __launch_bounds__(IN_THREADS) void inst_count_kernel(const InstCountArgs a) {
    __shared__ unsigned wcnt[4];
    __shared__ double wsum[4];
    const long long k = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool truth_side = blockIdx.x >= a.gp;
    const long long g = truth_side ? blockIdx.x - a.gp : blockIdx.x;
    const long long n = truth_side ? a.nt : a.np;
    const long long* area = truth_side ? a.area_t : a.area_p;
    const void* cls = truth_side ? a.class_t : a.class_p;
    const int eb = truth_side ? a.eb_t : a.eb_p;
    const long long i0 = g * IN_CHUNK + (long long)threadIdx.x * 4;
    bool mine[4];
    double iou[4];
    unsigned present = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = i0 + j < n;
        mine[j] = in && (!cls || inst_class(cls, eb, i0 + j) == k);
        iou[j] = (mine[j] && !truth_side) ? a.iou_p[i0 + j] : 0.0;
        present += (mine[j] && area[i0 + j] > 0) ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) present += __shfl_xor(present, d);
    if (lane == 0) wcnt[wave] = present;
    __syncthreads();
    if (threadIdx.x == 0) (truth_side ? a.part_pt : a.part_pp)[g * a.K + k] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (truth_side) return;
#pragma unroll 1
    for (int j = 0; j < a.T; ++j) {
        const double tau = inst_tau(a, j);
        unsigned c = 0;
        double x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool hit = iou[q] > tau;
            c += hit ? 1u : 0u;
            x[q] = hit ? iou[q] : 0.0;
        }
        double sum = ((x[0] + x[1]) + x[2]) + x[3];              // a fixed tree: the lane's four, the wave's butterfly, the waves in order
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            c += __shfl_xor(c, d);
            sum += __shfl_xor(sum, d);
        }
        __syncthreads();
        if (lane == 0) { wcnt[wave] = c; wsum[wave] = sum; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const long long o = (g * a.K + k) * a.T + j;
            a.part_tp[o] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            a.part_sum[o] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        }
    }
}

struct InstFinishArgs {
    const unsigned* part_tp;
    const double* part_sum;
    const unsigned* part_pp;
    const unsigned* part_pt;
    const int* flag;
    const unsigned* distinct;
    long long* tp;              // [K, T] each
    long long* fp;
    long long* fn;
    double* sum_iou;
    double* sq;
    double* rq;
    double* pq;
    double* ap;
    long long* num_pairs;
    long long K, max_pairs;
    unsigned gp, gt;
    int T;
};

__global__ __launch_bounds__(IN_THREADS) void inst_finish_kernel(const InstFinishArgs a) {
    const long long o = (long long)blockIdx.x * IN_THREADS + threadIdx.x;
    const bool over = *a.flag != 0 || (long long)*a.distinct > a.max_pairs;
    if (o == 0) *a.num_pairs = over ? -1 : (long long)*a.distinct;
    if (o >= a.K * a.T) return;
    const long long k = o / a.T, j = o - k * a.T;
    long long tp = 0, pp = 0, pt = 0;
    double sum = 0.0;
    for (unsigned g = 0; g < a.gp; ++g) {                        // block order
        const long long r = ((long long)g * a.K + k) * a.T + j;
        tp += a.part_tp[r];
        sum += a.part_sum[r];
        pp += a.part_pp[(long long)g * a.K + k];
    }
    for (unsigned g = 0; g < a.gt; ++g) pt += a.part_pt[(long long)g * a.K + k];
    const long long fp = pp - tp, fn = pt - tp;
    const double nan = __builtin_nan("");
    const double half = (double)tp + (double)fp / 2.0 + (double)fn / 2.0;
    const double all = (double)(tp + fp + fn);
    a.tp[o] = tp; a.fp[o] = fp; a.fn[o] = fn; a.sum_iou[o] = sum;
    a.sq[o] = (over || tp == 0) ? nan : sum / (double)tp;
    a.rq[o] = (over || half == 0.0) ? nan : (double)tp / half;
    a.pq[o] = (over || half == 0.0) ? nan : sum / half;
    a.ap[o] = (over || all == 0.0) ? nan : (double)tp / all;
}

// ---------------------------------------------------------------------------------------------------------- host side
struct InstPlan {
    long long n, np, nt, m, K, T, slots, words, gp, gt, rows;
    int shift, levels;
    long long cnt[SCAN_MAX_LEVELS];
    long long off_hdr, off_key, off_cnt, off_bitmap, off_counts, zero_bytes, off_pos, off_excl, off_sums[SCAN_MAX_LEVELS];
    long long off_ptp, off_psum, off_ppp, off_ppt, ws_bytes;
    long long out[IN_OUTPUTS], out_bytes;
};

enum { IN_NUM_PAIRS, IN_PRED_AREA, IN_TRUTH_AREA, IN_PAIRS, IN_INTERSECTION, IN_PRED_MATCH, IN_TRUTH_MATCH, IN_PRED_IOU, IN_TRUTH_IOU, IN_TP, IN_FP, IN_FN,
       IN_SUM_IOU, IN_SQ, IN_RQ, IN_PQ, IN_AP };

// T == 0: the overlap table (rows = max_pairs); T >= 1: the matching (no rows)
static int inst_plan(long long n, long long np, long long nt, long long m, int T, long long K, InstPlan& p) {
    if (n < 1 || np < 0 || nt < 0 || m < 0 || T < 0 || T > IN_MAX_T || K < 0 || (T == 0 && K != 0)) return PTB_EINVAL;
    if (n > MAX_POS || np > MAX_POS || nt > MAX_POS || m > IN_MAX_PAIRS || K > 65535) return PTB_EUNSUPPORTED;
    p.n = n; p.np = np; p.nt = nt; p.m = m; p.T = T; p.K = std::max<long long>(K, 1);
    p.slots = 2; p.shift = 63;
    while (p.slots < 2 * m) { p.slots *= 2; --p.shift; }
    p.rows = T == 0 ? m : 0;
    p.words = T == 0 ? (n + 31) / 32 : 0;
    p.gp = (np + IN_CHUNK - 1) / IN_CHUNK; p.gt = (nt + IN_CHUNK - 1) / IN_CHUNK;
    p.levels = T == 0 ? scan_levels(p.words + 1, p.cnt) : 0;
    long long o = 0;
    p.off_hdr = o; o += 16;
    p.off_key = o; o += up16(8 * p.slots);
    p.off_cnt = o; o += up16(4 * p.slots);
    p.off_bitmap = o; o += up16(4 * p.words);
    p.off_counts = o; o += T == 0 ? up16(4 * (p.words + 1)) : 0;
    p.zero_bytes = o;
    p.off_pos = o; o += up16(4 * p.slots);
    p.off_excl = o; o += T == 0 ? up16(8 * (p.words + 1)) : 0;
    for (int l = 0; l < p.levels; ++l) { p.off_sums[l] = o; o += up16(8 * p.cnt[l]); }
    const long long kt = p.K * T;
    p.off_ptp = o; o += up16(4 * p.gp * kt);
    p.off_psum = o; o += up16(8 * p.gp * kt);
    p.off_ppp = o; o += T ? up16(4 * p.gp * p.K) : 0;
    p.off_ppt = o; o += T ? up16(4 * p.gt * p.K) : 0;
    p.ws_bytes = o;
    const long long sizes[IN_OUTPUTS] = {8, 8 * np, 8 * nt, 8 * p.rows, 8 * p.rows, T ? 4 * np : 0, T ? 4 * nt : 0, T ? 8 * np : 0, T ? 8 * nt : 0,
                                         8 * kt, 8 * kt, 8 * kt, 8 * kt, 8 * kt, 8 * kt, 8 * kt, 8 * kt};
    o = 0;
    for (int i = 0; i < IN_OUTPUTS; ++i) { p.out[i] = o; o += up16(sizes[i]); }
    p.out_bytes = o;
    return PTB_OK;
}

// the zeroed workspace and outputs, then phase 1
static int inst_pairs(const int32_t* pred, const int32_t* truth, const InstPlan& p, char* out, char* ws, InstTable& t, hipStream_t s) {
    t.key = reinterpret_cast<unsigned long long*>(ws + p.off_key);
    t.cnt = reinterpret_cast<unsigned*>(ws + p.off_cnt);
    t.pos = reinterpret_cast<unsigned*>(ws + p.off_pos);
    t.flag = reinterpret_cast<int*>(ws + p.off_hdr);
    t.slots = (unsigned)p.slots; t.shift = p.shift;
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)p.zero_bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(t.pos, 0xff, (size_t)(4 * p.slots), s);
    if (e == hipSuccess) e = hipMemsetAsync(out, 0, (size_t)p.out_bytes, s);
    if (e != hipSuccess) { set_hip_error(e); return PTB_ELAUNCH; }
    InstPairArgs a{};
    a.pred = pred; a.truth = truth; a.t = t; a.n = (unsigned)p.n; a.np = (int)p.np; a.nt = (int)p.nt;
    a.area_p = reinterpret_cast<unsigned long long*>(out + p.out[IN_PRED_AREA]);
    a.area_t = reinterpret_cast<unsigned long long*>(out + p.out[IN_TRUTH_AREA]);
    const unsigned chunks = (unsigned)((p.n + IN_CHUNK - 1) / IN_CHUNK);
    with_bool(aligned16(pred) && aligned16(truth), [&](auto w) {
        hipLaunchKernelGGL((inst_pair_kernel<w()>), dim3(chunks), dim3(IN_THREADS), 0, s, a);
    });
    return PTB_OK;
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_inst_plan(int64_t positions, int64_t n_pred, int64_t n_truth, int64_t max_pairs, int T, int64_t K, int64_t* slots,
                             int64_t* workspace_bytes, int64_t* out_offsets, int64_t* out_bytes) {
    InstPlan p;
    if (int rc = inst_plan(positions, n_pred, n_truth, max_pairs, T, K, p)) return rc;
    if (slots) *slots = p.slots;
    if (workspace_bytes) *workspace_bytes = p.ws_bytes;
    if (out_offsets)
        for (int i = 0; i < IN_OUTPUTS; ++i) out_offsets[i] = p.out[i];
    if (out_bytes) *out_bytes = p.out_bytes;
    return PTB_OK;
}

extern "C" int ptb_inst_overlaps(const int32_t* pred, const int32_t* truth, int64_t positions, int64_t n_pred, int64_t n_truth, int64_t max_pairs, void* out,
                                 int64_t out_bytes, void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (!pred || !truth || !out || !workspace) return PTB_EINVAL;
    InstPlan p;
    if (int rc = inst_plan(positions, n_pred, n_truth, max_pairs, 0, 0, p)) return rc;
    if (out_bytes < p.out_bytes || workspace_bytes < p.ws_bytes || !aligned16(out) || !aligned16(workspace)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    char* o = reinterpret_cast<char*>(out);
    hipStream_t s = (hipStream_t)stream;
    InstTable t{};
    if (int rc = inst_pairs(pred, truth, p, o, ws, t, s)) return rc;
    unsigned* bitmap = reinterpret_cast<unsigned*>(ws + p.off_bitmap);
    unsigned* counts = reinterpret_cast<unsigned*>(ws + p.off_counts);
    long long* excl = reinterpret_cast<long long*>(ws + p.off_excl);
    const dim3 over_slots((unsigned)((p.slots + IN_THREADS - 1) / IN_THREADS));
    hipLaunchKernelGGL(inst_mark_kernel, over_slots, dim3(IN_THREADS), 0, s, t, bitmap, counts, (unsigned)p.n);
    long long* sums[SCAN_MAX_LEVELS] = {};
    for (int l = 0; l < p.levels; ++l) sums[l] = reinterpret_cast<long long*>(ws + p.off_sums[l]);
    scan_exclusive(counts, p.words + 1, p.levels, p.cnt, sums, excl, s);
    hipLaunchKernelGGL(inst_rank_kernel, over_slots, dim3(IN_THREADS), 0, s, t, (const unsigned*)bitmap, (const long long*)excl, (unsigned)p.n, (unsigned)p.words,
                       p.rows, p.m, reinterpret_cast<int*>(o + p.out[IN_PAIRS]), reinterpret_cast<long long*>(o + p.out[IN_INTERSECTION]),
                       reinterpret_cast<long long*>(o + p.out[IN_NUM_PAIRS]));
    return check_launch();
}

extern "C" int ptb_inst_match(const int32_t* pred, const int32_t* truth, int64_t positions, int64_t n_pred, int64_t n_truth, int64_t max_pairs,
                              const double* thresholds, int T, const void* pred_class, int pred_class_elem_bytes, const void* truth_class,
                              int truth_class_elem_bytes, int64_t K, void* out, int64_t out_bytes, void* workspace, int64_t workspace_bytes,
                              ptb_stream_t stream) {
    if (!pred || !truth || !out || !workspace || !thresholds || T < 1 || T > IN_MAX_T) return PTB_EINVAL;
    const bool classes = K > 0;
    if (!classes && (pred_class || truth_class)) return PTB_EINVAL;
    if (classes && ((!pred_class && n_pred > 0) || (!truth_class && n_truth > 0))) return PTB_EINVAL;      // (a side without instances needs no classes)
    if (classes && (bad_elem_bytes(pred_class_elem_bytes) || bad_elem_bytes(truth_class_elem_bytes))) return PTB_EINVAL;
    for (int j = 0; j < T; ++j)
        if (!(thresholds[j] >= 0.5 && thresholds[j] < 1.0) || (j > 0 && !(thresholds[j] > thresholds[j - 1]))) return PTB_EINVAL;
    InstPlan p;
    if (int rc = inst_plan(positions, n_pred, n_truth, max_pairs, T, K, p)) return rc;
    if (out_bytes < p.out_bytes || workspace_bytes < p.ws_bytes || !aligned16(out) || !aligned16(workspace)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    char* o = reinterpret_cast<char*>(out);
    hipStream_t s = (hipStream_t)stream;
    InstTable t{};
    if (int rc = inst_pairs(pred, truth, p, o, ws, t, s)) return rc;
    unsigned* distinct = reinterpret_cast<unsigned*>(ws + p.off_hdr) + 1;
    InstMatchArgs m{};
    m.area_p = reinterpret_cast<const long long*>(o + p.out[IN_PRED_AREA]); m.area_t = reinterpret_cast<const long long*>(o + p.out[IN_TRUTH_AREA]);
    m.class_p = pred_class; m.class_t = truth_class; m.eb_p = pred_class_elem_bytes; m.eb_t = truth_class_elem_bytes; m.K = p.K;
    m.match_p = reinterpret_cast<int*>(o + p.out[IN_PRED_MATCH]); m.match_t = reinterpret_cast<int*>(o + p.out[IN_TRUTH_MATCH]);
    m.iou_p = reinterpret_cast<double*>(o + p.out[IN_PRED_IOU]); m.iou_t = reinterpret_cast<double*>(o + p.out[IN_TRUTH_IOU]);
    m.distinct = distinct; m.tau0 = thresholds[0];
    hipLaunchKernelGGL(inst_match_kernel, dim3((unsigned)((p.slots + IN_THREADS - 1) / IN_THREADS)), dim3(IN_THREADS), 0, s, t, m);
    InstCountArgs c{};
    c.area_p = m.area_p; c.area_t = m.area_t; c.iou_p = m.iou_p; c.class_p = pred_class; c.class_t = truth_class; c.eb_p = m.eb_p; c.eb_t = m.eb_t;
    c.part_tp = reinterpret_cast<unsigned*>(ws + p.off_ptp); c.part_sum = reinterpret_cast<double*>(ws + p.off_psum);
    c.part_pp = reinterpret_cast<unsigned*>(ws + p.off_ppp); c.part_pt = reinterpret_cast<unsigned*>(ws + p.off_ppt);
    c.np = p.np; c.nt = p.nt; c.K = p.K; c.gp = (unsigned)p.gp; c.T = T;
    for (int j = 0; j < IN_MAX_T; ++j) c.tau[j] = j < T ? thresholds[j] : 2.0;
    if (p.gp + p.gt > 0) hipLaunchKernelGGL(inst_count_kernel, dim3((unsigned)(p.gp + p.gt), (unsigned)p.K), dim3(IN_THREADS), 0, s, c);
    InstFinishArgs f{};
    f.part_tp = c.part_tp; f.part_sum = c.part_sum; f.part_pp = c.part_pp; f.part_pt = c.part_pt; f.flag = t.flag; f.distinct = distinct;
    f.tp = reinterpret_cast<long long*>(o + p.out[IN_TP]); f.fp = reinterpret_cast<long long*>(o + p.out[IN_FP]); f.fn = reinterpret_cast<long long*>(o + p.out[IN_FN]);
    f.sum_iou = reinterpret_cast<double*>(o + p.out[IN_SUM_IOU]); f.sq = reinterpret_cast<double*>(o + p.out[IN_SQ]); f.rq = reinterpret_cast<double*>(o + p.out[IN_RQ]);
    f.pq = reinterpret_cast<double*>(o + p.out[IN_PQ]); f.ap = reinterpret_cast<double*>(o + p.out[IN_AP]);
    f.num_pairs = reinterpret_cast<long long*>(o + p.out[IN_NUM_PAIRS]);
    f.K = p.K; f.max_pairs = p.m; f.gp = (unsigned)p.gp; f.gt = (unsigned)p.gt; f.T = T;
    hipLaunchKernelGGL(inst_finish_kernel, dim3((unsigned)((p.K * T + IN_THREADS - 1) / IN_THREADS)), dim3(IN_THREADS), 0, s, f);
    return check_launch();
}
