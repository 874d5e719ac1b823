// Marker-controlled watershed of a height map (utils/watershed.py; the reference has no counterpart), by an ORDER-FREE definition:
//   M      the flooded set: mask != 0, height neither NaN nor +inf.  Seeds: the positions of M whose marker is not the background.
//   C(p)   the pass height: min over paths of M from a seed to p of the max of the height along the path.  The fixed point of
//          C(p) <- min(C(p), max(C(q), h(p))) over neighbours q, from h on seeds and "none" elsewhere.
//   K(p)   D(p) << 32 | sigma(p): the fewest ADMISSIBLE steps (q -> p with C(q) <= C(p)) from a seed, and the smallest linear index among
//          the seeds that reach p in that many.  The fixed point of K(p) <- min(K(p), K(q) + 2^32) over admissible q, from 0 << 32 | index.
// Both rules are monotone, so every order of relaxation -- tile by tile, with neighbours' values of the sweep before or of this one --
// ends at the same maps: the result is a function of the inputs alone.  The phases cannot be fused ((C, D, sigma) is not monotone):
// the path phase starts when the cost phase has converged.
//   1. ws_init_kernel    one pass over height / markers / mask: the ordered 32-bit key of every height (float32 bits mapped monotonically,
//                        -0 as +0, 0xFFFFFFFF outside M), the start of C and K, and a flag for every tile that holds a seed.
//   2. ws_cost_kernel,   the two relaxations.  A workgroup owns a tile (2-D: 64 x 64; 3-D: a brick 8 x 8 x 32) and holds it with a one-position
//   3. ws_path_kernel    halo in LDS.  A thread owns a run of positions along the slowest axis of the tile and relaxes them: from the neighbours
//                        in LDS, then down and up its run in registers.  Barriers separate the reads of a trip from its writes, a workgroup-wide
//                        flag ends the trips, WS_CAP bounds them (a tile that ends at the cap has changed, so it runs again).  Only the
//                        owning tile writes a position, and only the positions that changed.  Halo reads and the write-back are relaxed
//                        agent-scope 32- / 64-bit accesses; a stale halo value is one the fixed point lies below as well.
//   4. ws_gather_kernel  labels[p] = markers[entry + sigma(p)] or the background, and the optional cost (float32) and seed (int32) maps.
// TILE ACTIVITY.  A tile runs in sweep k iff it or a tile next to it changed in sweep k - 1 (sweep 0: holds a seed); it writes its own
// flag of sweep k, zero included.  One word per phase holds 1 + the last sweep that changed anything: a sweep whose predecessor changed
// nothing returns at once, and the host reads that word back after every WS_BATCH launches.
// EVERY LOOP IS BOUNDED (the trips by WS_CAP, the sweeps by max_sweeps).  No workgroup waits for another one; there are no atomic
// read-modify-writes at all.
#include <algorithm>
#include <cmath>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_edt_common.h"

namespace ptb {

using u64 = unsigned long long;

constexpr unsigned WS_NONE = 0xFFFFFFFFu;       // the cost key of "outside M" / "not reached"
constexpr u64 WS_NONE64 = ~0ull;                // the path key of the same
constexpr u64 WS_STEP = 1ull << 32;
constexpr int WS_THREADS = 256;
constexpr int WS_BATCH = 8;                     // sweeps launched between two read-backs of the "changed" word

// a tile: A x B x X positions along (slowest, middle, fastest); a thread owns RUN consecutive positions along A.  2-D: A = rows, no
// middle axis (HB: its halo).  A / RUN * B * X == WS_THREADS.
template <int DIMS>
struct WsTile;
template <>
struct WsTile<2> {
    static constexpr int A = 64, B = 1, X = 64, RUN = 16, HB = 0, CAP = 64;
};
template <>
struct WsTile<3> {
    static constexpr int A = 8, B = 8, X = 32, RUN = 8, HB = 1, CAP = 32;
};
template <int DIMS>
struct WsLds {
    using G = WsTile<DIMS>;
    static constexpr int LB = G::B + 2 * G::HB, LX = G::X + 2, CELLS = (G::A + 2) * LB * LX;
    static_assert(G::A / G::RUN * G::B * G::X == WS_THREADS && G::A % G::RUN == 0, "a thread per run");
    static_assert(CELLS * 12 <= 64 * 1024, "the path kernel holds a 64-bit and a 32-bit map");
};

__device__ __forceinline__ unsigned ws_order(float h) {                        // monotone: a < b <=> ws_order(a) < ws_order(b); -0 as +0
    unsigned b = __float_as_uint(h);
    if (h == 0.0f) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ws_unorder(unsigned k) {
    if (k == WS_NONE) return INFINITY;
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// element types of the height map: every value is exact in float32
template <int HT>
struct WsHeight;
template <>
struct WsHeight<PTB_F32> {
    using R = float;
    static __device__ __forceinline__ float get(R v) { return v; }
};
template <>
struct WsHeight<PTB_F16> {
    using R = _Float16;
    static __device__ __forceinline__ float get(R v) { return (float)v; }
};
template <>
struct WsHeight<PTB_BF16> {
    using R = unsigned short;
    static __device__ __forceinline__ float get(R v) { return __uint_as_float((unsigned)v << 16); }
};
template <>
struct WsHeight<PTB_U8> {
    using R = unsigned char;
    static __device__ __forceinline__ float get(R v) { return (float)v; }
};
template <>
struct WsHeight<PTB_I16> {
    using R = short;
    static __device__ __forceinline__ float get(R v) { return (float)v; }
};

// ---------------------------------------------------------------------------------------------------------- init
struct WsInitArgs {
    const void* height;
    const void* markers;
    const unsigned char* mask;  // or NULL
    unsigned* hkey;             // [total] the ordered key of the height, WS_NONE outside M
    unsigned* cost;             // [total] hkey on seeds, WS_NONE elsewhere
    u64* key;                   // [total] the index within the entry on seeds, WS_NONE64 elsewhere
    unsigned* seed_flags;       // [tiles] zeroed by the caller: 1 where the tile holds a seed
    long long background;
    unsigned total, per_entry, tiles_per_entry;
    int EB, W, TA, TB, TX, ntb, ntx, all_seeds;
};

template <int HT, class T, bool WIDE>
__global__ __launch_bounds__(WS_THREADS) void ws_init_kernel(const WsInitArgs a) {
    using R = typename WsHeight<HT>::R;
    const unsigned p0 = (blockIdx.x * (unsigned)WS_THREADS + threadIdx.x) * 4u;                  // (total <= 2^31 - 2: p0 + 3 fits 32 bits)
    if (p0 >= a.total) return;
    const R* height = reinterpret_cast<const R*>(a.height);
    const T* markers = reinterpret_cast<const T*>(a.markers);
    const T bg = (T)a.background;
    R h[4] = {(R)0, (R)0, (R)0, (R)0};
    T m[4] = {bg, bg, bg, bg};
    unsigned char k[4] = {1, 1, 1, 1};
    if constexpr (WIDE) {                                                      // total % 4 == 0 and aligned bases: all four positions exist
        constexpr int AH = sizeof(R) * 4 < 16 ? sizeof(R) * 4 : 16, AM = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        __builtin_memcpy(h, __builtin_assume_aligned(height + p0, AH), sizeof(h));
        __builtin_memcpy(m, __builtin_assume_aligned(markers + p0, AM), sizeof(m));
        if (a.mask) __builtin_memcpy(k, __builtin_assume_aligned(a.mask + p0, 4), sizeof(k));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < a.total) {
                h[j] = height[p0 + j];
                m[j] = markers[p0 + j];
                if (a.mask) k[j] = a.mask[p0 + j];
            }
    }
    unsigned e0 = p0 - p0 % a.per_entry;                                       // the first position of p0's entry
    unsigned hk[4], c[4];
    u64 key[4];
    bool prev_seed = false;
    unsigned prev_tile = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (p0 + j - e0 >= a.per_entry) e0 += a.per_entry;                     // (at most once per position)
        const float v = WsHeight<HT>::get(h[j]);
        const bool in_m = (WIDE || p0 + j < a.total) && k[j] != 0 && !(v != v) && v != INFINITY;
        const bool seed = in_m && (a.all_seeds || m[j] != bg);
        const unsigned idx = p0 + j - e0;
        hk[j] = in_m ? ws_order(v) : WS_NONE;
        c[j] = seed ? hk[j] : WS_NONE;
        key[j] = seed ? (u64)idx : WS_NONE64;
        if (seed) {
            const unsigned x = idx % (unsigned)a.W, r = idx / (unsigned)a.W;
            const unsigned tile = (e0 / a.per_entry) * a.tiles_per_entry +
                                  ((r / (unsigned)a.EB / (unsigned)a.TA) * (unsigned)a.ntb + r % (unsigned)a.EB / (unsigned)a.TB) * (unsigned)a.ntx + x / (unsigned)a.TX;
            if (!prev_seed || tile != prev_tile) a.seed_flags[tile] = 1u;      // (every writer stores the same value)
            prev_tile = tile;
        }
        prev_seed = seed;
    }
    if constexpr (WIDE) {
        *reinterpret_cast<uint4*>(a.hkey + p0) = make_uint4(hk[0], hk[1], hk[2], hk[3]);
        *reinterpret_cast<uint4*>(a.cost + p0) = make_uint4(c[0], c[1], c[2], c[3]);
        *reinterpret_cast<ulonglong2*>(a.key + p0) = make_ulonglong2(key[0], key[1]);
        *reinterpret_cast<ulonglong2*>(a.key + p0 + 2) = make_ulonglong2(key[2], key[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < a.total) {
                a.hkey[p0 + j] = hk[j];
                a.cost[p0 + j] = c[j];
                a.key[p0 + j] = key[j];
            }
    }
}

// ---------------------------------------------------------------------------------------------------------- relaxation
struct WsRelaxArgs {
    const unsigned* hkey;
    unsigned* cost;             // relaxed by the cost kernel, read by the path kernel
    u64* key;                   // relaxed by the path kernel
    const unsigned* prev;       // [tiles] the tiles' flags of the sweep before (sweep 0: the seed flags)
    unsigned* cur;              // [tiles] ... of this sweep
    unsigned* gate;             // 1 + the last sweep of this phase in which a tile changed
    unsigned sweep;
    unsigned per_entry, tiles_per_entry;
    int EA, EB, W, nta, ntb, ntx;
};

// where a workgroup's tile lies, and what a thread owns in it
template <int DIMS>
struct WsPlace {
    using G = WsTile<DIMS>;
    using L = WsLds<DIMS>;
    unsigned tile;
    size_t ebase;               // the entry's first position
    int ta, tb, tx;             // tile coordinates within the entry
    int x, b, a0;               // the thread's column, middle coordinate and first position along A, within the tile

    __device__ __forceinline__ WsPlace(const WsRelaxArgs& a) {
        tile = blockIdx.x;
        const unsigned e = tile / a.tiles_per_entry;
        unsigned t = tile - e * a.tiles_per_entry;
        ebase = (size_t)e * a.per_entry;
        tx = (int)(t % (unsigned)a.ntx);
        t /= (unsigned)a.ntx;
        tb = (int)(t % (unsigned)a.ntb);
        ta = (int)(t / (unsigned)a.ntb);
        const int rest = (int)threadIdx.x / G::X;
        x = (int)threadIdx.x % G::X;
        b = rest % G::B;
        a0 = rest / G::B * G::RUN;
    }
    // is this tile, or one next to it, flagged?  (workgroup-uniform; a barrier inside)
    __device__ __forceinline__ bool active(const WsRelaxArgs& a) const {
        int act = 0;
        if (threadIdx.x < 27) {
            const int na = ta + (int)threadIdx.x / 9 - 1, nb = tb + (int)threadIdx.x / 3 % 3 - 1, nx = tx + (int)threadIdx.x % 3 - 1;
            if (na >= 0 && na < a.nta && nb >= 0 && nb < a.ntb && nx >= 0 && nx < a.ntx)
                act = a.prev[(tile - ((unsigned)(ta * a.ntb + tb) * (unsigned)a.ntx + (unsigned)tx)) + (unsigned)(na * a.ntb + nb) * (unsigned)a.ntx + (unsigned)nx] != 0u;
        }
        return __syncthreads_or(act) != 0;
    }
    // the position of LDS cell c within the entry, or -1 outside the entry
    __device__ __forceinline__ long long cell_position(const WsRelaxArgs& a, int c) const {
        const int lx = c % L::LX, r = c / L::LX, lb = r % L::LB, la = r / L::LB;
        const int ga = ta * G::A + la - 1, gb = tb * G::B + lb - G::HB, gx = tx * G::X + lx - 1;
        if (ga < 0 || ga >= a.EA || gb < 0 || gb >= a.EB || gx < 0 || gx >= a.W) return -1;
        return ((long long)ga * a.EB + gb) * a.W + gx;
    }
    __device__ __forceinline__ int own_cell(int i) const { return ((a0 + i + 1) * L::LB + b + G::HB) * L::LX + x + 1; }
    __device__ __forceinline__ long long own_position(const WsRelaxArgs& a, int i) const {
        const int ga = ta * G::A + a0 + i, gb = tb * G::B + b, gx = tx * G::X + x;
        if (ga >= a.EA || gb >= a.EB || gx >= a.W) return -1;
        return ((long long)ga * a.EB + gb) * a.W + gx;
    }
    __device__ __forceinline__ void report(const WsRelaxArgs& a, bool changed) const {
        if (threadIdx.x == 0) {
            a.cur[tile] = changed ? 1u : 0u;
            if (changed) __hip_atomic_store(a.gate, a.sweep + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (every writer of a sweep stores the same value)
        }
    }
};

// a sweep runs iff it is the first of its phase or the sweep before it changed something (a tile of THIS sweep may have raised the word already)
__device__ __forceinline__ bool ws_sweep_runs(const WsRelaxArgs& a) {
    return a.sweep == 0u || __hip_atomic_load(a.gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= a.sweep;
}

template <int DIMS, bool FULL>
__global__ __launch_bounds__(WS_THREADS) void ws_cost_kernel(const WsRelaxArgs a) {
    using G = WsTile<DIMS>;
    using L = WsLds<DIMS>;
    __shared__ unsigned sC[L::CELLS];
    if (!ws_sweep_runs(a)) return;
    const WsPlace<DIMS> w(a);
    if (!w.active(a)) {
        w.report(a, false);
        return;
    }
#pragma unroll 1
    for (int c = (int)threadIdx.x; c < L::CELLS; c += WS_THREADS) {
        const long long p = w.cell_position(a, c);
        sC[c] = p >= 0 ? __hip_atomic_load(a.cost + w.ebase + (size_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : WS_NONE;
    }
    unsigned h[G::RUN];
#pragma unroll
    for (int i = 0; i < G::RUN; ++i) {
        const long long p = w.own_position(a, i);
        h[i] = p >= 0 ? a.hkey[w.ebase + (size_t)p] : WS_NONE;                 // (outside the entry: never lowered, never written)
    }
    __syncthreads();

    unsigned dirty = 0u;
    bool changed = false;
#pragma unroll 1
    for (int trip = 0; trip < G::CAP; ++trip) {
        unsigned cur[G::RUN], nb[G::RUN];
#pragma unroll
        for (int i = 0; i < G::RUN; ++i) nb[i] = WS_NONE;
#pragma unroll
        for (int r = -1; r <= G::RUN; ++r) {                                   // level r of the run: its own value, its neighbours in the level, what the levels next to it see
            const int base = w.own_cell(r);
            const unsigned mid = sC[base];
            unsigned in_level = min(sC[base - 1], sC[base + 1]);
            if constexpr (DIMS == 3) {
                in_level = min(in_level, min(sC[base - L::LX], sC[base + L::LX]));
                if constexpr (FULL) in_level = min(min(in_level, min(sC[base - L::LX - 1], sC[base - L::LX + 1])), min(sC[base + L::LX - 1], sC[base + L::LX + 1]));
            }
            const unsigned across = FULL ? min(mid, in_level) : mid;
            if (r >= 0 && r < G::RUN) {
                cur[r] = mid;
                nb[r] = min(nb[r], in_level);
            }
            if (r - 1 >= 0) nb[r - 1] = min(nb[r - 1], across);
            if (r + 1 < G::RUN) nb[r + 1] = min(nb[r + 1], across);
        }
        unsigned v[G::RUN];
#pragma unroll
        for (int i = 0; i < G::RUN; ++i) v[i] = min(cur[i], max(nb[i], h[i]));
#pragma unroll
        for (int i = 1; i < G::RUN; ++i) v[i] = min(v[i], max(v[i - 1], h[i]));        // down the run, then up: in registers
#pragma unroll
        for (int i = G::RUN - 2; i >= 0; --i) v[i] = min(v[i], max(v[i + 1], h[i]));
        unsigned ch = 0u;
#pragma unroll
        for (int i = 0; i < G::RUN; ++i) ch |= v[i] < cur[i] ? 1u << i : 0u;
        __syncthreads();                                                       // every read of this trip is done
#pragma unroll
        for (int i = 0; i < G::RUN; ++i)
            if (ch >> i & 1u) sC[w.own_cell(i)] = v[i];
        dirty |= ch;
        if (!__syncthreads_or(ch != 0u)) break;
        changed = true;
    }
#pragma unroll
    for (int i = 0; i < G::RUN; ++i)
        if (dirty >> i & 1u) {
            const long long p = w.own_position(a, i);
            if (p >= 0) __hip_atomic_store(a.cost + w.ebase + (size_t)p, sC[w.own_cell(i)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    w.report(a, changed);
}

template <int DIMS, bool FULL>
__global__ __launch_bounds__(WS_THREADS) void ws_path_kernel(const WsRelaxArgs a) {
    using G = WsTile<DIMS>;
    using L = WsLds<DIMS>;
    __shared__ u64 sK[L::CELLS];
    __shared__ unsigned sC[L::CELLS];
    if (!ws_sweep_runs(a)) return;
    const WsPlace<DIMS> w(a);
    if (!w.active(a)) {
        w.report(a, false);
        return;
    }
#pragma unroll 1
    for (int c = (int)threadIdx.x; c < L::CELLS; c += WS_THREADS) {
        const long long p = w.cell_position(a, c);
        sK[c] = p >= 0 ? __hip_atomic_load(a.key + w.ebase + (size_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : WS_NONE64;
        sC[c] = p >= 0 ? a.cost[w.ebase + (size_t)p] : WS_NONE;                // (final since the cost phase ended)
    }
    __syncthreads();
    // the largest cost a step INTO position i may come from.  0 where i was not reached -- outside M, or in M without a path -- so
    // that nothing steps into it: every reached position has a cost key above 0 (the key of -inf is 0x007FFFFF)
    unsigned ct[G::RUN];
#pragma unroll
    for (int i = 0; i < G::RUN; ++i) {
        const unsigned c = sC[w.own_cell(i)];
        ct[i] = c == WS_NONE ? 0u : c;
    }

    unsigned dirty = 0u;
    bool changed = false;
#pragma unroll 1
    for (int trip = 0; trip < G::CAP; ++trip) {
        u64 best[G::RUN];
#pragma unroll
        for (int i = 0; i < G::RUN; ++i) best[i] = sK[w.own_cell(i)];
#pragma unroll
        for (int r = -1; r <= G::RUN; ++r) {
            const int base = w.own_cell(r);
#pragma unroll
            for (int db = -G::HB; db <= G::HB; ++db) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int off = (db != 0) + (dx != 0);
                    const bool same = off > 0 && (FULL || off == 1), across = FULL || off == 0;       // whom the cell is a neighbour of: level r, levels r - 1 and r + 1
                    if (!same && !across) continue;
                    const int c = base + db * L::LX + dx;
                    const u64 kq = sK[c];
                    const unsigned cq = sC[c];
                    const u64 k1 = kq == WS_NONE64 ? WS_NONE64 : kq + WS_STEP;
                    auto step_into = [&](int i) {                              // (i is a constant once the loops are unrolled)
                        if (i >= 0 && i < G::RUN && cq <= ct[i]) best[i] = min(best[i], k1);
                    };
                    if (same) step_into(r);
                    if (across) {
                        step_into(r - 1);
                        step_into(r + 1);
                    }
                }
            }
        }
        // down the run, then up, in registers.  (an unreached source has ct 0 and the key WS_NONE64: it passes the first test only
        // towards another unreached position, and the second never)
#pragma unroll
        for (int i = 1; i < G::RUN; ++i)
            if (ct[i - 1] <= ct[i] && best[i - 1] != WS_NONE64) best[i] = min(best[i], best[i - 1] + WS_STEP);
#pragma unroll
        for (int i = G::RUN - 2; i >= 0; --i)
            if (ct[i + 1] <= ct[i] && best[i + 1] != WS_NONE64) best[i] = min(best[i], best[i + 1] + WS_STEP);
        __syncthreads();                                                       // every read of this trip is done
        unsigned ch = 0u;
#pragma unroll
        for (int i = 0; i < G::RUN; ++i)
            if (best[i] < sK[w.own_cell(i)]) {                                 // (its own cell: nobody else writes it)
                sK[w.own_cell(i)] = best[i];
                ch |= 1u << i;
            }
        dirty |= ch;
        if (!__syncthreads_or(ch != 0u)) break;
        changed = true;
    }
#pragma unroll
    for (int i = 0; i < G::RUN; ++i)
        if (dirty >> i & 1u) {
            const long long p = w.own_position(a, i);
            if (p >= 0) __hip_atomic_store(a.key + w.ebase + (size_t)p, sK[w.own_cell(i)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    w.report(a, changed);
}

// ---------------------------------------------------------------------------------------------------------- gather
struct WsGatherArgs {
    const void* markers;
    void* out;                  // markers' element type; must not overlap markers
    const u64* key;
    const unsigned* cost;
    float* cost_out;            // or NULL
    int* seed_out;              // or NULL
    long long fill;             // what an unreached position holds
    unsigned total, per_entry;
};

template <class T, bool WIDE>
__global__ __launch_bounds__(WS_THREADS) void ws_gather_kernel(const WsGatherArgs a) {
    const unsigned p0 = (blockIdx.x * (unsigned)WS_THREADS + threadIdx.x) * 4u;
    if (p0 >= a.total) return;
    const T* markers = reinterpret_cast<const T*>(a.markers);
    T* out = reinterpret_cast<T*>(a.out);
    const T fill = (T)a.fill;
    u64 key[4] = {WS_NONE64, WS_NONE64, WS_NONE64, WS_NONE64};
    unsigned c[4] = {WS_NONE, WS_NONE, WS_NONE, WS_NONE};
    if constexpr (WIDE) {                                                      // total % 4 == 0: all four positions exist (the workspace maps are aligned)
        __builtin_memcpy(key, __builtin_assume_aligned(a.key + p0, 16), sizeof(key));
        if (a.cost_out) __builtin_memcpy(c, __builtin_assume_aligned(a.cost + p0, 16), sizeof(c));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < a.total) {
                key[j] = a.key[p0 + j];
                if (a.cost_out) c[j] = a.cost[p0 + j];
            }
    }
    unsigned e0 = p0 - p0 % a.per_entry;
    T r[4];
    int s[4];
    float f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (p0 + j - e0 >= a.per_entry) e0 += a.per_entry;
        const bool reached = key[j] != WS_NONE64;
        s[j] = reached ? (int)(unsigned)key[j] : -1;                           // 0 <= sigma < per_entry: inside the entry
        r[j] = reached ? markers[e0 + (unsigned)s[j]] : fill;
        f[j] = ws_unorder(reached ? c[j] : WS_NONE);
    }
    if constexpr (WIDE) {
        constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        __builtin_memcpy(__builtin_assume_aligned(out + p0, A), r, sizeof(r));
        if (a.cost_out) *reinterpret_cast<float4*>(a.cost_out + p0) = make_float4(f[0], f[1], f[2], f[3]);
        if (a.seed_out) *reinterpret_cast<int4*>(a.seed_out + p0) = make_int4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < a.total) {
                out[p0 + j] = r[j];
                if (a.cost_out) a.cost_out[p0 + j] = f[j];
                if (a.seed_out) a.seed_out[p0 + j] = s[j];
            }
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
// The workspace: 16 bytes of sweep words (one per phase), the tiles' seed flags and their two sweep flags (4 bytes each), then per
// position the height key (4), the cost key (4) and the path key (8).
struct WsPlan {
    int dims, EA, EB, W, nta, ntb, ntx, TA, TB, TX;
    long long B, total, per_entry, tiles_per_entry, tiles;
    long long off_gate, off_seed, off_flags, off_hkey, off_cost, off_key, bytes;
};

static int ws_plan(int dims, long long B, long long D, long long H, long long W, int flags, WsPlan& p) {
    if ((dims != 2 && dims != 3) || B < 1 || D < 1 || H < 1 || W < 1 || (dims == 2 && D != 1)) return PTB_EINVAL;
    if (flags & ~(PTB_WATERSHED_COST | PTB_WATERSHED_SEED)) return PTB_EINVAL;
    if (D > EDT_MAX_POS || H > EDT_MAX_POS || W > EDT_MAX_POS || H * W > EDT_MAX_POS || D * H * W > EDT_MAX_POS || B > EDT_MAX_POS / (D * H * W)) return PTB_EUNSUPPORTED;
    p.dims = dims; p.B = B; p.W = (int)W;
    p.EA = dims == 2 ? (int)H : (int)D; p.EB = dims == 2 ? 1 : (int)H;
    p.TA = dims == 2 ? WsTile<2>::A : WsTile<3>::A; p.TB = dims == 2 ? WsTile<2>::B : WsTile<3>::B; p.TX = dims == 2 ? WsTile<2>::X : WsTile<3>::X;
    p.nta = (p.EA + p.TA - 1) / p.TA; p.ntb = (p.EB + p.TB - 1) / p.TB; p.ntx = (p.W + p.TX - 1) / p.TX;
    p.per_entry = D * H * W; p.total = B * p.per_entry;
    p.tiles_per_entry = (long long)p.nta * p.ntb * p.ntx; p.tiles = B * p.tiles_per_entry;       // (a tile holds a position: tiles <= total)
    long long o = 0;
    p.off_gate = o; o += 16;
    p.off_seed = o; o += edt_up16(4 * p.tiles);
    p.off_flags = o; o += 2 * edt_up16(4 * p.tiles);
    p.off_hkey = o; o += edt_up16(4 * p.total);
    p.off_cost = o; o += edt_up16(4 * p.total);
    p.off_key = o; o += edt_up16(8 * p.total);
    p.bytes = o;
    return PTB_OK;
}

static int ws_hip(hipError_t e) {
    if (e == hipSuccess) return PTB_OK;
    set_hip_error(e);
    return PTB_ELAUNCH;
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_watershed_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int flags, int64_t* workspace_bytes) {
    WsPlan p;
    if (int rc = ws_plan(dims, B, D, H, W, flags, p)) return rc;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return PTB_OK;
}

extern "C" int ptb_watershed(const void* height, int height_dtype, const void* markers, int marker_bytes, const void* mask, int dims, int64_t B, int64_t D,
                             int64_t H, int64_t W, int connectivity, int64_t background, int64_t fill, int flags, int max_sweeps, void* labels_out,
                             float* cost_out, int32_t* seed_out, int32_t* sweeps_out, void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (sweeps_out) sweeps_out[0] = sweeps_out[1] = -1;
    if (!height || !markers || !labels_out || !workspace) return PTB_EINVAL;
    if (height_dtype != PTB_F32 && height_dtype != PTB_F16 && height_dtype != PTB_BF16 && height_dtype != PTB_U8 && height_dtype != PTB_I16) return PTB_EINVAL;
    if (marker_bytes != 1 && marker_bytes != 2 && marker_bytes != 4 && marker_bytes != 8) return PTB_EINVAL;
    WsPlan p;
    if (int rc = ws_plan(dims, B, D, H, W, flags, p)) return rc;
    if (dims == 2 ? (connectivity != 4 && connectivity != 8) : (connectivity != 6 && connectivity != 26)) return PTB_EINVAL;
    if (((flags & PTB_WATERSHED_COST) != 0) != (cost_out != nullptr) || ((flags & PTB_WATERSHED_SEED) != 0) != (seed_out != nullptr)) return PTB_EINVAL;
    if (max_sweeps < 1) return PTB_EINVAL;
    if (workspace_bytes < p.bytes || !aligned16(workspace) || !aligned16(labels_out) || !aligned16(cost_out) || !aligned16(seed_out)) return PTB_EINVAL;
    if (labels_out == markers) return PTB_EINVAL;                              // the gather reads markers at other positions than it writes
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const bool full = connectivity == 8 || connectivity == 26;
    const int height_bytes = height_dtype == PTB_F32 ? 4 : height_dtype == PTB_U8 ? 1 : 2;
    unsigned* gates = reinterpret_cast<unsigned*>(ws + p.off_gate);
    unsigned* seed_flags = reinterpret_cast<unsigned*>(ws + p.off_seed);
    unsigned* tile_flags[2] = {reinterpret_cast<unsigned*>(ws + p.off_flags), reinterpret_cast<unsigned*>(ws + p.off_flags + edt_up16(4 * p.tiles))};

    if (int rc = ws_hip(hipMemsetAsync(ws, 0, (size_t)(p.off_flags - p.off_gate), st))) return rc;      // the sweep words and the seed flags
    WsInitArgs in{};
    in.height = height; in.markers = markers; in.mask = reinterpret_cast<const unsigned char*>(mask);
    in.hkey = reinterpret_cast<unsigned*>(ws + p.off_hkey); in.cost = reinterpret_cast<unsigned*>(ws + p.off_cost); in.key = reinterpret_cast<u64*>(ws + p.off_key);
    in.seed_flags = seed_flags; in.background = background;
    in.total = (unsigned)p.total; in.per_entry = (unsigned)p.per_entry; in.tiles_per_entry = (unsigned)p.tiles_per_entry;
    in.EB = p.EB; in.W = p.W; in.TA = p.TA; in.TB = p.TB; in.TX = p.TX; in.ntb = p.ntb; in.ntx = p.ntx;
    in.all_seeds = !edt_holds(marker_bytes, background);                       // a background the element type cannot hold occurs nowhere
    const bool markers_wide = p.total % 4 == 0 && reinterpret_cast<uintptr_t>(markers) % std::min(4 * marker_bytes, 16) == 0;
    const bool wide = markers_wide && reinterpret_cast<uintptr_t>(height) % std::min(4 * height_bytes, 16) == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0;
    const unsigned blocks = (unsigned)((p.total + 4 * WS_THREADS - 1) / (4 * WS_THREADS));
    with_value<PTB_F32, PTB_F16, PTB_BF16, PTB_U8, PTB_I16>(height_dtype, [&](auto ht) {
        with_value<1, 2, 4, 8>(marker_bytes, [&](auto eb) {
            using T = edt_label_t<eb()>;
            with_bool(wide, [&](auto wd) {
                hipLaunchKernelGGL((ws_init_kernel<ht(), T, wd()>), dim3(blocks), dim3(WS_THREADS), 0, st, in);
            });
        });
    });

    WsRelaxArgs r{};
    r.hkey = in.hkey; r.cost = in.cost; r.key = in.key;
    r.per_entry = in.per_entry; r.tiles_per_entry = in.tiles_per_entry;
    r.EA = p.EA; r.EB = p.EB; r.W = p.W; r.nta = p.nta; r.ntb = p.ntb; r.ntx = p.ntx;
    for (int phase = 0; phase < 2; ++phase) {
        r.gate = gates + phase;
        int done = 0;
        for (;;) {                                                             // (each trip launches at least one sweep: at most max_sweeps trips)
            const int n = std::min(WS_BATCH, max_sweeps - done);
            for (int k = done; k < done + n; ++k) {
                r.sweep = (unsigned)k;
                r.prev = k == 0 ? seed_flags : tile_flags[(k - 1) & 1];
                r.cur = tile_flags[k & 1];
                with_value<2, 3>(p.dims, [&](auto dm) {
                    with_bool(full, [&](auto fl) {
                        if (phase == 0) hipLaunchKernelGGL((ws_cost_kernel<dm(), fl()>), dim3((unsigned)p.tiles), dim3(WS_THREADS), 0, st, r);
                        else hipLaunchKernelGGL((ws_path_kernel<dm(), fl()>), dim3((unsigned)p.tiles), dim3(WS_THREADS), 0, st, r);
                    });
                });
            }
            done += n;
            if (int rc = check_launch()) return rc;
            unsigned last = 0;                                                 // 1 + the last sweep that changed something
            if (int rc = ws_hip(hipMemcpyAsync(&last, r.gate, sizeof(last), hipMemcpyDeviceToHost, st))) return rc;
            if (int rc = ws_hip(hipStreamSynchronize(st))) return rc;
            if (last < (unsigned)done) {                                       // sweep `last` ran and changed nothing
                if (sweeps_out) sweeps_out[phase] = (int)last + 1;
                break;
            }
            if (done >= max_sweeps) {
                if (sweeps_out) sweeps_out[phase] = done;
                return PTB_ENOTCONVERGED;
            }
        }
    }

    WsGatherArgs g{};
    g.markers = markers; g.out = labels_out; g.key = in.key; g.cost = in.cost; g.cost_out = cost_out; g.seed_out = seed_out; g.fill = fill;
    g.total = in.total; g.per_entry = in.per_entry;
    with_value<1, 2, 4, 8>(marker_bytes, [&](auto eb) {
        using T = edt_label_t<eb()>;
        with_bool(markers_wide, [&](auto wd) {
            hipLaunchKernelGGL((ws_gather_kernel<T, wd()>), dim3(blocks), dim3(WS_THREADS), 0, st, g);
        });
    });
    return check_launch();
}
