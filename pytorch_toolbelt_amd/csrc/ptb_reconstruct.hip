// Morphological reconstruction and what is built on it (utils/reconstruct.py; the reference has no counterpart): grey reconstruction by
// dilation / erosion, regional extrema, h-extrema and hole filling, all as THE LEAST FIXED POINT OF ONE MONOTONE RULE
//     R(p) <- max(R(p), min(R(q), mask(p)))   over the neighbours q of p inside the domain, from R = min(seed, mask).
// min and max only select, so no order of relaxation and no tie rule enters the result: it is a function of the inputs alone.
// ONE KEY SPACE.  Every value becomes an ordered 32-bit key: the float32 bits mapped monotonically, -0 as +0.  Reconstruction by
// EROSION is the same rule on the COMPLEMENTED key (flip = 0xFFFFFFFF), not a second kernel.  The keys of the non-NaN values lie in
// [0x007FFFFF, 0xFF800000], flipped or not; 0 is the key of a position OUTSIDE THE DOMAIN (domain == 0, or a NaN in the mask): its mask
// key and its R are 0, so the rule never raises it and it never raises a neighbour.
//   1. rc_init_kernel     one pass over the value map(s) and the domain, read where they lie: the mask key, the start of R (from the seed
//                         map; the mask one key step down; float32(mask) - h; or the mask on the faces of the entry and the lowest key
//                         elsewhere) and a flag for every tile sweep 0 has to run (holds a domain position; hole filling: one on a face).
//   2. rc_relax_kernel    a workgroup owns a tile (2-D: 64 x 64; 3-D: a brick 8 x 8 x 32) and holds its R with a one-position halo in LDS.  A
//                         thread owns a run of positions along the slowest axis of the tile: it takes the maximum of the neighbours in LDS,
//                         then relaxes down and up its run in registers.  Barriers separate the reads of a trip from its writes, a workgroup-wide
//                         vote ends the trips, the trip cap bounds them (a tile that ends at the cap has changed, so it runs again).  Only the
//                         owning tile writes a position, and only the positions that changed.  Halo reads and the write-back are relaxed
//                         agent-scope 32-bit accesses; a stale halo value is one the fixed point lies above as well.
//   3. rc_restage_kernel  between the two phases of the h-extrema: R becomes the mask, the start of the second phase is R one key step down.
//   4. rc_gather_kernel   R back as a value of the source type (outside the domain: the mask's own element),
//      rc_compare_kernel  or the bool map R < mask (the extrema).
// TILE ACTIVITY, as in ptb_watershed.hip: a tile runs in sweep k iff it or a tile next to it changed in sweep k - 1 (sweep 0: the init
// kernel's flags); it writes its own flag of sweep k, zero included.  One word per phase holds 1 + the last sweep that changed anything: a
// sweep whose predecessor changed nothing returns at once, and the host reads that word back after every RC_BATCH launches.
// EVERY LOOP IS BOUNDED (the trips by the cap, the sweeps by max_sweeps).  No workgroup waits for another one; there are no atomic
// read-modify-writes at all.
#include <algorithm>
#include <cmath>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_edt_common.h"

namespace ptb {

constexpr unsigned RC_OUTSIDE = 0u;             // the key of a position outside the domain
constexpr unsigned RC_LOWEST = 0x007FFFFFu;     // the smallest key of a value: -inf (flipped: +inf)
constexpr int RC_THREADS = 256;
constexpr int RC_BATCH = 8;                     // sweeps launched between two read-backs of the "changed" word

enum { RC_START_SEED = 0, RC_START_STEP = 1, RC_START_H = 2, RC_START_FACES = 3 };

// a tile: A x B x X positions along (slowest, middle, fastest); a thread owns RUN consecutive positions along A.  2-D: A = rows, no
// middle axis (HB: its halo).  A / RUN * B * X == RC_THREADS.
template <int DIMS>
struct RcTile;
template <>
struct RcTile<2> {
    static constexpr int A = 64, B = 1, X = 64, RUN = 16, HB = 0, CAP = 64;
};
template <>
struct RcTile<3> {
    static constexpr int A = 8, B = 8, X = 32, RUN = 8, HB = 1, CAP = 32;
};
template <int DIMS>
struct RcLds {
    using G = RcTile<DIMS>;
    static constexpr int LB = G::B + 2 * G::HB, LX = G::X + 2, CELLS = (G::A + 2) * LB * LX;
    static_assert(G::A / G::RUN * G::B * G::X == RC_THREADS && G::A % G::RUN == 0, "a thread per run");
    static_assert(CELLS * 4 <= 32 * 1024, "at least four workgroups per CU by LDS");
};

// monotone: a < b <=> rc_order(a, 0) < rc_order(b, 0) <=> rc_order(a, ~0) > rc_order(b, ~0); -0 as +0
__device__ __forceinline__ unsigned rc_order(float v, unsigned flip) {
    unsigned b = __float_as_uint(v);
    if (v == 0.0f) b = 0u;
    return ((b & 0x80000000u) ? ~b : (b | 0x80000000u)) ^ flip;
}
__device__ __forceinline__ float rc_unorder(unsigned k, unsigned flip) {
    k ^= flip;
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// element types of the value maps: every value is exact in float32, and put() gets back a value the type holds (the gather kernel has
// capped the one infinity no input held: the start of a position that no face reaches in hole filling)
template <int DT>
struct RcValue;
template <>
struct RcValue<PTB_F32> {
    using R = float;
    static __device__ __forceinline__ float get(R v) { return v; }
    static __device__ __forceinline__ R put(float v) { return v; }
};
template <>
struct RcValue<PTB_F16> {
    using R = _Float16;
    static __device__ __forceinline__ float get(R v) { return (float)v; }
    static __device__ __forceinline__ R put(float v) { return (_Float16)v; }
};
template <>
struct RcValue<PTB_BF16> {
    using R = unsigned short;
    static __device__ __forceinline__ float get(R v) { return __uint_as_float((unsigned)v << 16); }
    static __device__ __forceinline__ R put(float v) { return (unsigned short)(__float_as_uint(v) >> 16); }
};
template <>
struct RcValue<PTB_U8> {
    using R = unsigned char;
    static __device__ __forceinline__ float get(R v) { return (float)v; }
    static __device__ __forceinline__ R put(float v) { return (R)v; }
};
template <>
struct RcValue<PTB_I16> {
    using R = short;
    static __device__ __forceinline__ float get(R v) { return (float)v; }
    static __device__ __forceinline__ R put(float v) { return (R)v; }
};

// ---------------------------------------------------------------------------------------------------------- init
struct RcInitArgs {
    const void* seed;           // RC_START_SEED only
    const void* mask;
    const unsigned char* domain;        // or NULL
    unsigned* mkey;             // [total] the key of the mask, RC_OUTSIDE outside the domain
    unsigned* r;                // [total] the start of R: <= mkey
    unsigned* start_flags;      // [tiles] zeroed by the caller: 1 where sweep 0 runs the tile
    unsigned flip;
    float h;                    // RC_START_H: the start is float32(mask) - h (the caller negates h for the minima)
    int start;
    unsigned total, per_entry, tiles_per_entry;
    int EA, EB, W, TA, TB, TX, ntb, ntx, HB;
};

template <int DT, bool TWO, bool WIDE>
__global__ __launch_bounds__(RC_THREADS) void rc_init_kernel(const RcInitArgs a) {
    using V = RcValue<DT>;
    using R = typename V::R;
    const unsigned p0 = (blockIdx.x * (unsigned)RC_THREADS + threadIdx.x) * 4u;                  // (total <= 2^31 - 2: p0 + 3 fits 32 bits)
    if (p0 >= a.total) return;
    const R* mask = reinterpret_cast<const R*>(a.mask);
    const R* seed = reinterpret_cast<const R*>(a.seed);
    R m[4] = {(R)0, (R)0, (R)0, (R)0}, s[4] = {(R)0, (R)0, (R)0, (R)0};
    unsigned char k[4] = {1, 1, 1, 1};
    if constexpr (WIDE) {                                                      // total % 4 == 0 and aligned bases: all four positions exist
        constexpr int AL = sizeof(R) * 4 < 16 ? sizeof(R) * 4 : 16;
        __builtin_memcpy(m, __builtin_assume_aligned(mask + p0, AL), sizeof(m));
        if constexpr (TWO) __builtin_memcpy(s, __builtin_assume_aligned(seed + p0, AL), sizeof(s));
        if (a.domain) __builtin_memcpy(k, __builtin_assume_aligned(a.domain + p0, 4), sizeof(k));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < a.total) {
                m[j] = mask[p0 + j];
                if constexpr (TWO) s[j] = seed[p0 + j];
                if (a.domain) k[j] = a.domain[p0 + j];
            }
    }
    unsigned e0 = p0 - p0 % a.per_entry;                                       // the first position of p0's entry
    unsigned mk[4], r0[4];
    bool prev_flag = false;
    unsigned prev_tile = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (p0 + j - e0 >= a.per_entry) e0 += a.per_entry;                     // (at most once per position)
        const float v = V::get(m[j]);
        const bool in = (WIDE || p0 + j < a.total) && k[j] != 0 && !(v != v);
        mk[j] = RC_OUTSIDE;
        r0[j] = RC_OUTSIDE;
        bool flag = false;
        if (in) {
            const unsigned idx = p0 + j - e0;
            const unsigned x = idx % (unsigned)a.W, row = idx / (unsigned)a.W;
            const unsigned pa = row / (unsigned)a.EB, pb = row % (unsigned)a.EB;
            mk[j] = rc_order(v, a.flip);
            unsigned st;
            if constexpr (TWO) {
                const float sv = V::get(s[j]);
                st = sv != sv ? RC_LOWEST : rc_order(sv, a.flip);              // a NaN in the seed: the lowest value (erosion: the highest)
            } else if (a.start == RC_START_STEP) {
                st = mk[j] - 1u;                                               // (mk >= RC_LOWEST > 0: no underflow)
            } else if (a.start == RC_START_H) {
                st = rc_order(v - a.h, a.flip);                                // one float32 subtraction (h finite: never a NaN)
            } else {
                const bool face = x == 0u || x + 1u == (unsigned)a.W || pa == 0u || pa + 1u == (unsigned)a.EA || (a.HB && (pb == 0u || pb + 1u == (unsigned)a.EB));
                st = face ? mk[j] : RC_LOWEST;
                flag = face;
            }
            r0[j] = min(st, mk[j]);                                            // the clamp: seed > mask starts at the mask
            if (a.start != RC_START_FACES) flag = true;
            if (flag) {
                const unsigned tile = (e0 / a.per_entry) * a.tiles_per_entry + ((pa / (unsigned)a.TA) * (unsigned)a.ntb + pb / (unsigned)a.TB) * (unsigned)a.ntx + x / (unsigned)a.TX;
                if (!prev_flag || tile != prev_tile) a.start_flags[tile] = 1u;  // (every writer stores the same value)
                prev_tile = tile;
            }
        }
        prev_flag = flag;
    }
    if constexpr (WIDE) {
        *reinterpret_cast<uint4*>(a.mkey + p0) = make_uint4(mk[0], mk[1], mk[2], mk[3]);
        *reinterpret_cast<uint4*>(a.r + p0) = make_uint4(r0[0], r0[1], r0[2], r0[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < a.total) {
                a.mkey[p0 + j] = mk[j];
                a.r[p0 + j] = r0[j];
            }
    }
}

// ---------------------------------------------------------------------------------------------------------- relaxation
struct RcRelaxArgs {
    const unsigned* mkey;
    unsigned* r;
    const unsigned* prev;       // [tiles] the tiles' flags of the sweep before (sweep 0: the start flags)
    unsigned* cur;              // [tiles] ... of this sweep
    unsigned* gate;             // 1 + the last sweep of this phase in which a tile changed
    unsigned sweep;
    unsigned per_entry, tiles_per_entry;
    int EA, EB, W, nta, ntb, ntx;
};

// where a workgroup's tile lies, and what a thread owns in it
template <int DIMS>
struct RcPlace {
    using G = RcTile<DIMS>;
    using L = RcLds<DIMS>;
    unsigned tile, first;       // this tile, and the first tile of its entry
    size_t ebase;               // the entry's first position
    int ta, tb, tx;             // tile coordinates within the entry
    int x, b, a0;               // the thread's column, middle coordinate and first position along A, within the tile

    __device__ __forceinline__ RcPlace(const RcRelaxArgs& a) {
        tile = blockIdx.x;
        const unsigned e = tile / a.tiles_per_entry;
        first = e * a.tiles_per_entry;
        unsigned t = tile - first;
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
    __device__ __forceinline__ bool active(const RcRelaxArgs& a) const {
        int act = 0;
        if (threadIdx.x < 27) {
            const int na = ta + (int)threadIdx.x / 9 - 1, nb = tb + (int)threadIdx.x / 3 % 3 - 1, nx = tx + (int)threadIdx.x % 3 - 1;
            if (na >= 0 && na < a.nta && nb >= 0 && nb < a.ntb && nx >= 0 && nx < a.ntx)
                act = a.prev[first + (unsigned)(na * a.ntb + nb) * (unsigned)a.ntx + (unsigned)nx] != 0u;
        }
        return __syncthreads_or(act) != 0;
    }
    // the position of LDS cell c within the entry, or -1 outside the entry
    __device__ __forceinline__ long long cell_position(const RcRelaxArgs& a, int c) const {
        const int lx = c % L::LX, rest = c / L::LX, lb = rest % L::LB, la = rest / L::LB;
        const int ga = ta * G::A + la - 1, gb = tb * G::B + lb - G::HB, gx = tx * G::X + lx - 1;
        if (ga < 0 || ga >= a.EA || gb < 0 || gb >= a.EB || gx < 0 || gx >= a.W) return -1;
        return ((long long)ga * a.EB + gb) * a.W + gx;
    }
    __device__ __forceinline__ int own_cell(int i) const { return ((a0 + i + 1) * L::LB + b + G::HB) * L::LX + x + 1; }
    __device__ __forceinline__ long long own_position(const RcRelaxArgs& a, int i) const {
        const int ga = ta * G::A + a0 + i, gb = tb * G::B + b, gx = tx * G::X + x;
        if (ga >= a.EA || gb >= a.EB || gx >= a.W) return -1;
        return ((long long)ga * a.EB + gb) * a.W + gx;
    }
    __device__ __forceinline__ void report(const RcRelaxArgs& a, bool changed) const {
        if (threadIdx.x == 0) {
            a.cur[tile] = changed ? 1u : 0u;
            if (changed) __hip_atomic_store(a.gate, a.sweep + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (every writer of a sweep stores the same value)
        }
    }
};

template <int DIMS, bool FULL>
__global__ __launch_bounds__(RC_THREADS) void rc_relax_kernel(const RcRelaxArgs a) {
    using G = RcTile<DIMS>;
    using L = RcLds<DIMS>;
    __shared__ unsigned sR[L::CELLS];
    // a sweep runs iff it is the first of its phase or the sweep before it changed something (a tile of THIS sweep may have raised the word already)
    if (a.sweep != 0u && __hip_atomic_load(a.gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < a.sweep) return;
    const RcPlace<DIMS> w(a);
    if (!w.active(a)) {
        w.report(a, false);
        return;
    }
#pragma unroll 1
    for (int c = (int)threadIdx.x; c < L::CELLS; c += RC_THREADS) {
        const long long p = w.cell_position(a, c);
        sR[c] = p >= 0 ? __hip_atomic_load(a.r + w.ebase + (size_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : RC_OUTSIDE;
    }
    unsigned m[G::RUN];
#pragma unroll
    for (int i = 0; i < G::RUN; ++i) {
        const long long p = w.own_position(a, i);
        m[i] = p >= 0 ? a.mkey[w.ebase + (size_t)p] : RC_OUTSIDE;              // (outside the entry: never raised, never written)
    }
    __syncthreads();

    unsigned dirty = 0u;
    bool changed = false;
#pragma unroll 1
    for (int trip = 0; trip < G::CAP; ++trip) {
        unsigned cur[G::RUN], nb[G::RUN];
#pragma unroll
        for (int i = 0; i < G::RUN; ++i) nb[i] = RC_OUTSIDE;
#pragma unroll
        for (int lv = -1; lv <= G::RUN; ++lv) {                                // level lv of the run: its own value, its neighbours in the level, what the levels next to it see
            const int base = w.own_cell(lv);
            const unsigned mid = sR[base];
            unsigned in_level = max(sR[base - 1], sR[base + 1]);
            if constexpr (DIMS == 3) {
                in_level = max(in_level, max(sR[base - L::LX], sR[base + L::LX]));
                if constexpr (FULL) in_level = max(max(in_level, max(sR[base - L::LX - 1], sR[base - L::LX + 1])), max(sR[base + L::LX - 1], sR[base + L::LX + 1]));
            }
            const unsigned across = FULL ? max(mid, in_level) : mid;
            if (lv >= 0 && lv < G::RUN) {
                cur[lv] = mid;
                nb[lv] = max(nb[lv], in_level);
            }
            if (lv - 1 >= 0) nb[lv - 1] = max(nb[lv - 1], across);
            if (lv + 1 < G::RUN) nb[lv + 1] = max(nb[lv + 1], across);
        }
        unsigned v[G::RUN];
#pragma unroll
        for (int i = 0; i < G::RUN; ++i) v[i] = max(cur[i], min(nb[i], m[i]));
#pragma unroll
        for (int i = 1; i < G::RUN; ++i) v[i] = max(v[i], min(v[i - 1], m[i]));         // down the run, then up: in registers
#pragma unroll
        for (int i = G::RUN - 2; i >= 0; --i) v[i] = max(v[i], min(v[i + 1], m[i]));
        unsigned ch = 0u;
#pragma unroll
        for (int i = 0; i < G::RUN; ++i) ch |= v[i] > cur[i] ? 1u << i : 0u;
        __syncthreads();                                                       // every read of this trip is done
#pragma unroll
        for (int i = 0; i < G::RUN; ++i)
            if (ch >> i & 1u) sR[w.own_cell(i)] = v[i];
        dirty |= ch;
        if (!__syncthreads_or(ch != 0u)) break;
        changed = true;
    }
#pragma unroll
    for (int i = 0; i < G::RUN; ++i)
        if (dirty >> i & 1u) {
            const long long p = w.own_position(a, i);                          // (a changed position has a mask key above 0: it lies inside the entry)
            if (p >= 0) __hip_atomic_store(a.r + w.ebase + (size_t)p, sR[w.own_cell(i)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    w.report(a, changed);
}

// ---------------------------------------------------------------------------------------------------------- restage, gather
// between the phases of the h-extrema: mask <- R, R <- R one key step down (outside the domain both stay 0)
template <bool WIDE>
__global__ __launch_bounds__(RC_THREADS) void rc_restage_kernel(unsigned* mkey, unsigned* r, unsigned total) {
    const unsigned p0 = (blockIdx.x * (unsigned)RC_THREADS + threadIdx.x) * 4u;
    if (p0 >= total) return;
    if constexpr (WIDE) {
        const uint4 v = *reinterpret_cast<const uint4*>(r + p0);
        *reinterpret_cast<uint4*>(mkey + p0) = v;
        *reinterpret_cast<uint4*>(r + p0) = make_uint4(v.x ? v.x - 1u : 0u, v.y ? v.y - 1u : 0u, v.z ? v.z - 1u : 0u, v.w ? v.w - 1u : 0u);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < total) {
                const unsigned v = r[p0 + j];
                mkey[p0 + j] = v;
                r[p0 + j] = v ? v - 1u : 0u;
            }
    }
}

// R as values of the source type; outside the domain the mask's own element.  out may be the mask itself (a thread reads its four
// positions before it writes them) but must not overlap it otherwise.
template <int DT, bool WIDE>
__global__ __launch_bounds__(RC_THREADS) void rc_gather_kernel(const void* mask_, void* out_, const unsigned* r, unsigned flip, float top, unsigned total) {
    using V = RcValue<DT>;
    using R = typename V::R;
    const unsigned p0 = (blockIdx.x * (unsigned)RC_THREADS + threadIdx.x) * 4u;
    if (p0 >= total) return;
    const R* mask = reinterpret_cast<const R*>(mask_);
    R* out = reinterpret_cast<R*>(out_);
    unsigned k[4] = {RC_OUTSIDE, RC_OUTSIDE, RC_OUTSIDE, RC_OUTSIDE};
    R m[4] = {(R)0, (R)0, (R)0, (R)0};
    constexpr int AL = sizeof(R) * 4 < 16 ? sizeof(R) * 4 : 16;
    if constexpr (WIDE) {                                                      // total % 4 == 0, the mask aligned (out and the workspace always are)
        __builtin_memcpy(k, __builtin_assume_aligned(r + p0, 16), sizeof(k));
        __builtin_memcpy(m, __builtin_assume_aligned(mask + p0, AL), sizeof(m));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < total) {
                k[j] = r[p0 + j];
                m[j] = mask[p0 + j];
            }
    }
    R o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = k[j] == RC_OUTSIDE ? m[j] : V::put(fminf(rc_unorder(k[j], flip), top));
    if constexpr (WIDE) {
        __builtin_memcpy(__builtin_assume_aligned(out + p0, AL), o, sizeof(o));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < total) out[p0 + j] = o[j];
    }
}

// the extrema: R < mask (both 0 outside the domain: false)
template <bool WIDE>
__global__ __launch_bounds__(RC_THREADS) void rc_compare_kernel(const unsigned* mkey, const unsigned* r, unsigned char* out, unsigned total) {
    const unsigned p0 = (blockIdx.x * (unsigned)RC_THREADS + threadIdx.x) * 4u;
    if (p0 >= total) return;
    if constexpr (WIDE) {
        const uint4 m = *reinterpret_cast<const uint4*>(mkey + p0), v = *reinterpret_cast<const uint4*>(r + p0);
        *reinterpret_cast<uchar4*>(out + p0) = make_uchar4(v.x < m.x, v.y < m.y, v.z < m.z, v.w < m.w);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < total) out[p0 + j] = r[p0 + j] < mkey[p0 + j];
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
// The workspace: 16 bytes of sweep words (one per phase), the tiles' start flags and their two sweep flags (4 bytes each), then per
// position the mask key (4) and R (4).
struct RcPlan {
    int dims, EA, EB, W, nta, ntb, ntx, TA, TB, TX;
    long long B, total, per_entry, tiles_per_entry, tiles;
    long long off_gate, off_start, off_flags, off_mkey, off_r, bytes;
};

static int rc_plan(int dims, long long B, long long D, long long H, long long W, int op, RcPlan& p) {
    if ((dims != 2 && dims != 3) || B < 1 || D < 1 || H < 1 || W < 1 || (dims == 2 && D != 1)) return PTB_EINVAL;
    if (op < PTB_RECONSTRUCT_VALUES || op > PTB_RECONSTRUCT_FILL) return PTB_EINVAL;
    if (D > EDT_MAX_POS || H > EDT_MAX_POS || W > EDT_MAX_POS || H * W > EDT_MAX_POS || D * H * W > EDT_MAX_POS || B > EDT_MAX_POS / (D * H * W)) return PTB_EUNSUPPORTED;
    p.dims = dims; p.B = B; p.W = (int)W;
    p.EA = dims == 2 ? (int)H : (int)D; p.EB = dims == 2 ? 1 : (int)H;
    p.TA = dims == 2 ? RcTile<2>::A : RcTile<3>::A; p.TB = dims == 2 ? RcTile<2>::B : RcTile<3>::B; p.TX = dims == 2 ? RcTile<2>::X : RcTile<3>::X;
    p.nta = (p.EA + p.TA - 1) / p.TA; p.ntb = (p.EB + p.TB - 1) / p.TB; p.ntx = (p.W + p.TX - 1) / p.TX;
    p.per_entry = D * H * W; p.total = B * p.per_entry;
    p.tiles_per_entry = (long long)p.nta * p.ntb * p.ntx; p.tiles = B * p.tiles_per_entry;       // (a tile holds a position: tiles <= total)
    long long o = 0;
    p.off_gate = o; o += 16;
    p.off_start = o; o += edt_up16(4 * p.tiles);
    p.off_flags = o; o += 2 * edt_up16(4 * p.tiles);
    p.off_mkey = o; o += edt_up16(4 * p.total);
    p.off_r = o; o += edt_up16(4 * p.total);
    p.bytes = o;
    return PTB_OK;
}

static int rc_hip(hipError_t e) {
    if (e == hipSuccess) return PTB_OK;
    set_hip_error(e);
    return PTB_ELAUNCH;
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_reconstruct_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int op, int64_t* workspace_bytes) {
    RcPlan p;
    if (int rc = rc_plan(dims, B, D, H, W, op, p)) return rc;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return PTB_OK;
}

extern "C" int ptb_reconstruct(const void* seed, const void* mask, int dtype, const void* domain, int dims, int64_t B, int64_t D, int64_t H, int64_t W,
                               int connectivity, int op, int erosion, float h, float top, int max_sweeps, void* out, int32_t* sweeps_out, void* workspace,
                               int64_t workspace_bytes, ptb_stream_t stream) {
    if (sweeps_out) sweeps_out[0] = sweeps_out[1] = -1;
    if (!mask || !out || !workspace) return PTB_EINVAL;
    if (dtype != PTB_F32 && dtype != PTB_F16 && dtype != PTB_BF16 && dtype != PTB_U8 && dtype != PTB_I16) return PTB_EINVAL;
    RcPlan p;
    if (int rc = rc_plan(dims, B, D, H, W, op, p)) return rc;
    if (dims == 2 ? (connectivity != 4 && connectivity != 8) : (connectivity != 6 && connectivity != 26)) return PTB_EINVAL;
    if ((op == PTB_RECONSTRUCT_VALUES) != (seed != nullptr)) return PTB_EINVAL;
    if ((erosion != 0 && erosion != 1) || (op == PTB_RECONSTRUCT_FILL && !erosion)) return PTB_EINVAL;
    if (op == PTB_RECONSTRUCT_H_EXTREMA ? !(h >= 0.0f && std::isfinite(h)) : h != 0.0f) return PTB_EINVAL;
    if (op == PTB_RECONSTRUCT_FILL ? top != top : top != INFINITY) return PTB_EINVAL;
    if (max_sweeps < 1) return PTB_EINVAL;
    if (workspace_bytes < p.bytes || !aligned16(workspace) || !aligned16(out)) return PTB_EINVAL;
    const bool values = op == PTB_RECONSTRUCT_VALUES || op == PTB_RECONSTRUCT_FILL;
    if (out == seed) return PTB_EINVAL;                                        // (out == mask is fine: see rc_gather_kernel)
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const bool full = connectivity == 8 || connectivity == 26;
    const int elem = dtype == PTB_F32 ? 4 : dtype == PTB_U8 ? 1 : 2;
    unsigned* gates = reinterpret_cast<unsigned*>(ws + p.off_gate);
    unsigned* start_flags = reinterpret_cast<unsigned*>(ws + p.off_start);
    unsigned* tile_flags[2] = {reinterpret_cast<unsigned*>(ws + p.off_flags), reinterpret_cast<unsigned*>(ws + p.off_flags + edt_up16(4 * p.tiles))};

    if (int rc = rc_hip(hipMemsetAsync(ws, 0, (size_t)(p.off_flags - p.off_gate), st))) return rc;      // the sweep words and the start flags
    RcInitArgs in{};
    in.seed = seed; in.mask = mask; in.domain = reinterpret_cast<const unsigned char*>(domain);
    in.mkey = reinterpret_cast<unsigned*>(ws + p.off_mkey); in.r = reinterpret_cast<unsigned*>(ws + p.off_r); in.start_flags = start_flags;
    in.flip = erosion ? 0xFFFFFFFFu : 0u;
    in.h = erosion ? -h : h;                                                   // (v - (-h) is v + h, bit for bit)
    in.start = op == PTB_RECONSTRUCT_VALUES ? RC_START_SEED : op == PTB_RECONSTRUCT_EXTREMA ? RC_START_STEP : op == PTB_RECONSTRUCT_H_EXTREMA ? RC_START_H : RC_START_FACES;
    in.total = (unsigned)p.total; in.per_entry = (unsigned)p.per_entry; in.tiles_per_entry = (unsigned)p.tiles_per_entry;
    in.EA = p.EA; in.EB = p.EB; in.W = p.W; in.TA = p.TA; in.TB = p.TB; in.TX = p.TX; in.ntb = p.ntb; in.ntx = p.ntx; in.HB = dims == 3;
    const bool quads = p.total % 4 == 0;
    const bool mask_wide = quads && reinterpret_cast<uintptr_t>(mask) % std::min(4 * elem, 16) == 0;
    const bool wide = mask_wide && reinterpret_cast<uintptr_t>(seed) % std::min(4 * elem, 16) == 0 && reinterpret_cast<uintptr_t>(domain) % 4 == 0;
    const unsigned blocks = (unsigned)((p.total + 4 * RC_THREADS - 1) / (4 * RC_THREADS));
    with_value<PTB_F32, PTB_F16, PTB_BF16, PTB_U8, PTB_I16>(dtype, [&](auto dt) {
        with_bool(seed != nullptr, [&](auto two) {
            with_bool(wide, [&](auto wd) {
                hipLaunchKernelGGL((rc_init_kernel<dt(), two(), wd()>), dim3(blocks), dim3(RC_THREADS), 0, st, in);
            });
        });
    });

    RcRelaxArgs r{};
    r.mkey = in.mkey; r.r = in.r;
    r.per_entry = in.per_entry; r.tiles_per_entry = in.tiles_per_entry;
    r.EA = p.EA; r.EB = p.EB; r.W = p.W; r.nta = p.nta; r.ntb = p.ntb; r.ntx = p.ntx;
    const int phases = op == PTB_RECONSTRUCT_H_EXTREMA ? 2 : 1;
    for (int phase = 0; phase < phases; ++phase) {
        if (phase == 1)
            with_bool(quads, [&](auto wd) {
                hipLaunchKernelGGL((rc_restage_kernel<wd()>), dim3(blocks), dim3(RC_THREADS), 0, st, in.mkey, in.r, in.total);
            });
        r.gate = gates + phase;
        int done = 0;
        for (;;) {                                                             // (each trip launches at least one sweep: at most max_sweeps trips)
            const int n = std::min(RC_BATCH, max_sweeps - done);
            for (int k = done; k < done + n; ++k) {
                r.sweep = (unsigned)k;
                r.prev = k == 0 ? start_flags : tile_flags[(k - 1) & 1];       // (the start flags of the first phase serve the second: the same domain)
                r.cur = tile_flags[k & 1];
                with_value<2, 3>(p.dims, [&](auto dm) {
                    with_bool(full, [&](auto fl) {
                        hipLaunchKernelGGL((rc_relax_kernel<dm(), fl()>), dim3((unsigned)p.tiles), dim3(RC_THREADS), 0, st, r);
                    });
                });
            }
            done += n;
            if (int rc = check_launch()) return rc;
            unsigned last = 0;                                                 // 1 + the last sweep that changed something
            if (int rc = rc_hip(hipMemcpyAsync(&last, r.gate, sizeof(last), hipMemcpyDeviceToHost, st))) return rc;
            if (int rc = rc_hip(hipStreamSynchronize(st))) return rc;
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

    if (values)
        with_value<PTB_F32, PTB_F16, PTB_BF16, PTB_U8, PTB_I16>(dtype, [&](auto dt) {
            with_bool(mask_wide, [&](auto wd) {
                hipLaunchKernelGGL((rc_gather_kernel<dt(), wd()>), dim3(blocks), dim3(RC_THREADS), 0, st, mask, out, in.r, in.flip, top, in.total);
            });
        });
    else
        with_bool(quads, [&](auto wd) {
            hipLaunchKernelGGL((rc_compare_kernel<wd()>), dim3(blocks), dim3(RC_THREADS), 0, st, in.mkey, in.r, reinterpret_cast<unsigned char*>(out), in.total);
        });
    return check_launch();
}
