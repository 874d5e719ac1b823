// The tile-relaxation layer of the watershed (ptb_watershed.hip) and of the reconstruction (ptb_reconstruct.hip): both bring a map of
// ordered 32- or 64-bit keys to the fixed point of a monotone neighbourhood rule, tile by tile.  Here: the tile and its LDS layout, the
// geometry of a call, where a workgroup and a thread stand in it (RelaxPlace), the ordered keys and the element types they come from,
// the 32-bit relaxation of one tile (relax_tile, lowering or raising by its Rule), and on the host the plan of the shared start of the
// workspace and the sweep loop.  Device pieces are forced inline, host pieces are static: each translation unit compiles its own copy.
// A TILE.  A workgroup owns a tile (2-D: 64 x 64; 3-D: a brick 8 x 8 x 32) and holds it with a one-position halo in LDS.  A thread owns a
// run of positions along the slowest axis of the tile and relaxes them: from the neighbours in LDS, then down and up its run in registers.
// Barriers separate the reads of a trip from its writes, a workgroup-wide vote ends the trips, the tile's CAP bounds them (a tile that
// ends at the cap has changed, so it runs again).  Only the owning tile writes a position, and only the positions that changed.  Halo
// reads and the write-back are relaxed agent-scope accesses; a stale halo value is one the fixed point lies beyond as well.
// TILE ACTIVITY.  A tile runs in sweep k iff it or a tile next to it changed in sweep k - 1 (sweep 0: the init kernel's start flags); it
// writes its own flag of sweep k, zero included.  One word per phase holds 1 + the last sweep that changed anything: a sweep whose
// predecessor changed nothing returns at once, and the host reads that word back after every RELAX_BATCH launches.
// EVERY LOOP IS BOUNDED (the trips by the cap, the sweeps by max_sweeps).  No workgroup waits for another one; there are no atomic
// read-modify-writes at all.
#pragma once

#include <algorithm>

#include "ptb_common.h"

namespace ptb {

constexpr int RELAX_THREADS = 256;
constexpr int RELAX_BATCH = 8;                  // sweeps launched between two read-backs of the "changed" word

// a tile: A x B x X positions along (slowest, middle, fastest); a thread owns RUN consecutive positions along A.  2-D: A = rows, no
// middle axis (HB: its halo).  A / RUN * B * X == RELAX_THREADS.
template <int DIMS>
struct RelaxTile;
template <>
struct RelaxTile<2> {
    static constexpr int A = 64, B = 1, X = 64, RUN = 16, HB = 0, CAP = 64;
};
template <>
struct RelaxTile<3> {
    static constexpr int A = 8, B = 8, X = 32, RUN = 8, HB = 1, CAP = 32;
};
template <int DIMS>
struct RelaxLds {
    using G = RelaxTile<DIMS>;
    static constexpr int LB = G::B + 2 * G::HB, LX = G::X + 2, CELLS = (G::A + 2) * LB * LX;
    static_assert(G::A / G::RUN * G::B * G::X == RELAX_THREADS && G::A % G::RUN == 0, "a thread per run");
};

// an entry is EA x EB x W positions (2-D: EB = 1) in nta x ntb x ntx tiles of TA x TB x TX
struct RelaxGeom {
    unsigned per_entry, tiles_per_entry;
    int EA, EB, W, nta, ntb, ntx, TA, TB, TX;

    // the tile of position idx of entry e
    __device__ __forceinline__ unsigned tile_of(unsigned e, unsigned idx) const {
        const unsigned x = idx % (unsigned)W, r = idx / (unsigned)W;
        return e * tiles_per_entry + ((r / (unsigned)EB / (unsigned)TA) * (unsigned)ntb + r % (unsigned)EB / (unsigned)TB) * (unsigned)ntx + x / (unsigned)TX;
    }
};

// what every relaxation kernel gets besides its maps
struct RelaxSweep {
    const unsigned* prev;       // [tiles] the tiles' flags of the sweep before (sweep 0: the start flags)
    unsigned* cur;              // [tiles] ... of this sweep
    unsigned* gate;             // 1 + the last sweep of this phase in which a tile changed
    unsigned sweep;
    RelaxGeom g;
};

// a sweep runs iff it is the first of its phase or the sweep before it changed something (a tile of THIS sweep may have raised the word already)
__device__ __forceinline__ bool sweep_runs(const RelaxSweep& a) {
    return a.sweep == 0u || __hip_atomic_load(a.gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= a.sweep;
}

// where a workgroup's tile lies, and what a thread owns in it
template <int DIMS>
struct RelaxPlace {
    using G = RelaxTile<DIMS>;
    using L = RelaxLds<DIMS>;
    unsigned tile, first;       // this tile, and the first tile of its entry
    size_t ebase;               // the entry's first position
    int ta, tb, tx;             // tile coordinates within the entry
    int x, b, a0;               // the thread's column, middle coordinate and first position along A, within the tile

    __device__ __forceinline__ RelaxPlace(const RelaxSweep& a) {
        tile = blockIdx.x;
        const unsigned e = tile / a.g.tiles_per_entry;
        first = e * a.g.tiles_per_entry;
        unsigned t = tile - first;
        ebase = (size_t)e * a.g.per_entry;
        tx = (int)(t % (unsigned)a.g.ntx);
        t /= (unsigned)a.g.ntx;
        tb = (int)(t % (unsigned)a.g.ntb);
        ta = (int)(t / (unsigned)a.g.ntb);
        const int rest = (int)threadIdx.x / G::X;
        x = (int)threadIdx.x % G::X;
        b = rest % G::B;
        a0 = rest / G::B * G::RUN;
    }
    // is this tile, or one next to it, flagged?  (workgroup-uniform; a barrier inside)
    __device__ __forceinline__ bool active(const RelaxSweep& a) const {
        int act = 0;
        if (threadIdx.x < 27) {
            const int na = ta + (int)threadIdx.x / 9 - 1, nb = tb + (int)threadIdx.x / 3 % 3 - 1, nx = tx + (int)threadIdx.x % 3 - 1;
            if (na >= 0 && na < a.g.nta && nb >= 0 && nb < a.g.ntb && nx >= 0 && nx < a.g.ntx)
                act = a.prev[first + (unsigned)(na * a.g.ntb + nb) * (unsigned)a.g.ntx + (unsigned)nx] != 0u;
        }
        return __syncthreads_or(act) != 0;
    }
    // the position of LDS cell c within the entry, or -1 outside the entry
    __device__ __forceinline__ long long cell_position(const RelaxSweep& a, int c) const {
        const int lx = c % L::LX, rest = c / L::LX, lb = rest % L::LB, la = rest / L::LB;
        const int ga = ta * G::A + la - 1, gb = tb * G::B + lb - G::HB, gx = tx * G::X + lx - 1;
        if (ga < 0 || ga >= a.g.EA || gb < 0 || gb >= a.g.EB || gx < 0 || gx >= a.g.W) return -1;
        return ((long long)ga * a.g.EB + gb) * a.g.W + gx;
    }
    __device__ __forceinline__ int own_cell(int i) const { return ((a0 + i + 1) * L::LB + b + G::HB) * L::LX + x + 1; }
    __device__ __forceinline__ long long own_position(const RelaxSweep& a, int i) const {
        const int ga = ta * G::A + a0 + i, gb = tb * G::B + b, gx = tx * G::X + x;
        if (ga >= a.g.EA || gb >= a.g.EB || gx >= a.g.W) return -1;
        return ((long long)ga * a.g.EB + gb) * a.g.W + gx;
    }
    __device__ __forceinline__ void report(const RelaxSweep& a, bool changed) const {
        if (threadIdx.x == 0) {
            a.cur[tile] = changed ? 1u : 0u;
            if (changed) __hip_atomic_store(a.gate, a.sweep + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (every writer of a sweep stores the same value)
        }
    }
};

// ---------------------------------------------------------------------------------------------------------- keys
// monotone: a < b <=> relax_order(a, 0) < relax_order(b, 0) <=> relax_order(a, ~0) > relax_order(b, ~0); -0 as +0.  The keys of the
// non-NaN values lie in [0x007FFFFF, 0xFF800000], flipped or not.
__device__ __forceinline__ unsigned relax_order(float v, unsigned flip) {
    unsigned b = __float_as_uint(v);
    if (v == 0.0f) b = 0u;
    return ((b & 0x80000000u) ? ~b : (b | 0x80000000u)) ^ flip;
}
__device__ __forceinline__ float relax_unorder(unsigned k, unsigned flip) {
    k ^= flip;
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// element types of the value maps: every value is exact in float32, and put() gets back a value the type holds
template <int DT>
struct RelaxValue;
template <>
struct RelaxValue<PTB_F32> {
    using R = float;
    static __device__ __forceinline__ float get(R v) { return v; }
    static __device__ __forceinline__ R put(float v) { return v; }
};
template <>
struct RelaxValue<PTB_F16> {
    using R = _Float16;
    static __device__ __forceinline__ float get(R v) { return (float)v; }
    static __device__ __forceinline__ R put(float v) { return (_Float16)v; }
};
template <>
struct RelaxValue<PTB_BF16> {
    using R = unsigned short;
    static __device__ __forceinline__ float get(R v) { return __uint_as_float((unsigned)v << 16); }
    static __device__ __forceinline__ R put(float v) { return (unsigned short)(__float_as_uint(v) >> 16); }
};
template <>
struct RelaxValue<PTB_U8> {
    using R = unsigned char;
    static __device__ __forceinline__ float get(R v) { return (float)v; }
    static __device__ __forceinline__ R put(float v) { return (R)v; }
};
template <>
struct RelaxValue<PTB_I16> {
    using R = short;
    static __device__ __forceinline__ float get(R v) { return (float)v; }
    static __device__ __forceinline__ R put(float v) { return (R)v; }
};

// ---------------------------------------------------------------------------------------------------------- the 32-bit relaxation
// The direction of a rule V(p) <- better(V(p), clamp(V(q), own(p))) over the neighbours q of p: the key of a position outside the entry
// (never better than anything, so it moves nobody and is never moved), which of two keys wins, the clamp against the position's own key,
// and whether a key has improved on another.
struct RelaxLower {             // V(p) <- min(V(p), max(V(q), own(p))): the watershed's pass height
    static constexpr unsigned OUTSIDE = 0xFFFFFFFFu;
    static __device__ __forceinline__ unsigned better(unsigned a, unsigned b) { return min(a, b); }
    static __device__ __forceinline__ unsigned clamp(unsigned v, unsigned own) { return max(v, own); }
    static __device__ __forceinline__ bool improved(unsigned v, unsigned on) { return v < on; }
};
struct RelaxRaise {             // V(p) <- max(V(p), min(V(q), own(p))): reconstruction by dilation
    static constexpr unsigned OUTSIDE = 0u;
    static __device__ __forceinline__ unsigned better(unsigned a, unsigned b) { return max(a, b); }
    static __device__ __forceinline__ unsigned clamp(unsigned v, unsigned own) { return min(v, own); }
    static __device__ __forceinline__ bool improved(unsigned v, unsigned on) { return v > on; }
};

// One sweep of one tile: `value` is relaxed under `own`, both [total]; sV is the workgroup's LDS tile of RelaxLds<DIMS>::CELLS words.
// THE KERNEL THAT CALLS THIS IS LAUNCHED WITH EXACTLY RELAX_THREADS THREADS: the thread-per-run decode, the stride of the LDS fill and
// the assumption below all rest on it.
template <int DIMS, bool FULL, class Rule>
__device__ __forceinline__ void relax_tile(const RelaxSweep& a, const unsigned* own, unsigned* value, unsigned* sV) {
    using G = RelaxTile<DIMS>;
    using L = RelaxLds<DIMS>;
    // The compiler simplifies this body on its own before it inlines it into a kernel, where the launch bounds are not known yet.
    // Told here, it proves that the LDS indices do not wrap and folds the neighbours' offsets into the loads, as it did when the
    // body stood in the kernels: without it the 3-D full-connectivity instance takes 79 registers instead of 71 and loses a wave.
    const unsigned tid = threadIdx.x;
    __builtin_assume(tid < (unsigned)RELAX_THREADS);
    if (!sweep_runs(a)) return;
    const RelaxPlace<DIMS> w(a);
    if (!w.active(a)) {
        w.report(a, false);
        return;
    }
#pragma unroll 1
    for (int c = (int)threadIdx.x; c < L::CELLS; c += RELAX_THREADS) {
        const long long p = w.cell_position(a, c);
        sV[c] = p >= 0 ? __hip_atomic_load(value + w.ebase + (size_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : Rule::OUTSIDE;
    }
    unsigned m[G::RUN];
#pragma unroll
    for (int i = 0; i < G::RUN; ++i) {
        const long long p = w.own_position(a, i);
        m[i] = p >= 0 ? own[w.ebase + (size_t)p] : Rule::OUTSIDE;              // (outside the entry: never improved, never written)
    }
    __syncthreads();

    unsigned dirty = 0u;
    bool changed = false;
#pragma unroll 1
    for (int trip = 0; trip < G::CAP; ++trip) {
        unsigned cur[G::RUN], nb[G::RUN];
#pragma unroll
        for (int i = 0; i < G::RUN; ++i) nb[i] = Rule::OUTSIDE;
#pragma unroll
        for (int lv = -1; lv <= G::RUN; ++lv) {                                // level lv of the run: its own value, its neighbours in the level, what the levels next to it see
            const int base = w.own_cell(lv);
            const unsigned mid = sV[base];
            unsigned in_level = Rule::better(sV[base - 1], sV[base + 1]);
            if constexpr (DIMS == 3) {
                in_level = Rule::better(in_level, Rule::better(sV[base - L::LX], sV[base + L::LX]));
                if constexpr (FULL)
                    in_level = Rule::better(Rule::better(in_level, Rule::better(sV[base - L::LX - 1], sV[base - L::LX + 1])), Rule::better(sV[base + L::LX - 1], sV[base + L::LX + 1]));
            }
            const unsigned across = FULL ? Rule::better(mid, in_level) : mid;
            if (lv >= 0 && lv < G::RUN) {
                cur[lv] = mid;
                nb[lv] = Rule::better(nb[lv], in_level);
            }
            if (lv - 1 >= 0) nb[lv - 1] = Rule::better(nb[lv - 1], across);
            if (lv + 1 < G::RUN) nb[lv + 1] = Rule::better(nb[lv + 1], across);
        }
        unsigned v[G::RUN];
#pragma unroll
        for (int i = 0; i < G::RUN; ++i) v[i] = Rule::better(cur[i], Rule::clamp(nb[i], m[i]));
#pragma unroll
        for (int i = 1; i < G::RUN; ++i) v[i] = Rule::better(v[i], Rule::clamp(v[i - 1], m[i]));          // down the run, then up: in registers
#pragma unroll
        for (int i = G::RUN - 2; i >= 0; --i) v[i] = Rule::better(v[i], Rule::clamp(v[i + 1], m[i]));
        unsigned ch = 0u;
#pragma unroll
        for (int i = 0; i < G::RUN; ++i) ch |= Rule::improved(v[i], cur[i]) ? 1u << i : 0u;
        __syncthreads();                                                       // every read of this trip is done
#pragma unroll
        for (int i = 0; i < G::RUN; ++i)
            if (ch >> i & 1u) sV[w.own_cell(i)] = v[i];
        dirty |= ch;
        if (!__syncthreads_or(ch != 0u)) break;
        changed = true;
    }
#pragma unroll
    for (int i = 0; i < G::RUN; ++i)
        if (dirty >> i & 1u) {
            const long long p = w.own_position(a, i);                          // (a changed position lies inside the entry: outside it `own` is Rule::OUTSIDE, which clamps every change away)
            if (p >= 0) __hip_atomic_store(value + w.ebase + (size_t)p, sV[w.own_cell(i)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    w.report(a, changed);
}

// ---------------------------------------------------------------------------------------------------------- host side
// The start of every workspace: 16 bytes of sweep words (one per phase), the tiles' start flags and their two sweep flags (4 bytes
// each).  The per-position maps of a module follow from `bytes` on.
struct RelaxPlan {
    RelaxGeom g;
    int dims;
    long long B, total, tiles;
    long long off_gate, off_start, off_flags, bytes;
};

static inline int relax_plan(int dims, long long B, long long D, long long H, long long W, RelaxPlan& p) {
    if (int rc = check_shape(dims, B, D, H, W)) return rc;
    RelaxGeom& g = p.g;
    p.dims = dims; p.B = B; g.W = (int)W;
    g.EA = dims == 2 ? (int)H : (int)D; g.EB = dims == 2 ? 1 : (int)H;
    g.TA = dims == 2 ? RelaxTile<2>::A : RelaxTile<3>::A; g.TB = dims == 2 ? RelaxTile<2>::B : RelaxTile<3>::B; g.TX = dims == 2 ? RelaxTile<2>::X : RelaxTile<3>::X;
    g.nta = (g.EA + g.TA - 1) / g.TA; g.ntb = (g.EB + g.TB - 1) / g.TB; g.ntx = (g.W + g.TX - 1) / g.TX;
    g.per_entry = (unsigned)(D * H * W); p.total = B * D * H * W;
    g.tiles_per_entry = (unsigned)((long long)g.nta * g.ntb * g.ntx); p.tiles = B * g.tiles_per_entry;        // (a tile holds a position: tiles <= total)
    long long o = 0;
    p.off_gate = o; o += 16;
    p.off_start = o; o += up16(4 * p.tiles);
    p.off_flags = o; o += 2 * up16(4 * p.tiles);
    p.bytes = o;
    return PTB_OK;
}

static inline int relax_hip(hipError_t e) {
    if (e == hipSuccess) return PTB_OK;
    set_hip_error(e);
    return PTB_ELAUNCH;
}

// the flag words of a call in its workspace
struct RelaxFlags {
    unsigned* gates;            // one word per phase
    unsigned* start;            // [tiles] written by the init kernel
    unsigned* sweep[2];         // [tiles] each: the flags of the even and of the odd sweeps
};

// zeroes the sweep words and the start flags
static inline int relax_flags(char* ws, const RelaxPlan& p, hipStream_t st, RelaxFlags& f) {
    f.gates = reinterpret_cast<unsigned*>(ws + p.off_gate);
    f.start = reinterpret_cast<unsigned*>(ws + p.off_start);
    f.sweep[0] = reinterpret_cast<unsigned*>(ws + p.off_flags);
    f.sweep[1] = reinterpret_cast<unsigned*>(ws + p.off_flags + up16(4 * p.tiles));
    return relax_hip(hipMemsetAsync(ws + p.off_gate, 0, (size_t)(p.off_flags - p.off_gate), st));
}

// One phase: launch(k, prev, cur) enqueues sweep k, which reads the tile flags prev and writes cur, until a sweep changes nothing.
// `sweeps` gets the number of sweeps that ran: 1 + the last one that changed something, or max_sweeps with PTB_ENOTCONVERGED; it is
// left alone when a launch or a HIP call fails.
template <class Launch>
static inline int relax_sweeps(unsigned* gate, const RelaxFlags& f, int max_sweeps, hipStream_t st, int& sweeps, Launch&& launch) {
    int done = 0;
    for (;;) {                                                                 // (each trip launches at least one sweep: at most max_sweeps trips)
        const int n = std::min(RELAX_BATCH, max_sweeps - done);
        for (int k = done; k < done + n; ++k) launch((unsigned)k, k == 0 ? f.start : f.sweep[(k - 1) & 1], f.sweep[k & 1]);
        done += n;
        if (int rc = check_launch()) return rc;
        unsigned last = 0;                                                     // 1 + the last sweep that changed something
        if (int rc = relax_hip(hipMemcpyAsync(&last, gate, sizeof(last), hipMemcpyDeviceToHost, st))) return rc;
        if (int rc = relax_hip(hipStreamSynchronize(st))) return rc;
        if (last < (unsigned)done) {                                           // sweep `last` ran and changed nothing
            sweeps = (int)last + 1;
            return PTB_OK;
        }
        if (done >= max_sweeps) {
            sweeps = done;
            return PTB_ENOTCONVERGED;
        }
    }
}

}  // namespace ptb
