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
//   2. ws_cost_kernel,   the two relaxations, tile by tile as ptb_relax_device.h describes.  The cost kernel is that header's relax_tile with the
//   3. ws_path_kernel    lowering rule.  The path kernel holds the 64-bit keys and the final costs of its tile in LDS and has a body of its
//                        own: a step q -> p is taken only where it is admissible, C(q) <= C(p).
//   4. ws_gather_kernel  labels[p] = markers[entry + sigma(p)] or the background, and the optional cost (float32) and seed (int32) maps.
// Tile activity, the sweep words and the bounds of every loop: ptb_relax_device.h.
#include <algorithm>
#include <cmath>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_relax_device.h"

namespace ptb {

using u64 = unsigned long long;

constexpr unsigned WS_NONE = 0xFFFFFFFFu;       // the cost key of "outside M" / "not reached"
constexpr u64 WS_NONE64 = ~0ull;                // the path key of the same
constexpr u64 WS_STEP = 1ull << 32;
constexpr int WS_THREADS = RELAX_THREADS;       // the pointwise kernels run the relaxations' block size

__device__ __forceinline__ float ws_unorder(unsigned k) { return k == WS_NONE ? INFINITY : relax_unorder(k, 0u); }

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
    unsigned total;
    int all_seeds;
    RelaxGeom g;
};

template <int HT, class T, bool WIDE>
__global__ __launch_bounds__(WS_THREADS) void ws_init_kernel(const WsInitArgs a) {
    using R = typename RelaxValue<HT>::R;
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
    unsigned e0 = p0 - p0 % a.g.per_entry;                                     // the first position of p0's entry
    unsigned hk[4], c[4];
    u64 key[4];
    bool prev_seed = false;
    unsigned prev_tile = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (p0 + j - e0 >= a.g.per_entry) e0 += a.g.per_entry;                 // (at most once per position)
        const float v = RelaxValue<HT>::get(h[j]);
        const bool in_m = (WIDE || p0 + j < a.total) && k[j] != 0 && !(v != v) && v != INFINITY;
        const bool seed = in_m && (a.all_seeds || m[j] != bg);
        const unsigned idx = p0 + j - e0;
        hk[j] = in_m ? relax_order(v, 0u) : WS_NONE;
        c[j] = seed ? hk[j] : WS_NONE;
        key[j] = seed ? (u64)idx : WS_NONE64;
        if (seed) {
            const unsigned tile = a.g.tile_of(e0 / a.g.per_entry, idx);
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
    RelaxSweep sw;
};

template <int DIMS, bool FULL>
__global__ __launch_bounds__(RELAX_THREADS) void ws_cost_kernel(const WsRelaxArgs a) {
    __shared__ unsigned sC[RelaxLds<DIMS>::CELLS];
    static_assert(sizeof(sC) <= 32 * 1024, "at least four workgroups per CU by LDS");
    relax_tile<DIMS, FULL, RelaxLower>(a.sw, a.hkey, a.cost, sC);
}

template <int DIMS, bool FULL>
__global__ __launch_bounds__(RELAX_THREADS) void ws_path_kernel(const WsRelaxArgs a) {
    using G = RelaxTile<DIMS>;
    using L = RelaxLds<DIMS>;
    __shared__ u64 sK[L::CELLS];
    __shared__ unsigned sC[L::CELLS];
    static_assert(sizeof(sK) + sizeof(sC) <= 64 * 1024, "a 64-bit and a 32-bit map of the tile");
    const RelaxSweep& sw = a.sw;
    if (!sweep_runs(sw)) return;
    const RelaxPlace<DIMS> w(sw);
    if (!w.active(sw)) {
        w.report(sw, false);
        return;
    }
#pragma unroll 1
    for (int c = (int)threadIdx.x; c < L::CELLS; c += RELAX_THREADS) {
        const long long p = w.cell_position(sw, c);
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
            const long long p = w.own_position(sw, i);
            if (p >= 0) __hip_atomic_store(a.key + w.ebase + (size_t)p, sK[w.own_cell(i)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    w.report(sw, changed);
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
// The workspace: the sweep words and tile flags (RelaxPlan), then per position the height key (4), the cost key (4) and the path key (8).
struct WsPlan : RelaxPlan {
    long long off_hkey, off_cost, off_key;
};

static int ws_plan(int dims, long long B, long long D, long long H, long long W, int flags, WsPlan& p) {
    if (flags & ~(PTB_WATERSHED_COST | PTB_WATERSHED_SEED)) return PTB_EINVAL;
    if (int rc = relax_plan(dims, B, D, H, W, p)) return rc;
    p.off_hkey = p.bytes; p.bytes += up16(4 * p.total);
    p.off_cost = p.bytes; p.bytes += up16(4 * p.total);
    p.off_key = p.bytes; p.bytes += up16(8 * p.total);
    return PTB_OK;
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
    if (bad_elem_bytes(marker_bytes)) return PTB_EINVAL;
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
    RelaxFlags f;
    if (int rc = relax_flags(ws, p, st, f)) return rc;
    WsInitArgs in{};
    in.height = height; in.markers = markers; in.mask = reinterpret_cast<const unsigned char*>(mask);
    in.hkey = reinterpret_cast<unsigned*>(ws + p.off_hkey); in.cost = reinterpret_cast<unsigned*>(ws + p.off_cost); in.key = reinterpret_cast<u64*>(ws + p.off_key);
    in.seed_flags = f.start; in.background = background;
    in.total = (unsigned)p.total; in.g = p.g;
    in.all_seeds = !holds(marker_bytes, background);                           // a background the element type cannot hold occurs nowhere
    const bool markers_wide = p.total % 4 == 0 && reinterpret_cast<uintptr_t>(markers) % std::min(4 * marker_bytes, 16) == 0;
    const bool wide = markers_wide && reinterpret_cast<uintptr_t>(height) % std::min(4 * height_bytes, 16) == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0;
    const unsigned blocks = (unsigned)((p.total + 4 * WS_THREADS - 1) / (4 * WS_THREADS));
    with_value<PTB_F32, PTB_F16, PTB_BF16, PTB_U8, PTB_I16>(height_dtype, [&](auto ht) {
        with_value<1, 2, 4, 8>(marker_bytes, [&](auto eb) {
            using T = label_t<eb()>;
            with_bool(wide, [&](auto wd) {
                hipLaunchKernelGGL((ws_init_kernel<ht(), T, wd()>), dim3(blocks), dim3(WS_THREADS), 0, st, in);
            });
        });
    });

    WsRelaxArgs r{};
    r.hkey = in.hkey; r.cost = in.cost; r.key = in.key;
    r.sw.g = p.g;
    for (int phase = 0; phase < 2; ++phase) {
        r.sw.gate = f.gates + phase;
        int sweeps = -1;
        const int rc = relax_sweeps(r.sw.gate, f, max_sweeps, st, sweeps, [&](unsigned k, const unsigned* prev, unsigned* cur) {
            r.sw.sweep = k; r.sw.prev = prev; r.sw.cur = cur;
            with_value<2, 3>(p.dims, [&](auto dm) {
                with_bool(full, [&](auto fl) {
                    if (phase == 0) hipLaunchKernelGGL((ws_cost_kernel<dm(), fl()>), dim3((unsigned)p.tiles), dim3(RELAX_THREADS), 0, st, r);
                    else hipLaunchKernelGGL((ws_path_kernel<dm(), fl()>), dim3((unsigned)p.tiles), dim3(RELAX_THREADS), 0, st, r);
                });
            });
        });
        if (sweeps_out) sweeps_out[phase] = sweeps;
        if (rc) return rc;
    }

    WsGatherArgs g{};
    g.markers = markers; g.out = labels_out; g.key = in.key; g.cost = in.cost; g.cost_out = cost_out; g.seed_out = seed_out; g.fill = fill;
    g.total = in.total; g.per_entry = p.g.per_entry;
    with_value<1, 2, 4, 8>(marker_bytes, [&](auto eb) {
        using T = label_t<eb()>;
        with_bool(markers_wide, [&](auto wd) {
            hipLaunchKernelGGL((ws_gather_kernel<T, wd()>), dim3(blocks), dim3(WS_THREADS), 0, st, g);
        });
    });
    return check_launch();
}
