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
//   2. rc_relax_kernel    the relaxation, tile by tile: relax_tile of ptb_relax_device.h with the raising rule.
//   3. rc_restage_kernel  between the two phases of the h-extrema: R becomes the mask, the start of the second phase is R one key step down.
//   4. rc_gather_kernel   R back as a value of the source type (outside the domain: the mask's own element),
//      rc_compare_kernel  or the bool map R < mask (the extrema).
// Tile activity, the sweep words and the bounds of every loop: ptb_relax_device.h.
#include <algorithm>
#include <cmath>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_relax_device.h"

namespace ptb {

constexpr unsigned RC_OUTSIDE = 0u;             // the key of a position outside the domain
constexpr unsigned RC_LOWEST = 0x007FFFFFu;     // the smallest key of a value: -inf (flipped: +inf)
constexpr int RC_THREADS = RELAX_THREADS;       // the pointwise kernels run the relaxation's block size

enum { RC_START_SEED = 0, RC_START_STEP = 1, RC_START_H = 2, RC_START_FACES = 3 };

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
    unsigned total;
    int HB;                     // dims == 3: the middle axis has faces
    RelaxGeom g;
};

template <int DT, bool TWO, bool WIDE>
__global__ __launch_bounds__(RC_THREADS) void rc_init_kernel(const RcInitArgs a) {
    using V = RelaxValue<DT>;
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
    unsigned e0 = p0 - p0 % a.g.per_entry;                                     // the first position of p0's entry
    unsigned mk[4], r0[4];
    bool prev_flag = false;
    unsigned prev_tile = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (p0 + j - e0 >= a.g.per_entry) e0 += a.g.per_entry;                 // (at most once per position)
        const float v = V::get(m[j]);
        const bool in = (WIDE || p0 + j < a.total) && k[j] != 0 && !(v != v);
        mk[j] = RC_OUTSIDE;
        r0[j] = RC_OUTSIDE;
        bool flag = false;
        if (in) {
            const unsigned idx = p0 + j - e0;
            const unsigned x = idx % (unsigned)a.g.W, row = idx / (unsigned)a.g.W;
            const unsigned pa = row / (unsigned)a.g.EB, pb = row % (unsigned)a.g.EB;
            mk[j] = relax_order(v, a.flip);
            unsigned st;
            if constexpr (TWO) {
                const float sv = V::get(s[j]);
                st = sv != sv ? RC_LOWEST : relax_order(sv, a.flip);           // a NaN in the seed: the lowest value (erosion: the highest)
            } else if (a.start == RC_START_STEP) {
                st = mk[j] - 1u;                                               // (mk >= RC_LOWEST > 0: no underflow)
            } else if (a.start == RC_START_H) {
                st = relax_order(v - a.h, a.flip);                             // one float32 subtraction (h finite: never a NaN)
            } else {
                const bool face = x == 0u || x + 1u == (unsigned)a.g.W || pa == 0u || pa + 1u == (unsigned)a.g.EA || (a.HB && (pb == 0u || pb + 1u == (unsigned)a.g.EB));
                st = face ? mk[j] : RC_LOWEST;
                flag = face;
            }
            r0[j] = min(st, mk[j]);                                            // the clamp: seed > mask starts at the mask
            if (a.start != RC_START_FACES) flag = true;
            if (flag) {
                const unsigned tile = a.g.tile_of(e0 / a.g.per_entry, idx);
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
    RelaxSweep sw;
};

template <int DIMS, bool FULL>
__global__ __launch_bounds__(RELAX_THREADS) void rc_relax_kernel(const RcRelaxArgs a) {
    __shared__ unsigned sR[RelaxLds<DIMS>::CELLS];
    static_assert(sizeof(sR) <= 32 * 1024, "at least four workgroups per CU by LDS");
    relax_tile<DIMS, FULL, RelaxRaise>(a.sw, a.mkey, a.r, sR);
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

// R as values of the source type, capped at `top` (the one infinity no input held: the start of a position that no face reaches in
// hole filling), so that put() gets a value the type holds; outside the domain the mask's own element.  out may be the mask itself
// (a thread reads its four positions before it writes them) but must not overlap it otherwise.
template <int DT, bool WIDE>
__global__ __launch_bounds__(RC_THREADS) void rc_gather_kernel(const void* mask_, void* out_, const unsigned* r, unsigned flip, float top, unsigned total) {
    using V = RelaxValue<DT>;
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
    for (int j = 0; j < 4; ++j) o[j] = k[j] == RC_OUTSIDE ? m[j] : V::put(fminf(relax_unorder(k[j], flip), top));
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
// The workspace: the sweep words and tile flags (RelaxPlan), then per position the mask key (4) and R (4).
struct RcPlan : RelaxPlan {
    long long off_mkey, off_r;
};

static int rc_plan(int dims, long long B, long long D, long long H, long long W, int op, RcPlan& p) {
    if (op < PTB_RECONSTRUCT_VALUES || op > PTB_RECONSTRUCT_FILL) return PTB_EINVAL;
    if (int rc = relax_plan(dims, B, D, H, W, p)) return rc;
    p.off_mkey = p.bytes; p.bytes += up16(4 * p.total);
    p.off_r = p.bytes; p.bytes += up16(4 * p.total);
    return PTB_OK;
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
    RelaxFlags f;
    if (int rc = relax_flags(ws, p, st, f)) return rc;
    RcInitArgs in{};
    in.seed = seed; in.mask = mask; in.domain = reinterpret_cast<const unsigned char*>(domain);
    in.mkey = reinterpret_cast<unsigned*>(ws + p.off_mkey); in.r = reinterpret_cast<unsigned*>(ws + p.off_r); in.start_flags = f.start;
    in.flip = erosion ? 0xFFFFFFFFu : 0u;
    in.h = erosion ? -h : h;                                                   // (v - (-h) is v + h, bit for bit)
    in.start = op == PTB_RECONSTRUCT_VALUES ? RC_START_SEED : op == PTB_RECONSTRUCT_EXTREMA ? RC_START_STEP : op == PTB_RECONSTRUCT_H_EXTREMA ? RC_START_H : RC_START_FACES;
    in.total = (unsigned)p.total; in.HB = dims == 3; in.g = p.g;
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
    r.sw.g = p.g;
    const int phases = op == PTB_RECONSTRUCT_H_EXTREMA ? 2 : 1;
    for (int phase = 0; phase < phases; ++phase) {
        if (phase == 1)
            with_bool(quads, [&](auto wd) {
                hipLaunchKernelGGL((rc_restage_kernel<wd()>), dim3(blocks), dim3(RC_THREADS), 0, st, in.mkey, in.r, in.total);
            });
        r.sw.gate = f.gates + phase;
        int sweeps = -1;                                                       // (the start flags of the first phase serve the second: the same domain)
        const int rc = relax_sweeps(r.sw.gate, f, max_sweeps, st, sweeps, [&](unsigned k, const unsigned* prev, unsigned* cur) {
            r.sw.sweep = k; r.sw.prev = prev; r.sw.cur = cur;
            with_value<2, 3>(p.dims, [&](auto dm) {
                with_bool(full, [&](auto fl) {
                    hipLaunchKernelGGL((rc_relax_kernel<dm(), fl()>), dim3((unsigned)p.tiles), dim3(RELAX_THREADS), 0, st, r);
                });
            });
        });
        if (sweeps_out) sweeps_out[phase] = sweeps;
        if (rc) return rc;
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
