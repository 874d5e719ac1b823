// Skeletons of volumes by 3-D thinning and the centreline Dice built on them (utils/skeleton.py with dims=3; the reference has no
// counterpart).  The definition -- simple points, end points, the six direction passes of an iteration and the eight sub-field
// sub-steps of a pass -- stands in ptb_thin3d_device.h next to the one function that evaluates it.
// STATE.  Bit planes as in ptb_skeleton.hip (ptb_skeleton_device.h): 32 x-positions a word, WW = ceil(W / 32) words a row, D * H rows an
// entry, two planes A and B (launch k reads plane k & 1 and writes the other one), for clDice a third with the masks.  Pack (the shared
// body under this unit's tile rule), unpack, count and finish are the plane unit's.
// THE THINNING KERNEL.  A workgroup owns a BRICK of T3_OZ x T3_OY rows of T3_OXW words and holds it in LDS with a halo of T3_HALO
// positions in z and y and one whole word in x, next to a brick of the same shape with the candidate bits of the running pass.  One
// launch runs T3_PASSES direction passes: a mark, then eight sub-steps.  A deletion reads N26 and a mark reads distance 1, so a wrong
// value at the rim of the halo travels at most one position per mark and per sub-step: after T3_HALO = 9 * T3_PASSES of them the
// owned words are still exact; only they are written, to the other plane.
//   A THREAD OWNS WORDS.  Sub-step f touches only rows of one (z, y) parity, a quarter of the region, and of their words only the bits
//   0x55555555 or 0xAAAAAAAA: the threads walk that quarter, leave a word at once when it holds no candidate of the subfield (the
//   common case after the first iterations), and else build the nine (dz, dy) rows around it as 34-bit strips, cut the 27-bit cube of
//   every candidate bit (__ffs) out of them with shifts and ask the rule.  The update is IN PLACE: the bits another thread clears in the
//   same sub-step belong to the same subfield, which is in nobody's N26 among that sub-step's candidates, and a word is read and
//   written whole.  One workgroup-wide vote per sub-step; a pass without a candidate in the region skips its sub-steps.
// TILE ACTIVITY.  The launches take turns at the directions, so "nothing changed in the launch before" proves nothing; T3_QUIET = 6 /
// T3_PASSES launches in a row cover every direction.  The flag of a tile is a COUNT-DOWN: T3_QUIET after a launch in which an owned
// bit of it changed (and at the start, where it holds an object position), one less after every other launch, and it runs iff it or
// one of its 26 neighbours holds a flag above 0.  Sound: a tile that does not run has seen, with all its neighbours, T3_QUIET launches
// -- every direction, every subfield -- without a change in the 3 x 3 x 3 bricks, so every position of it kept its decision with its
// neighbourhood; a change can only enter from outside those bricks, travels at most T3_HALO positions a launch and has to cross a
// whole brick (T3_HALO <= the brick's extents; a partial brick has only the outside of the entry behind it), and the neighbour it
// crosses raises its flag on the way.  The call has converged when T3_QUIET launches in a row changed nothing anywhere.  INVARIANT: A
// TILE THAT DOES NOT RUN HOLDS THE SAME BITS IN BOTH PLANES -- the pack kernel writes both, a tile that changed runs in the T3_QUIET
// launches after it, and a tile that ran without a change wrote what it read.  No workgroup waits for another one; the passes of a
// launch, the trips of a flood and the launches of a call are bounded.
#include <algorithm>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_relax_device.h"
#include "ptb_skeleton_device.h"
#include "ptb_thin3d_device.h"

namespace ptb {

// the brick and the passes of a launch: measured on the blob row (profiles/skeleton3d_bench.txt); utils/skeleton.py mirrors them
#ifndef PTB_THIN3D_PASSES
#define PTB_THIN3D_PASSES 1
#endif
#ifndef PTB_THIN3D_OZ
#define PTB_THIN3D_OZ 16
#endif
#ifndef PTB_THIN3D_OY
#define PTB_THIN3D_OY 16
#endif
#ifndef PTB_THIN3D_OXW
#define PTB_THIN3D_OXW 2
#endif
constexpr int T3_PASSES = PTB_THIN3D_PASSES, T3_OZ = PTB_THIN3D_OZ, T3_OY = PTB_THIN3D_OY, T3_OXW = PTB_THIN3D_OXW;
constexpr int T3_SUBSTEPS = 8, T3_DIRECTIONS = 6;
constexpr int T3_HALO = (1 + T3_SUBSTEPS) * T3_PASSES;                        // a mark and eight sub-steps a pass, one position each
constexpr int T3_QUIET = T3_DIRECTIONS / T3_PASSES;                           // the launches that cover every direction
static_assert(T3_PASSES >= 1 && T3_DIRECTIONS % T3_PASSES == 0, "whole launches to an iteration");
static_assert(T3_HALO <= 32, "the halo in x is one word");
static_assert(T3_HALO <= T3_OZ && T3_HALO <= T3_OY && T3_HALO <= 32 * T3_OXW, "a change does not cross a brick within one launch");

struct Thin3Lds {
    static constexpr int RZ = T3_OZ + 2 * T3_HALO, RY = T3_OY + 2 * T3_HALO, RW = T3_OXW + 2, SLAB = RY * RW, CELLS = RZ * SLAB;
    static constexpr int HZ = (RZ + 1) / 2, HY = (RY + 1) / 2, QUARTER = HZ * HY * RW;      // the rows of one (z, y) parity
    static constexpr int OWNED = T3_OZ * T3_OY * T3_OXW;
    static constexpr int BYTES = 2 * 4 * CELLS;                                // the state and the candidates
};
static_assert(Thin3Lds::BYTES + 1024 <= 160 * 1024, "the two bricks fit the LDS of a CU");

// ---------------------------------------------------------------------------------------------------------- pack
struct SkTile3 {                // row = z * H + y of an entry of g.EA x g.EB rows
    __device__ __forceinline__ unsigned operator()(const SkPackArgs& a, unsigned row, unsigned w) const {
        return ((row / (unsigned)a.g.EB / (unsigned)a.g.TA) * (unsigned)a.g.ntb + row % (unsigned)a.g.EB / (unsigned)a.g.TB) * (unsigned)a.g.ntx + w / (unsigned)T3_OXW;
    }
};

template <int EB, bool WIDE>
__global__ __launch_bounds__(SK_THREADS) void sk3_pack_kernel(const SkPackArgs a) {
    sk_pack_body<EB, WIDE>(a, SkTile3{});
}

// ---------------------------------------------------------------------------------------------------------- thin
struct Sk3ThinArgs {
    const unsigned* src;        // the plane this launch reads
    unsigned* dst;              // ... and the one it writes
    unsigned* last;             // 1 + the last sub-step of the call that cleared an owned bit (atomic max)
    unsigned step0;             // the sub-steps of the launches before this one
    int dir0;                   // the direction of this launch's first pass: 0 .. 5 = z-1, z+1, y-1, y+1, x-1, x+1
    int D, H, WW;
    RelaxSweep sw;
};

// the launch runs iff one of the T3_QUIET launches before it changed something (or there are fewer of them)
__device__ __forceinline__ bool thin3d_sweep_runs(const RelaxSweep& a) {
    return __hip_atomic_load(a.gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (unsigned)T3_QUIET > a.sweep;
}

// the count-down flag of this launch: from the start flag 0 | 1 in launch 0, from the flag of the launch before otherwise
__device__ __forceinline__ void thin3d_report(const RelaxSweep& a, unsigned tile, bool changed) {
    if (threadIdx.x == 0) {
        unsigned own = a.prev[tile];
        if (a.sweep == 0u && own) own = (unsigned)T3_QUIET;
        a.cur[tile] = changed ? (unsigned)T3_QUIET : own ? own - 1u : 0u;
        if (changed) __hip_atomic_store(a.gate, a.sweep + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (every writer of a launch stores the same value)
    }
}

// the words of row `row` around word column wd as a strip: bit 0 = the last position of the word before, bits 1 .. 32 the word, bit 33
// the first position of the word after; outside the region: background
__device__ __forceinline__ unsigned long long thin3d_strip(const unsigned* S, int row, int wd, bool in) {
    using L = Thin3Lds;
    if (!in) return 0ull;
    const unsigned l = wd > 0 ? S[row + wd - 1] : 0u, m = S[row + wd], r = wd + 1 < L::RW ? S[row + wd + 1] : 0u;
    return (unsigned long long)m << 1 | (unsigned long long)(l >> 31) | (unsigned long long)(r & 1u) << 33;
}

// LAUNCHED WITH EXACTLY SK_THREADS THREADS over one workgroup per brick of sk3_plan
__global__ __launch_bounds__(SK_THREADS) void sk3_thin_kernel(const Sk3ThinArgs a) {
    using L = Thin3Lds;
    __shared__ unsigned sS[L::CELLS];                                          // the state
    __shared__ unsigned sC[L::CELLS];                                          // the candidates of the running pass
    __shared__ unsigned sLast;
    if (!thin3d_sweep_runs(a.sw)) return;
    const RelaxPlace<3> place(a.sw);                                           // (the tile's coordinates and its neighbours' flags; the thread decode is relax_tile's and unused)
    if (!place.active(a.sw)) {
        thin3d_report(a.sw, place.tile, false);
        return;
    }
    const int tid = (int)threadIdx.x;
    const size_t base = (size_t)(place.tile / a.sw.g.tiles_per_entry) * ((size_t)a.D * (size_t)a.H * (size_t)a.WW);
    const int z0 = place.ta * T3_OZ - T3_HALO, y0 = place.tb * T3_OY - T3_HALO, w0 = place.tx * T3_OXW - 1;         // the region's first row and word
#pragma unroll 1
    for (int c = tid; c < L::CELLS; c += SK_THREADS) {
        const int wd = c % L::RW, ly = c / L::RW % L::RY, lz = c / L::SLAB;
        const int gz = z0 + lz, gy = y0 + ly, gw = w0 + wd;
        const bool in = gz >= 0 && gz < a.D && gy >= 0 && gy < a.H && gw >= 0 && gw < a.WW;
        sS[c] = in ? a.src[base + ((size_t)gz * (size_t)a.H + (size_t)gy) * (size_t)a.WW + (size_t)gw] : 0u;
    }
    if (tid == 0) sLast = 0u;
    __syncthreads();

    unsigned last = 0u;
#pragma unroll 1
    for (int pass = 0; pass < T3_PASSES; ++pass) {
        const int dir = (a.dir0 + pass) % T3_DIRECTIONS;
        int some = 0;
#pragma unroll 1
        for (int c = tid; c < L::CELLS; c += SK_THREADS) {                     // the mark: object, and background next to it in the pass's direction
            const unsigned s = sS[c];
            unsigned cand = 0u;
            if (s) {
                const int wd = c % L::RW, ly = c / L::RW % L::RY, lz = c / L::SLAB;
                unsigned nb;
                switch (dir) {
                    case 0: nb = lz > 0 ? sS[c - L::SLAB] : 0u; break;
                    case 1: nb = lz + 1 < L::RZ ? sS[c + L::SLAB] : 0u; break;
                    case 2: nb = ly > 0 ? sS[c - L::RW] : 0u; break;
                    case 3: nb = ly + 1 < L::RY ? sS[c + L::RW] : 0u; break;
                    case 4: nb = s << 1 | (wd > 0 ? sS[c - 1] >> 31 : 0u); break;
                    default: nb = s >> 1 | (wd + 1 < L::RW ? sS[c + 1] << 31 : 0u); break;
                }
                cand = s & ~nb;
            }
            sC[c] = cand;
            some |= cand != 0u;
        }
        if (!__syncthreads_or(some)) continue;                                 // (also: every read of the mark before a write of sub-step 0)
#pragma unroll 1
        for (int f = 0; f < T3_SUBSTEPS; ++f) {
            const int az = ((f >> 2) ^ z0) & 1, ay = ((f >> 1) ^ y0) & 1;       // the region's rows of the subfield's parities (coordinates within the entry)
            const unsigned xmask = f & 1 ? 0xAAAAAAAAu : 0x55555555u;
            int any = 0;
#pragma unroll 1
            for (int q = tid; q < L::QUARTER; q += SK_THREADS) {
                const int wd = q % L::RW, ly = 2 * (q / L::RW % L::HY) + ay, lz = 2 * (q / (L::RW * L::HY)) + az;
                if (ly >= L::RY || lz >= L::RZ) continue;
                const int row = lz * L::SLAB + ly * L::RW;
                const unsigned centre = sS[row + wd];
                unsigned cand = sC[row + wd] & centre & xmask;
                if (!cand) continue;
                unsigned long long strip[9];
#pragma unroll
                for (int r = 0; r < 9; ++r) {
                    const int dz = r / 3 - 1, dy = r % 3 - 1;
                    strip[r] = thin3d_strip(sS, row + dz * L::SLAB + dy * L::RW, wd, lz + dz >= 0 && lz + dz < L::RZ && ly + dy >= 0 && ly + dy < L::RY);
                }
                unsigned del = 0u;
#pragma unroll 1
                while (cand) {                                                 // (the candidates of a word are two columns apart: they do not see each other)
                    const int i = __ffs((int)cand) - 1;
                    cand &= cand - 1u;
                    unsigned cube = 0u;
#pragma unroll
                    for (int r = 0; r < 9; ++r) cube |= ((unsigned)(strip[r] >> i) & 7u) << (3 * r);
                    if (thin3d_deletable(thin3d_code(cube))) del |= 1u << i;
                }
                if (del) {
                    sS[row + wd] = centre & ~del;
                    any = 1;
                    if (lz >= T3_HALO && lz < T3_HALO + T3_OZ && ly >= T3_HALO && ly < T3_HALO + T3_OY && wd >= 1 && wd <= T3_OXW)
                        last = a.step0 + (unsigned)(pass * T3_SUBSTEPS + f) + 1u;
                }
            }
            (void)any;
            __syncthreads();                                                   // every write of this sub-step before a read of the next
        }
    }
    if (last) atomicMax(&sLast, last);
    __syncthreads();
#pragma unroll 1
    for (int o = tid; o < L::OWNED; o += SK_THREADS) {
        const int wd = 1 + o % T3_OXW, ly = T3_HALO + o / T3_OXW % T3_OY, lz = T3_HALO + o / (T3_OXW * T3_OY);
        const int gz = z0 + lz, gy = y0 + ly, gw = w0 + wd;                    // (an owned row and word are >= 0)
        if (gz < a.D && gy < a.H && gw < a.WW) a.dst[base + ((size_t)gz * (size_t)a.H + (size_t)gy) * (size_t)a.WW + (size_t)gw] = sS[lz * L::SLAB + ly * L::RW + wd];
    }
    const unsigned l = sLast;
    if (tid == 0 && l) atomicMax(a.last, l);
    thin3d_report(a.sw, place.tile, l != 0u);
}

// ---------------------------------------------------------------------------------------------------------- host side
static int sk3_plan(long long planes, long long D, long long H, long long W, bool masks, SkPlan& p) {
    if (int rc = relax_plan_tiles(3, planes, D, H, W, T3_OZ, T3_OY, 32 * T3_OXW, p)) return rc;
    sk_plan_planes(planes, D * H, W, masks, p);
    return PTB_OK;
}

static void sk3_pack(const void* labels, int elem_bytes, long long B, int K, const int64_t* values, int not_equal, unsigned plane0, const SkPlan& p, char* ws,
                     const RelaxFlags& f, hipStream_t st) {
    bool wide;
    unsigned blocks;
    const SkPackArgs a = sk_pack_args(labels, elem_bytes, B, K, values, not_equal, plane0, p, (long long)p.g.EA * p.g.EB, ws, f, wide, blocks);
    with_value<1, 2, 4, 8>(elem_bytes, [&](auto eb) {
        with_bool(wide, [&](auto wd) {
            hipLaunchKernelGGL((sk3_pack_kernel<eb(), wd()>), dim3(blocks), dim3(SK_THREADS), 0, st, a);
        });
    });
}

// The launch loop of both entries, as sk_thin of ptb_skeleton.hip.  max_iterations < 0: to stability, under a guard of D + H + W
// iterations (PTB_ENOTCONVERGED beyond it, as for max_iterations >= D + H + W); otherwise at most max_iterations iterations -- whole
// launches, T3_QUIET to an iteration.  `final_plane`: the plane that holds the result; took[0]: the iterations that deleted something,
// took[1]: the launches that ran.
static int sk3_thin(const SkPlan& p, char* ws, const RelaxFlags& f, long long max_iterations, hipStream_t st, int32_t* took, int& final_plane) {
    unsigned* planes[2] = {reinterpret_cast<unsigned*>(ws + p.off_a), reinterpret_cast<unsigned*>(ws + p.off_b)};
    const long long guard = (long long)p.g.EA + p.g.EB + p.g.W;
    const bool bounded = max_iterations >= 0 && max_iterations < guard;
    const int launches = (int)std::min<long long>((bounded ? max_iterations : guard + 1) * T3_QUIET, 0x7fffffffLL);     // (unbounded: and the iteration that finds nothing left)
    final_plane = 0;
    if (took) took[0] = took[1] = 0;
    if (launches == 0) return PTB_OK;
    Sk3ThinArgs a{};
    a.last = f.gates + 1;
    a.D = p.g.EA; a.H = p.g.EB; a.WW = (int)p.WW;
    a.sw.g = p.g; a.sw.gate = f.gates;
    int ran = 0;
    int rc = relax_sweeps(f.gates, f, launches, st, ran, [&](unsigned k, const unsigned* prev, unsigned* cur) {
        a.src = planes[k & 1u]; a.dst = planes[(k + 1u) & 1u];
        a.step0 = k * (unsigned)(T3_PASSES * T3_SUBSTEPS);
        a.dir0 = (int)(k % (unsigned)T3_QUIET) * T3_PASSES;
        a.sw.sweep = k; a.sw.prev = prev; a.sw.cur = cur;
        hipLaunchKernelGGL(sk3_thin_kernel, dim3((unsigned)p.tiles), dim3(SK_THREADS), 0, st, a);
    }, T3_QUIET);
    if (rc == PTB_ENOTCONVERGED && bounded) {                                  // the cut: launch `launches - 1` wrote the result
        rc = PTB_OK;
        final_plane = launches & 1;
    }
    if (took) took[1] = ran;
    if (rc) return rc;
    unsigned last = 0;                                                         // (the loop has synchronised the stream)
    if (int e = relax_hip(hipMemcpyAsync(&last, f.gates + 1, sizeof(last), hipMemcpyDeviceToHost, st))) return e;
    if (int e = relax_hip(hipStreamSynchronize(st))) return e;
    constexpr unsigned PER_ITERATION = T3_DIRECTIONS * T3_SUBSTEPS;
    if (took) took[0] = (int32_t)((last + PER_ITERATION - 1u) / PER_ITERATION);
    return PTB_OK;
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_thin3d_rule(uint32_t code26) { return thin3d_deletable(code26) ? 1 : 0; }

extern "C" int ptb_thin3d_geometry(int32_t* out) {
    if (!out) return PTB_EINVAL;
    out[0] = T3_OZ; out[1] = T3_OY; out[2] = 32 * T3_OXW; out[3] = T3_HALO; out[4] = T3_PASSES;
    return PTB_OK;
}

extern "C" int ptb_skeleton3d_plan(int64_t B, int64_t D, int64_t H, int64_t W, int64_t* workspace_bytes) {
    SkPlan p;
    if (int rc = sk3_plan(B, D, H, W, false, p)) return rc;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return PTB_OK;
}

extern "C" int ptb_skeleton3d(const void* labels, int elem_bytes, int64_t B, int64_t D, int64_t H, int64_t W, int object_rule, int64_t value, int64_t max_iterations,
                              void* out, int32_t* took, void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (took) took[0] = took[1] = 0;
    if (!labels || !out || !workspace || bad_elem_bytes(elem_bytes)) return PTB_EINVAL;
    if (object_rule != PTB_THIN_EQUAL && object_rule != PTB_THIN_NOT_EQUAL) return PTB_EINVAL;
    SkPlan p;
    if (int rc = sk3_plan(B, D, H, W, false, p)) return rc;
    if (workspace_bytes < p.bytes || !aligned16(workspace) || !aligned16(out)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    RelaxFlags f;
    if (int rc = relax_flags(ws, p, st, f)) return rc;
    sk3_pack(labels, elem_bytes, B, 1, &value, object_rule == PTB_THIN_NOT_EQUAL, 0u, p, ws, f, st);
    int final_plane = 0;
    if (int rc = sk3_thin(p, ws, f, max_iterations, st, took, final_plane)) return rc;
    sk_unpack(reinterpret_cast<const unsigned*>(ws + (final_plane ? p.off_b : p.off_a)), out, (unsigned)(B * p.plane_words), W, p.WW, st);
    return check_launch();
}

extern "C" int ptb_centerline_dice3d_plan(int64_t B, int64_t D, int64_t H, int64_t W, int K, int64_t* workspace_bytes) {
    if (K < 1 || K > SK_MAX_CLASSES || B < 1) return PTB_EINVAL;
    if (B > MAX_POS / (2 * K)) return PTB_EUNSUPPORTED;
    SkPlan p;
    if (int rc = sk3_plan(2 * K * B, D, H, W, true, p)) return rc;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return PTB_OK;
}

extern "C" int ptb_centerline_dice3d(const void* pred, int pred_elem_bytes, const void* truth, int truth_elem_bytes, int64_t B, int64_t D, int64_t H, int64_t W,
                                     const int64_t* class_values, int K, int object_rule, int64_t* counts, float* cldice, float* tprec, float* tsens, int32_t* took,
                                     void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (took) took[0] = took[1] = 0;
    if (!pred || !truth || !class_values || !counts || !cldice || !tprec || !tsens || !workspace) return PTB_EINVAL;
    if (bad_elem_bytes(pred_elem_bytes) || bad_elem_bytes(truth_elem_bytes)) return PTB_EINVAL;
    if (object_rule != PTB_THIN_EQUAL && object_rule != PTB_THIN_NOT_EQUAL) return PTB_EINVAL;
    if (K < 1 || K > SK_MAX_CLASSES || B < 1 || (object_rule == PTB_THIN_NOT_EQUAL && K != 1)) return PTB_EINVAL;
    if (B > MAX_POS / (2 * K)) return PTB_EUNSUPPORTED;
    SkPlan p;
    if (int rc = sk3_plan(2 * K * B, D, H, W, true, p)) return rc;
    if (workspace_bytes < p.bytes || !aligned16(workspace)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    RelaxFlags f;
    if (int rc = relax_flags(ws, p, st, f)) return rc;
    const unsigned BK = (unsigned)(B * K);
    if (int rc = relax_hip(hipMemsetAsync(counts, 0, (size_t)BK * 4 * sizeof(int64_t), st))) return rc;
    const int not_equal = object_rule == PTB_THIN_NOT_EQUAL;
    sk3_pack(pred, pred_elem_bytes, B, K, class_values, not_equal, 0u, p, ws, f, st);
    sk3_pack(truth, truth_elem_bytes, B, K, class_values, not_equal, BK, p, ws, f, st);
    int final_plane = 0;
    if (int rc = sk3_thin(p, ws, f, -1, st, took, final_plane)) return rc;
    sk_count_finish(reinterpret_cast<const unsigned*>(ws + (final_plane ? p.off_b : p.off_a)), reinterpret_cast<const unsigned*>(ws + p.off_v), p.planes, p.plane_words, BK, counts,
                    cldice, tprec, tsens, st);
    return check_launch();
}
