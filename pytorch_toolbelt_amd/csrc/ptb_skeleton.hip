// Skeletons by parallel thinning and the centreline Dice built on them (utils/skeleton.py; the reference has no counterpart).  The
// definitions -- the neighbours P2 .. P9, the two sub-iterations of an iteration, the deletion rules of Zhang & Suen and of Guo & Hall --
// stand in ptb_thin_device.h next to the one function that evaluates them on words.  The skeleton is the state after the first
// iteration that deletes nothing (or after max_iterations of them); the iteration count is the number of iterations that deleted
// something.
// STATE.  The object of every entry is a BIT PLANE: 32 positions a word, WW = ceil(W / 32) words a row; bits at columns >= W are 0 and
// stay 0, because thinning only clears bits.  Two planes, A and B: launch k reads plane k & 1 and writes the other one, so every tile
// reads the pre-launch state of its neighbours.  ptb_centerline_dice keeps a third plane, the untouched masks.  The flag words of
// ptb_relax_device.h follow; there is no other per-position map.
//   1. sk_pack_kernel     the label map under the class / background rule into bit planes (BOTH of them, and the mask plane), and a
//                         start flag for every tile that holds an object position.
//   2. sk_thin_kernel     a workgroup owns a 64 x 64 tile (RelaxTile<2>): 64 rows of 2 words.  It holds them in LDS with a halo of
//                         THIN_STEPS rows above and below and one whole word (32 columns) left and right, and runs up to THIN_STEPS
//                         sub-iterations there between two LDS buffers.  A wrong value at the rim of the halo travels one position a
//                         step, so after THIN_STEPS <= 32 steps the owned words are still exact; only they are written, to the other
//                         plane.  The tile reports whether one of them changed.
//   3. sk_unpack_kernel   the final plane as bytes.
//   4. sk_count_kernel, sk_finish_kernel   (clDice) the four popcounts of every (entry, class), folded per wave and added with 64-bit
//                         integer atomics -- integer sums: exact, the same on every run --, then the ratios in float64.
// TILE ACTIVITY.  A tile runs in launch k iff it or one of its 8 neighbours changed in launch k - 1 (launch 0: the start flags).  Sound:
// such a launch ran both kinds of sub-iteration (THIN_STEPS is even) without a change in the 3 x 3 tiles, so every position there whose
// neighbourhood lies in them keeps its decision until its neighbourhood changes; a change can only enter from outside the 3 x 3 tiles and
// travels one position a step, so it needs 64 > THIN_STEPS steps to reach the tile in the middle.  INVARIANT: A TILE THAT DOES NOT RUN
// HOLDS THE SAME BITS IN BOTH PLANES -- the pack kernel writes both, a tile that ran and changed runs again, and a tile that ran
// without a change wrote what it read.  After convergence the planes are equal; after a cut by max_iterations launch L - 1 wrote plane
// L & 1.  No workgroup waits for another one; the steps of a launch and the launches of a call are bounded.
#include <algorithm>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_relax_device.h"
#include "ptb_thin_device.h"

namespace ptb {

#ifndef PTB_THIN_STEPS
#define PTB_THIN_STEPS 32       // measured against 8 and 16 on the blob row (profiles/skeleton_bench.txt); utils/skeleton.py mirrors it
#endif
constexpr int THIN_STEPS = PTB_THIN_STEPS;
static_assert(THIN_STEPS % 2 == 0 && THIN_STEPS >= 2 && THIN_STEPS <= 32, "both kinds of sub-iteration in every launch; the halo is one word wide");
constexpr int SK_THREADS = RELAX_THREADS;
constexpr int SK_MAX_CLASSES = 32;

struct ThinLds {
    static constexpr int ROWS = RelaxTile<2>::A + 2 * THIN_STEPS, WORDS = RelaxTile<2>::X / 32 + 2, CELLS = ROWS * WORDS;
    static constexpr int PER_THREAD = (CELLS + SK_THREADS - 1) / SK_THREADS;
    static_assert(WORDS == 4, "a cell's word column is its index & 3");
};

// ---------------------------------------------------------------------------------------------------------- pack
struct SkPackArgs {
    const void* labels;         // [B, H, W]
    unsigned* a;                // the two thinning planes and (or NULL) the mask plane: [planes, H, WW] each
    unsigned* b;
    unsigned* v;
    unsigned* start_flags;      // [planes * tiles_per_entry] zeroed by the caller
    long long values[SK_MAX_CLASSES];
    unsigned held;              // bit k: the element type holds values[k] (else it occurs nowhere)
    int K, not_equal;           // the object of class k: labels == values[k], or (K == 1) labels != values[0]
    unsigned plane0;            // plane of (entry b, class k) = plane0 + b * K + k
    unsigned words;             // B * H * WW
    int H, W, WW;
    RelaxGeom g;
};

template <int EB, bool WIDE>
__global__ __launch_bounds__(SK_THREADS) void sk_pack_kernel(const SkPackArgs a) {
    using T = label_t<EB>;
    const unsigned idx = blockIdx.x * (unsigned)SK_THREADS + threadIdx.x;
    if (idx >= a.words) return;
    const unsigned w = idx % (unsigned)a.WW, row = idx / (unsigned)a.WW, y = row % (unsigned)a.H, e = row / (unsigned)a.H;
    const int x0 = (int)w * 32;
    const T* src = reinterpret_cast<const T*>(a.labels) + (size_t)row * (size_t)a.W + (size_t)x0;
    T el[32];
    if constexpr (WIDE) {                                                      // the base and every row are 16-byte aligned, W is whole chunks
        constexpr int CH = 16 / EB;
#pragma unroll
        for (int c = 0; c < 32 / CH; ++c) {
#pragma unroll
            for (int j = 0; j < CH; ++j) el[c * CH + j] = (T)0;
            if (x0 + c * CH < a.W) __builtin_memcpy(&el[c * CH], __builtin_assume_aligned(src + c * CH, 16), 16);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 32; ++j) el[j] = x0 + j < a.W ? src[j] : (T)0;
    }
    const int n = min(32, a.W - x0);
    const unsigned valid = n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u;             // bits at columns >= W are 0
    const unsigned tile = ((y / (unsigned)a.g.TA) * (unsigned)a.g.ntx + w / 2u);
    for (int k = 0; k < a.K; ++k) {
        const T val = (T)a.values[k];
        unsigned m = 0u;
#pragma unroll
        for (int j = 0; j < 32; ++j) m |= (el[j] == val ? 1u : 0u) << j;
        if (!(a.held >> k & 1u)) m = 0u;
        if (a.not_equal) m = ~m;
        m &= valid;
        const unsigned plane = a.plane0 + e * (unsigned)a.K + (unsigned)k;
        const size_t at = (size_t)plane * ((size_t)a.H * (size_t)a.WW) + (size_t)y * (size_t)a.WW + w;
        a.a[at] = m;
        a.b[at] = m;
        if (a.v) a.v[at] = m;
        if (m) a.start_flags[plane * a.g.tiles_per_entry + tile] = 1u;          // (every writer stores the same value)
    }
}

// ---------------------------------------------------------------------------------------------------------- thin
struct SkThinArgs {
    const unsigned* src;        // the plane this launch reads
    unsigned* dst;              // ... and the one it writes
    unsigned* last;             // 1 + the last sub-iteration of the call that cleared an owned bit (atomic max)
    unsigned step0;             // the sub-iterations done before this launch (even)
    int steps;                  // the sub-iterations this launch may run: 1 .. THIN_STEPS
    int H, WW;
    RelaxSweep sw;
};

// LAUNCHED WITH EXACTLY SK_THREADS THREADS over one workgroup per tile of relax_plan(2, planes, 1, H, W)
template <int METHOD>
__global__ __launch_bounds__(SK_THREADS) void sk_thin_kernel(const SkThinArgs a) {
    using G = RelaxTile<2>;
    using L = ThinLds;
    __shared__ unsigned sT[2][L::CELLS];
    __shared__ unsigned sLast;
    if (!sweep_runs(a.sw)) return;
    const RelaxPlace<2> place(a.sw);
    if (!place.active(a.sw)) {
        place.report(a.sw, false);
        return;
    }
    const int tid = (int)threadIdx.x;
    const int wd = tid & 3;                                                    // (SK_THREADS % 4 == 0: a thread keeps its word column)
    const size_t base = (size_t)(place.tile / a.sw.g.tiles_per_entry) * ((size_t)a.H * (size_t)a.WW);
    const int gw = place.tx * 2 - 1 + wd;
    const bool col_in = gw >= 0 && gw < a.WW;
    int gy[L::PER_THREAD];
#pragma unroll
    for (int j = 0; j < L::PER_THREAD; ++j) {
        const int c = tid + j * SK_THREADS;
        gy[j] = place.ta * G::A - THIN_STEPS + (c >> 2);
        if (c < L::CELLS) sT[0][c] = col_in && gy[j] >= 0 && gy[j] < a.H ? a.src[base + (size_t)gy[j] * (size_t)a.WW + (size_t)gw] : 0u;
    }
    if (tid == 0) sLast = 0u;
    __syncthreads();

    int cur = 0, quiet = 0;
    unsigned last = 0u;
#pragma unroll 1
    for (int s = 0; s < a.steps; ++s) {
        const unsigned* T = sT[cur];
        unsigned* O = sT[cur ^ 1];
        int any = 0;
#pragma unroll
        for (int j = 0; j < L::PER_THREAD; ++j) {
            const int c = tid + j * SK_THREADS;
            if (c >= L::CELLS) continue;
            const int r = c >> 2;
            const unsigned ctr = T[c];
            unsigned now = ctr;
            if (ctr) {                                                         // outside the LDS region: background
                const bool up = r > 0, dn = r + 1 < L::ROWS, lf = wd > 0, rt = wd < 3;
                uint32_t nbr[8];
                thin_neighbours(up && lf ? T[c - 5] : 0u, up ? T[c - 4] : 0u, up && rt ? T[c - 3] : 0u, lf ? T[c - 1] : 0u, ctr, rt ? T[c + 1] : 0u,
                                dn && lf ? T[c + 3] : 0u, dn ? T[c + 4] : 0u, dn && rt ? T[c + 5] : 0u, nbr);
                const unsigned del = thin_rule<METHOD>(s & 1, nbr, ctr);
                if (del) {
                    now = ctr & ~del;
                    any = 1;
                    if (r >= THIN_STEPS && r < THIN_STEPS + G::A && (wd == 1 || wd == 2)) last = a.step0 + (unsigned)s + 1u;
                }
            }
            O[c] = now;
        }
        cur ^= 1;
        if (__syncthreads_or(any)) quiet = 0;                                  // (also: every write of this step before a read of the next)
        else if (++quiet == 2) break;                                          // both kinds of sub-iteration left the region alone: a fixed point
    }
    if (last) atomicMax(&sLast, last);
#pragma unroll
    for (int j = 0; j < L::PER_THREAD; ++j) {
        const int c = tid + j * SK_THREADS, r = c >> 2;
        if (c < L::CELLS && r >= THIN_STEPS && r < THIN_STEPS + G::A && (wd == 1 || wd == 2) && col_in && gy[j] < a.H)
            a.dst[base + (size_t)gy[j] * (size_t)a.WW + (size_t)gw] = sT[cur][c];     // (an owned row is >= 0)
    }
    __syncthreads();
    const unsigned l = sLast;
    if (tid == 0 && l) atomicMax(a.last, l);
    place.report(a.sw, l != 0u);
}

// ---------------------------------------------------------------------------------------------------------- unpack
template <bool WIDE>
__global__ __launch_bounds__(SK_THREADS) void sk_unpack_kernel(const unsigned* plane, unsigned char* out, unsigned words, int W, int WW) {
    const unsigned idx = blockIdx.x * (unsigned)SK_THREADS + threadIdx.x;
    if (idx >= words) return;
    const unsigned w = idx % (unsigned)WW, row = idx / (unsigned)WW;
    const int x0 = (int)w * 32;
    const unsigned m = plane[idx];
    unsigned char* dst = out + (size_t)row * (size_t)W + (size_t)x0;
    if constexpr (WIDE) {                                                      // out is 16-byte aligned and W % 16 == 0
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (x0 + c * 16 < W) {
                unsigned char o[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) o[j] = (unsigned char)(m >> (c * 16 + j) & 1u);
                __builtin_memcpy(__builtin_assume_aligned(dst + c * 16, 16), o, 16);
            }
    } else {
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (x0 + j < W) dst[j] = (unsigned char)(m >> j & 1u);
    }
}

// ---------------------------------------------------------------------------------------------------------- clDice
// counts [B][K][4] (zeroed by the caller): |S_P & V_T|, |S_P|, |S_T & V_P|, |S_T|.  Plane (side, b, k) = (side * B + b) * K + k.
// `blocks` workgroups per plane, 2 * B * K planes
__global__ __launch_bounds__(SK_THREADS) void sk_count_kernel(const unsigned* skel, const unsigned* mask, unsigned long long* counts, unsigned plane_words, unsigned BK,
                                                              unsigned blocks) {
    const unsigned p = blockIdx.x / blocks, first = blockIdx.x % blocks, side = p >= BK ? 1u : 0u, obj = p - side * BK, q = (1u - side) * BK + obj;
    const unsigned* S = skel + (size_t)p * plane_words;
    const unsigned* V = mask + (size_t)q * plane_words;
    unsigned both = 0u, own = 0u;                                              // (a plane holds fewer than 2^31 positions)
    for (unsigned i = first * (unsigned)SK_THREADS + threadIdx.x; i < plane_words; i += blocks * (unsigned)SK_THREADS) {
        const unsigned s = S[i];
        own += (unsigned)__popc(s);
        both += (unsigned)__popc(s & V[i]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        own += (unsigned)__shfl_xor((int)own, d);
        both += (unsigned)__shfl_xor((int)both, d);
    }
    if ((threadIdx.x & 63u) == 0u && own) {                                    // (both <= own)
        atomicAdd(counts + (size_t)obj * 4u + side * 2u + 1u, (unsigned long long)own);
        if (both) atomicAdd(counts + (size_t)obj * 4u + side * 2u, (unsigned long long)both);
    }
}

// one workgroup: the ratios of every (entry, class) in float64, rounded once to float32
__global__ __launch_bounds__(SK_THREADS) void sk_finish_kernel(const unsigned long long* counts, float* cldice, float* tprec, float* tsens, unsigned BK) {
    for (unsigned o = threadIdx.x; o < BK; o += (unsigned)SK_THREADS) {
        const unsigned long long* c = counts + (size_t)o * 4u;
        const double nan = __builtin_nan("");
        const double p = c[1] ? (double)c[0] / (double)c[1] : nan, s = c[3] ? (double)c[2] / (double)c[3] : nan;
        double d;
        if (!c[1] && !c[3]) d = nan;
        else if (!c[1] || !c[3] || p + s == 0.0) d = 0.0;
        else d = 2.0 * p * s / (p + s);
        cldice[o] = (float)d;
        tprec[o] = (float)p;
        tsens[o] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
// The workspace: the sweep words and tile flags (RelaxPlan), then the planes A and B and, for clDice, the masks: 4 H WW bytes per plane.
struct SkPlan : RelaxPlan {
    long long planes, WW, plane_words, off_a, off_b, off_v;
};

static int sk_plan(long long planes, long long H, long long W, bool masks, SkPlan& p) {
    if (int rc = relax_plan(2, planes, 1, H, W, p)) return rc;
    p.planes = planes; p.WW = (W + 31) / 32; p.plane_words = H * p.WW;
    const long long bytes = up16(4 * planes * p.plane_words);
    p.off_a = p.bytes; p.bytes += bytes;
    p.off_b = p.bytes; p.bytes += bytes;
    p.off_v = masks ? p.bytes : -1;
    if (masks) p.bytes += bytes;
    return PTB_OK;
}

static void sk_pack(const void* labels, int elem_bytes, long long B, int K, const int64_t* values, int not_equal, unsigned plane0, const SkPlan& p,
                    char* ws, const RelaxFlags& f, hipStream_t st) {
    SkPackArgs a{};
    a.labels = labels;
    a.a = reinterpret_cast<unsigned*>(ws + p.off_a); a.b = reinterpret_cast<unsigned*>(ws + p.off_b);
    a.v = p.off_v >= 0 ? reinterpret_cast<unsigned*>(ws + p.off_v) : nullptr;
    a.start_flags = f.start;
    for (int k = 0; k < K; ++k) {
        a.values[k] = values[k];
        if (holds(elem_bytes, values[k])) a.held |= 1u << k;
    }
    a.K = K; a.not_equal = not_equal; a.plane0 = plane0;
    a.words = (unsigned)(B * p.plane_words);
    a.H = p.g.EA; a.W = p.g.W; a.WW = (int)p.WW; a.g = p.g;
    const bool wide = aligned16(labels) && ((long long)a.W * elem_bytes) % 16 == 0;
    const unsigned blocks = (a.words + SK_THREADS - 1) / SK_THREADS;
    with_value<1, 2, 4, 8>(elem_bytes, [&](auto eb) {
        with_bool(wide, [&](auto wd) {
            hipLaunchKernelGGL((sk_pack_kernel<eb(), wd()>), dim3(blocks), dim3(SK_THREADS), 0, st, a);
        });
    });
}

// The launch loop of both entries.  max_iterations < 0: to stability, under a guard of H + W iterations (PTB_ENOTCONVERGED beyond it,
// as for max_iterations >= H + W); otherwise at most max_iterations iterations.  `final_plane`: the plane that holds the result;
// took[0]: the iterations that deleted something, took[1]: the launches that ran.
static int sk_thin(const SkPlan& p, char* ws, const RelaxFlags& f, int method, long long max_iterations, hipStream_t st, int32_t* took, int& final_plane) {
    unsigned* planes[2] = {reinterpret_cast<unsigned*>(ws + p.off_a), reinterpret_cast<unsigned*>(ws + p.off_b)};
    const long long guard = (long long)p.g.EA + p.g.W;
    const bool bounded = max_iterations >= 0 && max_iterations < guard;
    const long long total = 2 * (bounded ? max_iterations : guard);           // sub-iterations the launches may run
    const int launches = (int)((total + THIN_STEPS - 1) / THIN_STEPS) + (bounded ? 0 : 1);        // (unbounded: and the one that finds nothing left)
    final_plane = 0;
    if (took) took[0] = took[1] = 0;
    if (launches == 0) return PTB_OK;
    SkThinArgs a{};
    a.last = f.gates + 1;
    a.H = p.g.EA; a.WW = (int)p.WW;
    a.sw.g = p.g; a.sw.gate = f.gates;
    int ran = 0;
    int rc = relax_sweeps(f.gates, f, launches, st, ran, [&](unsigned k, const unsigned* prev, unsigned* cur) {
        a.src = planes[k & 1u]; a.dst = planes[(k + 1u) & 1u];
        a.step0 = k * (unsigned)THIN_STEPS;
        a.steps = bounded ? (int)std::min<long long>(THIN_STEPS, total - (long long)k * THIN_STEPS) : THIN_STEPS;
        a.sw.sweep = k; a.sw.prev = prev; a.sw.cur = cur;
        with_value<THIN_ZHANG, THIN_GUO_HALL>(method, [&](auto me) {
            hipLaunchKernelGGL((sk_thin_kernel<me()>), dim3((unsigned)p.tiles), dim3(SK_THREADS), 0, st, a);
        });
    });
    if (rc == PTB_ENOTCONVERGED && bounded) {                                  // the cut: launch `launches - 1` wrote the result
        rc = PTB_OK;
        final_plane = launches & 1;
    }
    if (took) took[1] = ran;
    if (rc) return rc;
    unsigned last = 0;                                                         // (the loop has synchronised the stream)
    if (int e = relax_hip(hipMemcpyAsync(&last, f.gates + 1, sizeof(last), hipMemcpyDeviceToHost, st))) return e;
    if (int e = relax_hip(hipStreamSynchronize(st))) return e;
    if (took) took[0] = (int32_t)((last + 1u) / 2u);
    return PTB_OK;
}

static bool sk_bad_method(int method) { return method != PTB_THIN_ZHANG && method != PTB_THIN_GUO_HALL; }

}  // namespace ptb

using namespace ptb;

static_assert(PTB_THIN_ZHANG == THIN_ZHANG && PTB_THIN_GUO_HALL == THIN_GUO_HALL, "the header's codes are the rule's");

extern "C" uint32_t ptb_thin_rule(int method, int sub, const uint32_t* nbr, uint32_t centre) {
    if (sk_bad_method(method) || (sub != 0 && sub != 1) || !nbr) return 0u;
    const uint32_t n[8] = {nbr[0], nbr[1], nbr[2], nbr[3], nbr[4], nbr[5], nbr[6], nbr[7]};
    return method == PTB_THIN_ZHANG ? thin_rule<THIN_ZHANG>(sub, n, centre) : thin_rule<THIN_GUO_HALL>(sub, n, centre);
}

extern "C" int ptb_thin_steps(void) { return THIN_STEPS; }

extern "C" int ptb_skeleton_plan(int64_t B, int64_t H, int64_t W, int64_t* workspace_bytes) {
    SkPlan p;
    if (int rc = sk_plan(B, H, W, false, p)) return rc;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return PTB_OK;
}

extern "C" int ptb_skeleton(const void* labels, int elem_bytes, int64_t B, int64_t H, int64_t W, int object_rule, int64_t value, int method,
                            int64_t max_iterations, void* out, int32_t* took, void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (took) took[0] = took[1] = 0;
    if (!labels || !out || !workspace || bad_elem_bytes(elem_bytes) || sk_bad_method(method)) return PTB_EINVAL;
    if (object_rule != PTB_THIN_EQUAL && object_rule != PTB_THIN_NOT_EQUAL) return PTB_EINVAL;
    SkPlan p;
    if (int rc = sk_plan(B, H, W, false, p)) return rc;
    if (workspace_bytes < p.bytes || !aligned16(workspace) || !aligned16(out)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    RelaxFlags f;
    if (int rc = relax_flags(ws, p, st, f)) return rc;
    sk_pack(labels, elem_bytes, B, 1, &value, object_rule == PTB_THIN_NOT_EQUAL, 0u, p, ws, f, st);
    int final_plane = 0;
    if (int rc = sk_thin(p, ws, f, method, max_iterations, st, took, final_plane)) return rc;
    const unsigned words = (unsigned)(B * p.plane_words);
    with_bool(W % 16 == 0, [&](auto wd) {
        hipLaunchKernelGGL((sk_unpack_kernel<wd()>), dim3((words + SK_THREADS - 1) / SK_THREADS), dim3(SK_THREADS), 0, st,
                           reinterpret_cast<const unsigned*>(ws + (final_plane ? p.off_b : p.off_a)), reinterpret_cast<unsigned char*>(out), words, (int)W, (int)p.WW);
    });
    return check_launch();
}

extern "C" int ptb_centerline_dice_plan(int64_t B, int64_t H, int64_t W, int K, int64_t* workspace_bytes) {
    if (K < 1 || K > SK_MAX_CLASSES || B < 1) return PTB_EINVAL;
    if (B > MAX_POS / (2 * K)) return PTB_EUNSUPPORTED;
    SkPlan p;
    if (int rc = sk_plan(2 * K * B, H, W, true, p)) return rc;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return PTB_OK;
}

extern "C" int ptb_centerline_dice(const void* pred, int pred_elem_bytes, const void* truth, int truth_elem_bytes, int64_t B, int64_t H, int64_t W,
                                   const int64_t* class_values, int K, int object_rule, int method, int64_t* counts, float* cldice, float* tprec,
                                   float* tsens, int32_t* took, void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (took) took[0] = took[1] = 0;
    if (!pred || !truth || !class_values || !counts || !cldice || !tprec || !tsens || !workspace) return PTB_EINVAL;
    if (bad_elem_bytes(pred_elem_bytes) || bad_elem_bytes(truth_elem_bytes) || sk_bad_method(method)) return PTB_EINVAL;
    if (object_rule != PTB_THIN_EQUAL && object_rule != PTB_THIN_NOT_EQUAL) return PTB_EINVAL;
    if (K < 1 || K > SK_MAX_CLASSES || B < 1 || (object_rule == PTB_THIN_NOT_EQUAL && K != 1)) return PTB_EINVAL;
    if (B > MAX_POS / (2 * K)) return PTB_EUNSUPPORTED;
    SkPlan p;
    if (int rc = sk_plan(2 * K * B, H, W, true, p)) return rc;
    if (workspace_bytes < p.bytes || !aligned16(workspace)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    RelaxFlags f;
    if (int rc = relax_flags(ws, p, st, f)) return rc;
    const unsigned BK = (unsigned)(B * K);
    if (int rc = relax_hip(hipMemsetAsync(counts, 0, (size_t)BK * 4 * sizeof(int64_t), st))) return rc;
    const int not_equal = object_rule == PTB_THIN_NOT_EQUAL;
    sk_pack(pred, pred_elem_bytes, B, K, class_values, not_equal, 0u, p, ws, f, st);
    sk_pack(truth, truth_elem_bytes, B, K, class_values, not_equal, BK, p, ws, f, st);
    int final_plane = 0;
    if (int rc = sk_thin(p, ws, f, method, -1, st, took, final_plane)) return rc;
    const unsigned blocks = (unsigned)std::min<long long>((p.plane_words + SK_THREADS - 1) / SK_THREADS, std::max<long long>(1, std::min<long long>(1024, (1LL << 30) / p.planes)));
    hipLaunchKernelGGL(sk_count_kernel, dim3(blocks * 2u * BK), dim3(SK_THREADS), 0, st, reinterpret_cast<const unsigned*>(ws + (final_plane ? p.off_b : p.off_a)),
                       reinterpret_cast<const unsigned*>(ws + p.off_v), reinterpret_cast<unsigned long long*>(counts), (unsigned)p.plane_words, BK, blocks);
    hipLaunchKernelGGL(sk_finish_kernel, dim3(1), dim3(SK_THREADS), 0, st, reinterpret_cast<const unsigned long long*>(counts), cldice, tprec, tsens, BK);
    return check_launch();
}
