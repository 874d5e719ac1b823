// What the plane unit (ptb_skeleton.hip) and the volume unit (ptb_skeleton3d.hip) of the thinning share: the bit-plane layout and its
// place in the workspace, the body of the pack kernel (each unit wraps it in a kernel of its own with its rule for "the tile of a
// word"), and the host entries of the kernels that know no tile at all -- unpack, count, finish -- which live in ptb_skeleton.hip and
// are launched from both units.
// BIT PLANES.  32 positions along x a word, WW = ceil(W / 32) words a row, `rows` rows an entry (2-D: H, 3-D: D * H, row = z * H + y);
// bits at columns >= W are 0 and stay 0.  Two planes A and B for the ping-pong of the launches, and for clDice the untouched masks V.
#pragma once

#include "ptb_common.h"
#include "ptb_relax_device.h"

namespace ptb {

constexpr int SK_THREADS = RELAX_THREADS;
constexpr int SK_MAX_CLASSES = 32;

struct SkPackArgs {
    const void* labels;         // [B, rows, W]
    unsigned* a;                // the two thinning planes and (or NULL) the mask plane: [planes, rows, WW] each
    unsigned* b;
    unsigned* v;
    unsigned* start_flags;      // [planes * tiles_per_entry] zeroed by the caller
    long long values[SK_MAX_CLASSES];
    unsigned held;              // bit k: the element type holds values[k] (else it occurs nowhere)
    int K, not_equal;           // the object of class k: labels == values[k], or (K == 1) labels != values[0]
    unsigned plane0;            // plane of (entry b, class k) = plane0 + b * K + k
    unsigned words;             // B * rows * WW
    int H, W, WW;               // H: the rows of an entry
    RelaxGeom g;
};

// one thread packs one word of every class; tile_of(a, row within the entry, word column) names the tile whose start flag the word raises
template <int EB, bool WIDE, class TileOf>
__device__ __forceinline__ void sk_pack_body(const SkPackArgs& a, TileOf tile_of) {
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
    const unsigned tile = tile_of(a, y, w);
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

// The workspace: the sweep words and tile flags (RelaxPlan), then the planes A and B and, for clDice, the masks: 4 * rows * WW bytes per plane.
struct SkPlan : RelaxPlan {
    long long planes, WW, plane_words, off_a, off_b, off_v;
};

// the planes behind a RelaxPlan that is already laid out
static inline void sk_plan_planes(long long planes, long long rows, long long W, bool masks, SkPlan& p) {
    p.planes = planes; p.WW = (W + 31) / 32; p.plane_words = rows * p.WW;
    const long long bytes = up16(4 * planes * p.plane_words);
    p.off_a = p.bytes; p.bytes += bytes;
    p.off_b = p.bytes; p.bytes += bytes;
    p.off_v = masks ? p.bytes : -1;
    if (masks) p.bytes += bytes;
}

// the arguments of a pack launch over B entries of `rows` rows, and the workgroups it takes; `wide`: the 16-byte loads
static inline SkPackArgs sk_pack_args(const void* labels, int elem_bytes, long long B, int K, const int64_t* values, int not_equal, unsigned plane0, const SkPlan& p,
                                      long long rows, char* ws, const RelaxFlags& f, bool& wide, unsigned& blocks) {
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
    a.H = (int)rows; a.W = p.g.W; a.WW = (int)p.WW; a.g = p.g;
    wide = aligned16(labels) && ((long long)a.W * elem_bytes) % 16 == 0;
    blocks = (a.words + SK_THREADS - 1) / SK_THREADS;
    return a;
}

// ptb_skeleton.hip: `words` words of `plane` as bytes 0 | 1 into out [words / WW rows, W]
void sk_unpack(const unsigned* plane, void* out, unsigned words, long long W, long long WW, hipStream_t st);
// ptb_skeleton.hip: the clDice counts [BK][4] (zeroed by the caller) of the 2 * BK planes `skel` against `mask`, then the three ratios
void sk_count_finish(const unsigned* skel, const unsigned* mask, long long planes, long long plane_words, unsigned BK, int64_t* counts, float* cldice, float* tprec,
                     float* tsens, hipStream_t st);

}  // namespace ptb
