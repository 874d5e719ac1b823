// Grey and binary morphology with a flat structuring element (utils/morphology.py; the reference has no counterpart): erosion,
// dilation, opening, closing and, for grey values, the three differences built on them.
// DEFINITIONS.  The footprint F has shape (fh, fw) and anchor (fh / 2, fw / 2); its offsets are O = {(i - fh / 2, j - fw / 2) : F[i, j]},
// every one with |dy|, |dx| <= MORPH_REACH = 31.  E(x)(p) = min over o in O of x(p + o);  D(x)(p) = max over o in O of x(p - o) (the
// reflected footprint: scipy's convention, not OpenCV's);  opening = D o E, closing = E o D;  gradient = D - E, white top-hat = x - opening,
// black top-hat = closing - x.  Without a border value the positions outside the entry never take part, and a window that lies wholly
// outside gives the highest value of the element type (+inf for floats) for E and the lowest for D; with one they hold that value.
// Values are only selected, so a result is exact in the element type; the differences subtract in the type: integers saturate, floats
// take one float32 subtraction rounded once (to nearest even) to the type.
// ONE DESIGN FOR EVERY FOOTPRINT.  The host splits F into its horizontal RUNS (dy, a, b) -- the maximal stretches of set columns
// a .. b of row dy -- at most MORPH_MAX_RUNS = 256 of them, one 32-bit word each with the level p = floor(log2(b - a + 1)); the table travels in
// the kernel-argument structure.  Both walks compute R(p) = min over the GATHER offsets g of x(p + g): g = o for E, g = -o (the reflected
// table) on complemented keys for D.  A windowed minimum of length L along a row is min(T_p[x + a], T_p[x + b - 2^p + 1]) with T_0 the row
// and T_p+1[x] = min(T_p[x], T_p[x + 2^p]); levels 0 .. 5 cover L <= 63.
//   morph_walk_kernel   grey values.  A workgroup of MORPH_STRIP threads owns a strip of MORPH_STRIP columns of one entry and a band of
//                       MORPH_BAND of its rows, and walks the input rows y0 + dy_min .. y1 - 1 + dy_max top to bottom (with a border value
//                       the rows outside the entry too, as constant rows; without one they are skipped).  Per input row r: (1) the
//                       strip's segment with 31 columns on either side goes to LDS as ordered 32-bit keys (relax_order: monotone, -0 as
//                       +0, a NaN with the sign bit clear above +inf and one with it set below -inf); columns outside hold the border key
//                       or the identity 0xFFFFFFFF; (2) the levels the footprint uses are built in place next to it, one barrier each;
//                       (3) every lane owns one column: for every run it takes the two-read minimum from the run's level and folds it
//                       into the accumulator of output row r - dy -- the scatter form: each (row, run) pair is used exactly once.  The
//                       accumulators are a ring of RING >= dy_max - dy_min + 1 rows [slot][column] in LDS, slot = y mod RING, private to
//                       their lane: no synchronisation.  When row y + dy_max has been folded, slot y is converted back from its key (the
//                       identity: "nothing took part"), optionally subtracted from / by `other` at that position, stored, and reset.
//   morph_bits_kernel   the same walk on bit planes: 32 positions a word, one lane per word, one wave per workgroup, MORPH_BIT_WORDS
//                       owned words with ONE word of halo on either side (|dx| <= 31), MORPH_BIT_BAND rows.  It computes the dilation
//                       OR over g of x(p + g); T_p+1 = T_p | funnelshift(T_p, 2^p) across neighbouring words, a run is two funnel
//                       shifts and an OR.  Erosion is the dilation of the complement, complemented (duality).  The load stage packs the
//                       object rule from 32 label elements in registers or reads a bit plane; the store stage writes bytes 0 | 1 or a
//                       bit plane.  A bit of a halo word that would need the word beyond it is never consumed: a read at x + d, d <= 31 - 2^p
//                       + 1, of T_p covers columns up to x + 31, which lie in the next word.
// Opening and closing are two launches with the intermediate in the workspace (the element type; a bit plane); the differences are a
// store-stage mode of the last launch.  No scratch memory, no atomics, no workgroup waits for another one, every loop is bounded, and the
// result is a function of the inputs alone.
// LDS: the walk holds 6 levels of MORPH_ROW = MORPH_STRIP + 64 words and RING x MORPH_STRIP words: 4 * (6 * 256 + 64 * 192) = 55296 bytes
// for the largest ring, so two workgroups share the 160 KiB of a CU; the smaller rings (4, 16, 32) take 9216, 18432 and 30720 bytes.
#include <algorithm>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_relax_device.h"

namespace ptb {

constexpr int MORPH_REACH = PTB_MORPH_REACH;
constexpr int MORPH_MAX_RUNS = PTB_MORPH_MAX_RUNS;
constexpr int MORPH_LEVELS = 6;
constexpr int MORPH_STRIP = 192;                // columns a workgroup owns: one lane each
constexpr int MORPH_BAND = 128;                 // output rows a workgroup walks
constexpr int MORPH_ROW = MORPH_STRIP + 64;     // the segment with its halo of 31 on either side, and two words of padding
constexpr int MORPH_BIT_LANES = 64;             // one wave
constexpr int MORPH_BIT_WORDS = MORPH_BIT_LANES - 2;        // owned words of a strip: 1984 columns
constexpr int MORPH_BIT_BAND = 64;
constexpr unsigned MORPH_ID = 0xFFFFFFFFu;      // the key of "nothing took part"
static_assert(MORPH_STRIP + 2 * MORPH_REACH <= MORPH_ROW && (1 << (MORPH_LEVELS - 1)) <= MORPH_REACH + 1, "the halo and the levels cover every run");

// a run is ONE 32-bit word, dy | a << 8 | b << 16 | p << 24 (the first three signed bytes), taken apart with shifts: the table is read with
// scalar loads at a run-time index, and whole aligned words are what those read (with byte-wise fields the compiler formed them from a
// base one byte into the word plus an offset of 3, and that load returned the run before: DESIGN.md, "Morphology")
struct MorphRun {
    int dy, a, b, p;
};
__host__ __device__ __forceinline__ MorphRun morph_run(unsigned w) { return MorphRun{(int)(w << 24) >> 24, (int)(w << 16) >> 24, (int)(w << 8) >> 24, (int)(w >> 24)}; }

struct MorphTable {
    int n, dy_min, dy_max, p_max;
    unsigned runs[MORPH_MAX_RUNS];              // sorted by dy
};

struct MorphWalkArgs {
    const void* src;            // [B, H, W] of the element type
    const void* other;          // the same, read at the output position when diff != 0
    void* dst;
    int H, W, nstrips, nbands;
    unsigned flip;              // 0: minima; ~0: maxima, on complemented keys
    unsigned outside;           // the key of a position outside the entry
    int walk_outside;           // rows outside the entry are walked as constant rows (a border value)
    int diff;                   // 0: the result; 1: result - other; 2: other - result
    float empty;                // what a window that lies wholly outside gives
    MorphTable t;
};

// the difference forms round / saturate to the element type
template <int DT>
__device__ __forceinline__ typename RelaxValue<DT>::R morph_round(float v) {
    if constexpr (DT == PTB_U8) return (unsigned char)fminf(fmaxf(v, 0.0f), 255.0f);
    else if constexpr (DT == PTB_I16) return (short)fminf(fmaxf(v, -32768.0f), 32767.0f);
    else if constexpr (DT == PTB_BF16) {
        const unsigned b = __float_as_uint(v);
        if (v != v) return (unsigned short)0x7FC0u;
        return (unsigned short)((b + 0x7FFFu + (b >> 16 & 1u)) >> 16);         // to nearest even
    } else return RelaxValue<DT>::put(v);
}

// LAUNCHED WITH EXACTLY MORPH_STRIP THREADS over B * nbands * nstrips workgroups
template <int DT, int RING>
__global__ __launch_bounds__(MORPH_STRIP) void morph_walk_kernel(const MorphWalkArgs a) {
    using V = RelaxValue<DT>;
    using R = typename V::R;
    __shared__ unsigned sT[MORPH_LEVELS][MORPH_ROW];
    __shared__ unsigned sAcc[RING][MORPH_STRIP];
    const int tid = (int)threadIdx.x;
    unsigned blk = blockIdx.x;
    const int strip = (int)(blk % (unsigned)a.nstrips);
    blk /= (unsigned)a.nstrips;
    const int band = (int)(blk % (unsigned)a.nbands);
    const size_t ebase = (size_t)(blk / (unsigned)a.nbands) * ((size_t)a.H * (size_t)a.W);
    const int x0 = strip * MORPH_STRIP, y0 = band * MORPH_BAND, y1 = min(y0 + MORPH_BAND, a.H);
    const R* src = reinterpret_cast<const R*>(a.src) + ebase;
    const R* other = reinterpret_cast<const R*>(a.other) + ebase;
    R* dst = reinterpret_cast<R*>(a.dst) + ebase;
    const int gx = x0 + tid;
#pragma unroll 1
    for (int s = 0; s < RING; ++s) sAcc[s][tid] = MORPH_ID;

#pragma unroll 1
    for (int r = y0 + a.t.dy_min; r < y1 + a.t.dy_max; ++r) {
        const bool inside = r >= 0 && r < a.H;
        if (inside || a.walk_outside) {                                        // (workgroup-uniform)
            __syncthreads();                                                   // every read of the row before is done
#pragma unroll
            for (int c = tid; c < MORPH_ROW; c += MORPH_STRIP) {
                const int cx = x0 - MORPH_REACH + c;
                unsigned k = a.outside;
                if (inside && cx >= 0 && cx < a.W) k = relax_order(V::get(src[(size_t)r * (size_t)a.W + (size_t)cx]), a.flip);
                sT[0][c] = k;
            }
            __syncthreads();
#pragma unroll 1
            for (int p = 1; p <= a.t.p_max; ++p) {
                const int h = 1 << (p - 1);
#pragma unroll
                for (int c = tid; c < MORPH_ROW; c += MORPH_STRIP) {
                    unsigned v = sT[p - 1][c];
                    if (c + h < MORPH_ROW) v = min(v, sT[p - 1][c + h]);
                    sT[p][c] = v;
                }
                __syncthreads();
            }
            const int at = tid + MORPH_REACH;
            int j = 0;
#pragma unroll 1
            while (j < a.t.n) {                                                // the runs of one dy fold into one slot
                const int dy = morph_run(a.t.runs[j]).dy, y = r - dy;
                const bool live = y >= y0 && y < y1;
                unsigned v = MORPH_ID;
                do {
                    const MorphRun q = morph_run(a.t.runs[j]);
                    if (live) v = min(v, min(sT[q.p][at + q.a], sT[q.p][at + q.b - (1 << q.p) + 1]));
                    ++j;
                } while (j < a.t.n && morph_run(a.t.runs[j]).dy == dy);
                if (live) {
                    unsigned* acc = &sAcc[y & (RING - 1)][tid];
                    *acc = min(*acc, v);
                }
            }
        }
        const int y = r - a.t.dy_max;                                          // complete: every row it gathers from has been folded
        if (y >= y0) {                                                         // (y < y1 by the loop's bound)
            unsigned* acc = &sAcc[y & (RING - 1)][tid];
            const unsigned k = *acc;
            *acc = MORPH_ID;
            if (gx < a.W) {
                const size_t at = (size_t)y * (size_t)a.W + (size_t)gx;
                const float v = k == MORPH_ID ? a.empty : relax_unorder(k, a.flip);
                if (a.diff == 0) dst[at] = V::put(v);
                else {
                    const float o = V::get(other[at]);
                    dst[at] = morph_round<DT>(a.diff == 1 ? v - o : o - v);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- bit planes
struct MorphBitsArgs {
    const void* src;            // EB != 0: labels [B, H, W] of EB bytes; EB == 0: a bit plane [B, H, WW]
    void* dst;                  // bytes [B, H, W], or a bit plane
    long long value;
    int held, not_equal;        // the object: labels == value (nowhere, if the type does not hold it), or labels != value
    int H, W, WW, nstrips, nbands;
    int invert;                 // erosion: complement on load and on store
    unsigned outside;           // 0 | ~0: the positions outside the entry, in the space the walk runs in
    int walk_outside;
    int wide_in, wide_out;      // 16-byte loads of the labels / stores of the bytes
    int dst_plane;
    MorphTable t;
};

// the word of the row that starts at `row` (columns x0 .. x0 + 31) under the object rule
template <int EB>
__device__ __forceinline__ unsigned morph_pack_word(const MorphBitsArgs& a, const void* row, int x0) {
    using T = label_t<(EB ? EB : 1)>;
    const T* src = reinterpret_cast<const T*>(row) + x0;
    T el[32];
    if (a.wide_in) {                                                           // the base and every row are 16-byte aligned, W is whole chunks
        constexpr int CH = 16 / (EB ? EB : 1);
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
    const T val = (T)a.value;
    unsigned m = 0u;
#pragma unroll
    for (int j = 0; j < 32; ++j) m |= (el[j] == val ? 1u : 0u) << j;
    if (!a.held) m = 0u;
    return a.not_equal ? ~m : m;
}

// the word of T_p at column offset d (-31 .. 31) from the lane's own: lo, cur, hi are the words of the lane before, the lane and the lane behind
__device__ __forceinline__ unsigned morph_shifted(const unsigned* level, int lane, int d) {
    const int i = lane + (d < 0 ? 0 : 1);
    return __funnelshift_r(level[i], level[i + 1], (unsigned)d & 31u);
}

// LAUNCHED WITH EXACTLY MORPH_BIT_LANES THREADS (one wave) over B * nbands * nstrips workgroups
template <int EB, int RING>
__global__ __launch_bounds__(MORPH_BIT_LANES) void morph_bits_kernel(const MorphBitsArgs a) {
    __shared__ unsigned sT[MORPH_LEVELS][MORPH_BIT_LANES + 2];                  // word i + 1 is lane i's; words 0 and 65 stay 0 and are never consumed
    __shared__ unsigned sAcc[RING][MORPH_BIT_LANES];
    const int lane = (int)threadIdx.x;
    unsigned blk = blockIdx.x;
    const int strip = (int)(blk % (unsigned)a.nstrips);
    blk /= (unsigned)a.nstrips;
    const int band = (int)(blk % (unsigned)a.nbands);
    const size_t e = blk / (unsigned)a.nbands;
    const int w = strip * MORPH_BIT_WORDS - 1 + lane, y0 = band * MORPH_BIT_BAND, y1 = min(y0 + MORPH_BIT_BAND, a.H);
    const bool has_word = w >= 0 && w < a.WW, owned = has_word && lane >= 1 && lane <= MORPH_BIT_WORDS;
    const int left = a.W - w * 32;                                             // (only used where has_word)
    const unsigned valid = left >= 32 ? 0xFFFFFFFFu : (1u << (left & 31)) - 1u;
#pragma unroll 1
    for (int s = 0; s < RING; ++s) sAcc[s][lane] = 0u;
    if (lane < MORPH_LEVELS) sT[lane][0] = sT[lane][MORPH_BIT_LANES + 1] = 0u;

#pragma unroll 1
    for (int r = y0 + a.t.dy_min; r < y1 + a.t.dy_max; ++r) {
        const bool inside = r >= 0 && r < a.H;
        if (inside || a.walk_outside) {
            unsigned m = a.outside;
            if (inside && has_word) {
                const size_t row = e * (size_t)a.H + (size_t)r;
                if constexpr (EB == 0) m = reinterpret_cast<const unsigned*>(a.src)[row * (size_t)a.WW + (size_t)w];
                else m = morph_pack_word<EB>(a, reinterpret_cast<const char*>(a.src) + row * (size_t)a.W * EB, w * 32);
                if (a.invert) m = ~m;
                m = (m & valid) | (a.outside & ~valid);
            }
            __syncthreads();                                                   // every read of the row before is done
            sT[0][lane + 1] = m;
            __syncthreads();
#pragma unroll 1
            for (int p = 1; p <= a.t.p_max; ++p) {
                sT[p][lane + 1] = sT[p - 1][lane + 1] | morph_shifted(sT[p - 1], lane, 1 << (p - 1));
                __syncthreads();
            }
            int j = 0;
#pragma unroll 1
            while (j < a.t.n) {
                const int dy = morph_run(a.t.runs[j]).dy, y = r - dy;
                const bool live = y >= y0 && y < y1;
                unsigned v = 0u;
                do {
                    const MorphRun q = morph_run(a.t.runs[j]);
                    if (live) v |= morph_shifted(sT[q.p], lane, q.a) | morph_shifted(sT[q.p], lane, q.b - (1 << q.p) + 1);
                    ++j;
                } while (j < a.t.n && morph_run(a.t.runs[j]).dy == dy);
                if (live) sAcc[y & (RING - 1)][lane] |= v;
            }
        }
        const int y = r - a.t.dy_max;
        if (y >= y0) {
            unsigned m = sAcc[y & (RING - 1)][lane];
            sAcc[y & (RING - 1)][lane] = 0u;
            if (a.invert) m = ~m;
            if (owned) {
                const size_t row = e * (size_t)a.H + (size_t)y;
                if (a.dst_plane) reinterpret_cast<unsigned*>(a.dst)[row * (size_t)a.WW + (size_t)w] = m;
                else {
                    unsigned char* dst = reinterpret_cast<unsigned char*>(a.dst) + row * (size_t)a.W + (size_t)w * 32u;
                    if (a.wide_out) {                                          // dst is 16-byte aligned and W % 16 == 0
#pragma unroll
                        for (int c = 0; c < 2; ++c)
                            if (c * 16 < left) {
                                unsigned char o[16];
#pragma unroll
                                for (int i = 0; i < 16; ++i) o[i] = (unsigned char)(m >> (c * 16 + i) & 1u);
                                __builtin_memcpy(__builtin_assume_aligned(dst + c * 16, 16), o, 16);
                            }
                    } else {
#pragma unroll
                        for (int i = 0; i < 32; ++i)
                            if (i < left) dst[i] = (unsigned char)(m >> i & 1u);
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
static bool morph_bad_op(int op, int last) { return op < PTB_MORPH_EROSION || op > last; }

// the gather table of a launch from the footprint's runs (HOST int32 [n][3] = dy, a, b): reflected for a dilation, sorted by dy
static int morph_table(const int32_t* runs, int n, bool reflect, MorphTable& t) {
    if (!runs || n < 1 || n > MORPH_MAX_RUNS) return PTB_EINVAL;
    t.n = n; t.dy_min = MORPH_REACH; t.dy_max = -MORPH_REACH; t.p_max = 0;
    MorphRun sorted[MORPH_MAX_RUNS];
    for (int i = 0; i < n; ++i) {
        int dy = runs[3 * i], a = runs[3 * i + 1], b = runs[3 * i + 2];
        if (dy < -MORPH_REACH || dy > MORPH_REACH || a < -MORPH_REACH || b > MORPH_REACH || a > b) return PTB_EINVAL;
        if (reflect) {
            dy = -dy;
            const int na = -b;
            b = -a; a = na;
        }
        int p = 0;
        while ((2 << p) <= b - a + 1) ++p;
        sorted[i] = MorphRun{dy, a, b, p};
        t.dy_min = std::min(t.dy_min, dy); t.dy_max = std::max(t.dy_max, dy); t.p_max = std::max(t.p_max, p);
    }
    std::stable_sort(sorted, sorted + n, [](const MorphRun& l, const MorphRun& r) { return l.dy < r.dy; });
    for (int i = 0; i < n; ++i) t.runs[i] = ((unsigned)sorted[i].dy & 0xFFu) | ((unsigned)sorted[i].a & 0xFFu) << 8 | ((unsigned)sorted[i].b & 0xFFu) << 16 | (unsigned)sorted[i].p << 24;
    return PTB_OK;
}

static int morph_elem_bytes(int dtype) { return dtype == PTB_F32 ? 4 : dtype == PTB_U8 ? 1 : 2; }

static float morph_extreme(int dtype, bool top) {
    if (dtype == PTB_U8) return top ? 255.0f : 0.0f;
    if (dtype == PTB_I16) return top ? 32767.0f : -32768.0f;
    return top ? __builtin_inff() : -__builtin_inff();
}

static unsigned morph_host_key(float v, unsigned flip) {       // relax_order on the host
    unsigned b;
    __builtin_memcpy(&b, &v, 4);
    if (v == 0.0f) b = 0u;
    return ((b & 0x80000000u) ? ~b : (b | 0x80000000u)) ^ flip;
}

static void morph_walk(int dtype, MorphWalkArgs& a, long long B, const int32_t* runs, int n, bool dilate, int border, float border_value, hipStream_t st) {
    morph_table(runs, n, dilate, a.t);                                         // (validated by the caller)
    a.flip = dilate ? 0xFFFFFFFFu : 0u;
    a.outside = border ? morph_host_key(border_value, a.flip) : MORPH_ID;
    a.walk_outside = border != 0;
    a.empty = morph_extreme(dtype, !dilate);
    a.nstrips = (a.W + MORPH_STRIP - 1) / MORPH_STRIP; a.nbands = (a.H + MORPH_BAND - 1) / MORPH_BAND;
    const unsigned grid = (unsigned)(B * a.nbands * a.nstrips);                // (at most one workgroup per position: < 2^31)
    with_value<PTB_F16, PTB_BF16, PTB_U8, PTB_I16, PTB_F32>(dtype, [&](auto dt) {
        with_at_most<4, 16, 32, 64>(a.t.dy_max - a.t.dy_min + 1, [&](auto ring) {
            hipLaunchKernelGGL((morph_walk_kernel<dt(), ring()>), dim3(grid), dim3(MORPH_STRIP), 0, st, a);
        });
    });
}

static void morph_bits(int elem_bytes, MorphBitsArgs& a, long long B, const int32_t* runs, int n, bool dilate, int border, hipStream_t st) {
    morph_table(runs, n, dilate, a.t);
    a.invert = !dilate;
    a.outside = border < 0 ? 0u : ((border != 0) != !dilate ? 0xFFFFFFFFu : 0u);       // erosion walks the complement
    a.walk_outside = a.outside != 0u;
    a.nstrips = (a.WW + MORPH_BIT_WORDS - 1) / MORPH_BIT_WORDS; a.nbands = (a.H + MORPH_BIT_BAND - 1) / MORPH_BIT_BAND;
    const unsigned grid = (unsigned)(B * a.nbands * a.nstrips);
    with_value<0, 1, 2, 4, 8>(elem_bytes, [&](auto eb) {
        with_at_most<4, 16, 64>(a.t.dy_max - a.t.dy_min + 1, [&](auto ring) {
            hipLaunchKernelGGL((morph_bits_kernel<eb(), ring()>), dim3(grid), dim3(MORPH_BIT_LANES), 0, st, a);
        });
    });
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_morphology_geometry(int32_t* out) {
    if (!out) return PTB_EINVAL;
    out[0] = MORPH_STRIP; out[1] = MORPH_BAND; out[2] = MORPH_BIT_WORDS; out[3] = MORPH_BIT_BAND;
    return PTB_OK;
}

extern "C" int ptb_morphology_plan(int64_t B, int64_t H, int64_t W, int op, int elem_bytes, int64_t* workspace_bytes) {
    if (int rc = check_shape(2, B, 1, H, W)) return rc;
    if (morph_bad_op(op, PTB_MORPH_BLACK_TOPHAT) || (elem_bytes != 0 && elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)) return PTB_EINVAL;
    const bool compound = op >= PTB_MORPH_OPENING;
    if (workspace_bytes) *workspace_bytes = !compound ? 0 : elem_bytes ? up16(B * H * W * elem_bytes) : up16(4 * B * H * ((W + 31) / 32));
    return PTB_OK;
}

extern "C" int ptb_morphology(const void* image, int dtype, int64_t B, int64_t H, int64_t W, int op, const int32_t* runs, int n_runs, int border,
                              float border_value, void* out, void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (!image || !out || dtype < PTB_F32 || dtype > PTB_I16 || morph_bad_op(op, PTB_MORPH_BLACK_TOPHAT) || (border != 0 && border != 1)) return PTB_EINVAL;
    if (int rc = check_shape(2, B, 1, H, W)) return rc;
    MorphWalkArgs a{};
    if (int rc = morph_table(runs, n_runs, false, a.t)) return rc;
    if (border && border_value != border_value) return PTB_EINVAL;
    int64_t need = 0;
    ptb_morphology_plan(B, H, W, op, morph_elem_bytes(dtype), &need);
    if (need && (!workspace || workspace_bytes < need || !aligned16(workspace))) return PTB_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    a.H = (int)H; a.W = (int)W;
    // the first walk of a compound form is an erosion for the opening, the gradient and the white top-hat, a dilation for the closing and the black top-hat
    const bool first_dilates = op == PTB_MORPH_DILATION || op == PTB_MORPH_CLOSING || op == PTB_MORPH_BLACK_TOPHAT;
    a.src = image; a.other = image; a.dst = need ? workspace : out;
    morph_walk(dtype, a, B, runs, n_runs, first_dilates, border, border_value, st);
    if (need) {
        const bool gradient = op == PTB_MORPH_GRADIENT;
        a.src = gradient ? image : workspace; a.other = gradient ? workspace : image; a.dst = out;
        a.diff = gradient || op == PTB_MORPH_BLACK_TOPHAT ? 1 : op == PTB_MORPH_WHITE_TOPHAT ? 2 : 0;
        morph_walk(dtype, a, B, runs, n_runs, gradient || !first_dilates, border, border_value, st);
    }
    return check_launch();
}

extern "C" int ptb_binary_morphology(const void* labels, int elem_bytes, int64_t B, int64_t H, int64_t W, int object_rule, int64_t value, int op,
                                     const int32_t* runs, int n_runs, int border, void* out, void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (!labels || !out || bad_elem_bytes(elem_bytes) || morph_bad_op(op, PTB_MORPH_CLOSING) || border < -1 || border > 1) return PTB_EINVAL;
    if (object_rule != PTB_THIN_EQUAL && object_rule != PTB_THIN_NOT_EQUAL) return PTB_EINVAL;
    if (int rc = check_shape(2, B, 1, H, W)) return rc;
    MorphBitsArgs a{};
    if (int rc = morph_table(runs, n_runs, false, a.t)) return rc;
    int64_t need = 0;
    ptb_morphology_plan(B, H, W, op, 0, &need);
    if (need && (!workspace || workspace_bytes < need || !aligned16(workspace))) return PTB_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    a.H = (int)H; a.W = (int)W; a.WW = (int)((W + 31) / 32);
    a.value = value; a.held = holds(elem_bytes, value); a.not_equal = object_rule == PTB_THIN_NOT_EQUAL;
    a.wide_in = aligned16(labels) && (W * elem_bytes) % 16 == 0;
    a.wide_out = aligned16(out) && W % 16 == 0;
    const bool first_dilates = op == PTB_MORPH_DILATION || op == PTB_MORPH_CLOSING;
    a.src = labels; a.dst = need ? workspace : out; a.dst_plane = need != 0;
    morph_bits(elem_bytes, a, B, runs, n_runs, first_dilates, border, st);
    if (need) {
        a.src = workspace; a.dst = out; a.dst_plane = 0;
        morph_bits(0, a, B, runs, n_runs, !first_dilates, border, st);
    }
    return check_launch();
}
