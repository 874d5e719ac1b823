// Surface metrics of two label maps on the device (utils/surface.py; the reference has no counterpart): Hausdorff distance, a percentile
// of it, mean surface distances and surface Dice of K objects of every stack entry, from the two border maps and their distance
// transforms.  The classes are worked off in chunks of C; per chunk:
//   1. surf_border_kernel   (a launch per side) a wave per row, four neighbouring x per lane and trip like edt_row_kernel.  It reads the
//                           label map where it lies, in its dtype, the row itself and the neighbouring rows / slices from global memory
//                           (they are in L2: a row is read by the waves of three or nine rows), x - 1 and x + 4 by wave shuffles.  A
//                           position is BORDER of the object it belongs to iff a connectivity-neighbour belongs to another one or lies
//                           outside the map.  One 0/1 byte per position and class goes to border[c][side][b][...]; the surface counts are
//                           ballots added to LDS counters and flushed with one integer atomic per class and workgroup.
//   2. ptb_edt              ONE transform of the whole stack [C * 2 * B] of border maps (sites: the positions that hold 1): exact int32
//                           squared distances, or float32 ones with spacing.  2 C B maps share the launches of the line passes.
//   3. surf_stats_kernel    walks the border map of (class, side, entry) and, where the flag is set, loads the OTHER side's
//                           squared distance: the sample's key, its uint32 bits (int32 >= 0 and float32 >= +0 both order like their
//                           bits).  Maximum (atomicMax), tolerance counts (key <= threshold bits, atomicAdd), the sum of the roots in
//                           double, and the first histogram of the selection.
//      surf_hist_kernel     the same walk (one body, surf_sample<MODE>): the histograms of the three further bytes.
//      surf_upper_kernel    the same walk: the smallest key above the selected one (atomicMin).
//      surf_pick_kernel     between the histogram passes: a workgroup per (object, selection) scans the 256 counts, fixes the next byte
//                           of the key, lowers the rank and clears the counts.  Ranks live in device memory only.
// and at the end surf_finish_kernel, a lane per object: roots, interpolation and means in double, rounded once to float32.
// SELECTION.  Three per object: the two directed sample sets and the pooled one.  A workgroup of the sample kernels owns one map, hence
// two selections: 2 x 256 private 32-bit LDS counters, flushed with integer atomics where non-zero.  The maps are RE-READ in every pass
// (1 byte per position, 4 more where the flag is set); the samples are not compacted.
// DETERMINISM.  Counts, maxima, histograms and the minimum are integer atomics: exact whatever the order.  The sums are not atomics:
// workgroup j of a map owns the positions [j * seg, (j + 1) * seg) of THAT MAP, lane t of it the 16-position groups t, t + 256, ... of the
// segment in order, lanes are combined by a fixed butterfly and waves in index order, the partial sum goes to its own slot and the finish
// kernel adds the slots in index order.  seg and the slot count depend on D * H * W alone -- not on the device, not on the chunk a class
// falls into -- so neither a second run nor another chunking changes a bit.
// EVERY LOOP IS BOUNDED by the shape; no workgroup waits for another one; nothing is read back.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ptb_common.h"
#include "ptb_dispatch.h"

namespace ptb {

constexpr int SURF_THREADS = 256;
constexpr int SURF_MAX_CHUNK = 32;              // classes per chunk at most: their values travel as kernel arguments
constexpr int SURF_MAX_TOL = 8;
constexpr int SURF_SEG_MIN = 4096;              // positions a workgroup of the sample kernel owns at least ...
constexpr int SURF_MAX_SLOTS = 256;             // ... and workgroups (partial sums) per map at most
constexpr unsigned SURF_INT_INF = 0x7fffffffu;  // ptb_edt's int32 "no site"
constexpr long long SURF_MAX_GRID = 0x7fffffffLL; // workgroups of one launch at most

enum { SURF_IN_EQ = 0, SURF_IN_NE = 1, SURF_IN_NONE = 2, SURF_IN_ALL = 3 };   // a position belongs to the object iff label ==, != value; never; always
enum { SURF_STATS = 0, SURF_HIST = 1, SURF_UPPER = 2 };

// ---------------------------------------------------------------------------------------------------------- device state
// all uint32 unless said; obj = b * K + k
struct SurfState {
    unsigned* count;        // [obj][2]        surface positions of pred, truth
    unsigned* maxkey;       // [obj][2]        largest key of pred -> truth, truth -> pred
    unsigned* tol;          // [obj][8]        samples of both directions with key <= threshold t
    unsigned* prefix;       // [obj][3]        the bytes of the selected key fixed so far
    unsigned* rank;         // [obj][3]        rank of the wanted key among the keys that share the prefix
    unsigned* below;        // [obj][3]        keys smaller than every key that shares the prefix
    unsigned* le;           // [obj][3]        after the last pass: keys <= the selected one
    unsigned* upper;        // [obj][3]        the smallest key above the selected one
    unsigned* hist;         // [obj][3][256]
    double* partial;        // [obj][2][slots]
};

__device__ __forceinline__ double surf_distance(unsigned key, bool flt) {
    if (flt) return sqrt((double)__uint_as_float(key));                       // (inf stays inf)
    return key == SURF_INT_INF ? (double)INFINITY : sqrt((double)key);
}

// ---------------------------------------------------------------------------------------------------------- border
struct SurfBorderArgs {
    const void* labels;
    unsigned char* border;      // [C][2][B][P]
    unsigned* count;            // SurfState::count
    long long values[SURF_MAX_CHUNK];
    int modes[SURF_MAX_CHUNK];
    long long P;
    unsigned B, bpe;            // entries; workgroups per entry
    int D, H, W, K, k0, C, side, full, dims3, object_mode;
    long long object_value;     // labels=None: the background
};

template <class T>
__device__ __forceinline__ T surf_up1(T v) {
    if constexpr (sizeof(T) <= 4) return (T)__shfl_up((int)v, 1);
    else return (T)__shfl_up((long long)v, 1);
}

template <class T>
__device__ __forceinline__ T surf_down1(T v) {
    if constexpr (sizeof(T) <= 4) return (T)__shfl_down((int)v, 1);
    else return (T)__shfl_down((long long)v, 1);
}

// what decides "the same object": the label itself, or with labels=None whether it is foreground
template <class T>
__device__ __forceinline__ T surf_id(T v, int object_mode, T object_value) {
    switch (object_mode) {
        case SURF_IN_NE: return (T)(v != object_value);
        case SURF_IN_ALL: return (T)1;
        default: return v;
    }
}

template <class T, bool WIDE>
__device__ __forceinline__ void surf_load4(const T* row, int x, int W, T (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = (T)0;
    if constexpr (WIDE) {                                                      // W % 4 == 0 and an aligned base: x < W means x + 3 < W
        constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        if (x < W) __builtin_memcpy(v, __builtin_assume_aligned(row + x, A), sizeof(v));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j < W) v[j] = row[x + j];
    }
}

template <class T, bool WIDE>
__global__ __launch_bounds__(SURF_THREADS) void surf_border_kernel(const SurfBorderArgs a) {
    __shared__ unsigned cnt[SURF_MAX_CHUNK];
    if (threadIdx.x < SURF_MAX_CHUNK) cnt[threadIdx.x] = 0;
    __syncthreads();
    const unsigned b = blockIdx.x / a.bpe;                                     // the four rows of a workgroup lie in one entry
    const int r = (int)(blockIdx.x - b * a.bpe) * (SURF_THREADS / 64) + wave_id();
    const int W = a.W, H = a.H, D = a.D;
    if (r < D * H) {                                                           // (wave-uniform)
        const int lane = threadIdx.x & 63;
        const int z = r / H, y = r - z * H;
        const T* entry = reinterpret_cast<const T*>(a.labels) + (size_t)b * (size_t)a.P;
        const T* own_row = entry + (size_t)r * (size_t)W;
        const T ov = (T)a.object_value;
        const int om = a.object_mode;
        const int chunks = (W + 255) / 256;
#pragma unroll 1
        for (int c = 0; c < chunks; ++c) {
            const int x = c * 256 + lane * 4;
            T raw[4], own[4];
            surf_load4<T, WIDE>(own_row, x, W, raw);
#pragma unroll
            for (int j = 0; j < 4; ++j) own[j] = surf_id(raw[j], om, ov);
            bool edge[4] = {false, false, false, false};
#pragma unroll 1
            for (int dz = -1; dz <= 1; ++dz) {
#pragma unroll 1
                for (int dy = -1; dy <= 1; ++dy) {
                    const bool self = dz == 0 && dy == 0;
                    if (!a.full && dz != 0 && dy != 0) continue;               // an edge neighbour: full connectivity only
                    if (dz != 0 && !a.dims3) continue;                         // (dims = 2: no slices; a dims = 3 map of depth 1 has them, outside)
                    const int zz = z + dz, yy = y + dy;
                    if (zz < 0 || zz >= D || yy < 0 || yy >= H) {              // outside the map: not in the object
                        edge[0] = edge[1] = edge[2] = edge[3] = true;
                        continue;
                    }
                    const T* row = entry + ((size_t)zz * (size_t)H + (size_t)yy) * (size_t)W;
                    T v[4];
                    if (self) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = own[j];
                    } else {
                        surf_load4<T, WIDE>(row, x, W, v);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            v[j] = surf_id(v[j], om, ov);
                            edge[j] = edge[j] || v[j] != own[j];
                        }
                    }
                    if (self || a.full) {                                      // x - 1 and x + 1 of that row
                        T left = surf_up1(v[3]), right = surf_down1(v[0]);
                        if (lane == 0 && x > 0 && x - 1 < W) left = surf_id(row[x - 1], om, ov);
                        if (lane == 63 && x + 4 < W) right = surf_id(row[x + 4], om, ov);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const T l = j == 0 ? left : v[j > 0 ? j - 1 : 0];
                            const T rr = j == 3 ? right : v[j < 3 ? j + 1 : 3];
                            edge[j] = edge[j] || x + j - 1 < 0 || l != own[j] || x + j + 1 >= W || rr != own[j];
                        }
                    }
                }
            }
#pragma unroll 1
            for (int k = 0; k < a.C; ++k) {
                const int mode = a.modes[k];
                const T val = (T)a.values[k];
                unsigned n = 0, packed = 0;
                unsigned char* out = a.border + ((size_t)(k * 2 + a.side) * a.B + b) * (size_t)a.P + (size_t)r * (size_t)W;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool in = mode == SURF_IN_EQ ? raw[j] == val : mode == SURF_IN_NE ? raw[j] != val : mode == SURF_IN_ALL;
                    const bool f = x + j < W && in && edge[j];
                    packed |= (unsigned)f << (8 * j);
                    n += (unsigned)__popcll(__ballot(f));
                    if constexpr (!WIDE)
                        if (x + j < W) out[x + j] = (unsigned char)f;
                }
                if constexpr (WIDE)
                    if (x < W) *reinterpret_cast<unsigned*>(out + x) = packed;
                if (lane == 0 && n) atomicAdd(&cnt[k], n);
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < a.C && cnt[threadIdx.x])
        atomicAdd(&a.count[((size_t)b * a.K + a.k0 + threadIdx.x) * 2 + a.side], cnt[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------- samples
struct SurfSampleArgs {
    SurfState st;
    const unsigned char* border;    // [C][2][B][P]
    const unsigned* dist;           // the same stack, transformed
    unsigned thr[SURF_MAX_TOL];     // threshold bits
    long long P, seg;
    unsigned B, slots;
    int K, k0, C, T, shift, flt;
};

// hist: LDS, [2][256] (the directed and the pooled selection; not for SURF_UPPER); wsum: LDS, a double per wave (SURF_STATS only)
template <int MODE>
__device__ __forceinline__ void surf_sample(const SurfSampleArgs& a, unsigned (*hist)[256], double* wsum) {
    const unsigned m = blockIdx.x / a.slots, slot = blockIdx.x - m * a.slots;         // the map [c][side][b] and the segment of it
    const unsigned b = m % a.B, cs = m / a.B, side = cs & 1, c = cs >> 1;
    const size_t obj = (size_t)b * a.K + a.k0 + c;
    const unsigned other = (c * 2 + (side ^ 1)) * a.B + b;
    const unsigned char* bm = a.border + (size_t)m * (size_t)a.P;
    const unsigned* dm = a.dist + (size_t)other * (size_t)a.P;
    const long long lo = (long long)slot * a.seg, hi = std::min(a.P, lo + a.seg);     // (seg is a multiple of 16)
    const bool wide = (reinterpret_cast<uintptr_t>(bm) & 15u) == 0;                    // uniform: groups are aligned relative to the MAP
    const int lane = threadIdx.x & 63;

    unsigned pre_d = 0, pre_p = 0, sel_d = 0, sel_p = 0;
    if constexpr (MODE == SURF_HIST) {
        pre_d = a.st.prefix[obj * 3 + side];
        pre_p = a.st.prefix[obj * 3 + 2];
    }
    if constexpr (MODE == SURF_UPPER) {
        sel_d = a.st.prefix[obj * 3 + side];
        sel_p = a.st.prefix[obj * 3 + 2];
    }
    if constexpr (MODE != SURF_UPPER) {
        hist[0][threadIdx.x] = 0;
        hist[1][threadIdx.x] = 0;
        __syncthreads();
    }
    unsigned best = 0, up_d = 0xffffffffu, up_p = 0xffffffffu;
    unsigned tc[SURF_MAX_TOL] = {0, 0, 0, 0, 0, 0, 0, 0};
    double sum = 0.0;

#pragma unroll 1
    for (long long g = lo + (long long)threadIdx.x * 16; g < hi; g += (long long)SURF_THREADS * 16) {
        unsigned w[4] = {0, 0, 0, 0};
        if (wide) {                                                            // (the buffer is padded to 16: the last group may be read whole)
            __builtin_memcpy(w, __builtin_assume_aligned(bm + g, 16), 16);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)                                       // (unrolled: w is indexed by constants only)
                if (g + j < hi) w[j >> 2] |= (unsigned)bm[g + j] << (8 * (j & 3));
        }
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
            const unsigned word = q == 0 ? w[0] : q == 1 ? w[1] : q == 2 ? w[2] : w[3];
            if (!word) continue;
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const long long p = g + q * 4 + j;
                if (!((word >> (8 * j)) & 1u) || p >= hi) continue;
                const unsigned key = dm[p];
                if constexpr (MODE == SURF_STATS) {
                    best = max(best, key);
#pragma unroll
                    for (int t = 0; t < SURF_MAX_TOL; ++t) tc[t] += (unsigned)(t < a.T && key <= a.thr[t]);
                    sum += surf_distance(key, a.flt != 0);
                    atomicAdd(&hist[0][key >> 24], 1u);
                    atomicAdd(&hist[1][key >> 24], 1u);
                } else if constexpr (MODE == SURF_HIST) {
                    const unsigned top = key >> (a.shift + 8), bin = (key >> a.shift) & 255u;
                    if (top == pre_d) atomicAdd(&hist[0][bin], 1u);
                    if (top == pre_p) atomicAdd(&hist[1][bin], 1u);
                } else {
                    if (key > sel_d) up_d = min(up_d, key);
                    if (key > sel_p) up_p = min(up_p, key);
                }
            }
        }
    }

    if constexpr (MODE == SURF_UPPER) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            up_d = min(up_d, (unsigned)__shfl_xor((int)up_d, d));
            up_p = min(up_p, (unsigned)__shfl_xor((int)up_p, d));
        }
        if (lane == 0 && up_d != 0xffffffffu) atomicMin(&a.st.upper[obj * 3 + side], up_d);
        if (lane == 0 && up_p != 0xffffffffu) atomicMin(&a.st.upper[obj * 3 + 2], up_p);
    } else {
        if constexpr (MODE == SURF_STATS) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                best = max(best, (unsigned)__shfl_xor((int)best, d));
                sum += __shfl_xor(sum, d);                                     // (a butterfly: every lane adds the same pairs in the same order)
#pragma unroll
                for (int t = 0; t < SURF_MAX_TOL; ++t) tc[t] += (unsigned)__shfl_xor((int)tc[t], d);
            }
            if (lane == 0) {
                if (best) atomicMax(&a.st.maxkey[obj * 2 + side], best);
#pragma unroll
                for (int t = 0; t < SURF_MAX_TOL; ++t)
                    if (tc[t]) atomicAdd(&a.st.tol[obj * SURF_MAX_TOL + t], tc[t]);
                wsum[threadIdx.x >> 6] = sum;
            }
        }
        __syncthreads();
        const unsigned hd = hist[0][threadIdx.x], hp = hist[1][threadIdx.x];
        if (hd) atomicAdd(&a.st.hist[(obj * 3 + side) * 256 + threadIdx.x], hd);
        if (hp) atomicAdd(&a.st.hist[(obj * 3 + 2) * 256 + threadIdx.x], hp);
        if constexpr (MODE == SURF_STATS) {
            if (threadIdx.x == 0) a.st.partial[(obj * 2 + side) * a.slots + slot] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        }
    }
}

__global__ __launch_bounds__(SURF_THREADS) void surf_stats_kernel(const SurfSampleArgs a) {
    __shared__ unsigned hist[2][256];
    __shared__ double wsum[SURF_THREADS / 64];
    surf_sample<SURF_STATS>(a, hist, wsum);
}

__global__ __launch_bounds__(SURF_THREADS) void surf_hist_kernel(const SurfSampleArgs a) {
    __shared__ unsigned hist[2][256];
    surf_sample<SURF_HIST>(a, hist, nullptr);
}

__global__ __launch_bounds__(SURF_THREADS) void surf_upper_kernel(const SurfSampleArgs a) {
    surf_sample<SURF_UPPER>(a, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------------------- pick
struct SurfPickArgs {
    SurfState st;
    double q;                   // percentile / 100
    int K, k0, C, pass;
};

__device__ __forceinline__ unsigned surf_set_size(const SurfState& st, size_t obj, int sel) {
    return sel < 2 ? st.count[obj * 2 + sel] : st.count[obj * 2] + st.count[obj * 2 + 1];       // (2 P <= 2^31 - 2)
}

// rank (0-based) of the lower order statistic of n >= 1 samples and the weight of the upper one: numpy's (n - 1) * q
__device__ __forceinline__ unsigned surf_rank(unsigned n, double q, double& weight) {
    const double pos = (double)(n - 1) * q;
    const double fl = floor(pos);
    weight = pos - fl;
    return (unsigned)fl;
}

__global__ __launch_bounds__(256) void surf_pick_kernel(const SurfPickArgs a) {
    __shared__ unsigned scan[256];
    const unsigned oc = blockIdx.x / 3, sel = blockIdx.x - oc * 3;
    const size_t obj = (size_t)(oc / a.C) * a.K + a.k0 + oc % a.C;
    const size_t s = obj * 3 + sel;
    const unsigned tid = threadIdx.x;
    const unsigned h = a.st.hist[s * 256 + tid];
    a.st.hist[s * 256 + tid] = 0;                                              // (the next pass counts afresh)
    unsigned rank, prefix = 0, below = 0;
    if (a.pass == 0) {
        const unsigned n = surf_set_size(a.st, obj, sel);
        double wgt;
        rank = n ? surf_rank(n, a.q, wgt) : 0;
    } else {
        rank = a.st.rank[s]; prefix = a.st.prefix[s]; below = a.st.below[s];
    }
    scan[tid] = h;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < 256; d <<= 1) {
        const unsigned v = tid >= (unsigned)d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const unsigned incl = scan[tid], excl = incl - h;
    if (a.pass == 0 && tid == 0) a.st.upper[s] = 0xffffffffu;
    if (h && excl <= rank && rank < incl) {                                    // one lane at most; none in an empty set
        a.st.prefix[s] = (prefix << 8) | tid;
        a.st.rank[s] = rank - excl;
        a.st.below[s] = below + excl;
        if (a.pass == 3) a.st.le[s] = below + incl;
    }
}

// ---------------------------------------------------------------------------------------------------------- finish
struct SurfFinishArgs {
    SurfState st;
    long long* surface_count;
    float *directed_hausdorff, *hausdorff, *directed_percentile, *hausdorff_percentile, *mean_surface_distance, *assd, *surface_dice;
    double q;
    long long objects;
    unsigned slots;
    int T, flt;
};

__device__ __forceinline__ double surf_percentile(const SurfState& st, size_t obj, int sel, double q, bool flt) {
    const unsigned n = surf_set_size(st, obj, sel);
    if (!n) return (double)NAN;
    double wgt;
    const unsigned r = surf_rank(n, q, wgt);
    const size_t s = obj * 3 + sel;
    const double lower = surf_distance(st.prefix[s], flt);
    if (wgt == 0.0 || lower == (double)INFINITY) return lower;                // (no 0 * inf, no inf - inf)
    // the statistic of rank r + 1: the same key when more keys <= it remain than the rank needs, else the smallest key above it
    const double upper = st.le[s] >= r + 2 ? lower : surf_distance(st.upper[s], flt);
    return lower + (upper - lower) * wgt;
}

__global__ __launch_bounds__(64) void surf_finish_kernel(const SurfFinishArgs a) {
    const long long o = (long long)blockIdx.x * 64 + threadIdx.x;
    if (o >= a.objects) return;
    const size_t obj = (size_t)o;
    const bool flt = a.flt != 0;
    const unsigned n0 = a.st.count[obj * 2], n1 = a.st.count[obj * 2 + 1];
    const bool none = !n0 && !n1, one = !none && (!n0 || !n1);
    a.surface_count[obj * 2] = n0;
    a.surface_count[obj * 2 + 1] = n1;
    double mean[2], hd[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const unsigned n = side ? n1 : n0;
        double sum = 0.0;
#pragma unroll 1
        for (unsigned j = 0; j < a.slots; ++j) sum += a.st.partial[(obj * 2 + side) * a.slots + j];
        mean[side] = n ? sum / (double)n : (double)NAN;
        hd[side] = n ? surf_distance(a.st.maxkey[obj * 2 + side], flt) : (double)NAN;
        a.directed_hausdorff[obj * 2 + side] = (float)hd[side];
        a.mean_surface_distance[obj * 2 + side] = (float)mean[side];
        a.directed_percentile[obj * 2 + side] = (float)surf_percentile(a.st, obj, side, a.q, flt);
    }
    a.hausdorff[obj] = none ? NAN : one ? INFINITY : (float)fmax(hd[0], hd[1]);
    a.assd[obj] = none ? NAN : one ? INFINITY : (float)((mean[0] + mean[1]) * 0.5);
    a.hausdorff_percentile[obj] = (float)surf_percentile(a.st, obj, 2, a.q, flt);      // (one side empty: every pooled sample is inf)
#pragma unroll 1
    for (int t = 0; t < a.T; ++t)
        a.surface_dice[obj * a.T + t] = none ? NAN : (float)((double)a.st.tol[obj * SURF_MAX_TOL + t] / ((double)n0 + (double)n1));
}

// ---------------------------------------------------------------------------------------------------------- host side
struct SurfPlan {
    long long B, P, objects, seg;
    int chunk, slots;
    long long off_state[10], state_bytes;
    long long off_border, off_dist, off_edt, edt_bytes, bytes, min_bytes;
};

// bytes of the maps of a chunk of c classes; -1: past the transform's position limit or a launch's grid limit.  EVERY grid of
// ptb_surface_metrics is decided here, so that the plan refuses (or shrinks the chunk) and no launch loop does.  The sample kernels take a
// workgroup per map and segment: slots <= P, so maps * slots <= maps * P, which the position limit bounds.  The border kernel takes B
// workgroups per four rows: below B * P.  The pick kernel takes three per object of the chunk, 1.5 * maps: past the limit only for more
// than 2^31 / 3 maps of a single position.
static long long surf_chunk_bytes(const SurfPlan& p, int dims, long long D, long long H, long long W, int c, long long* edt_bytes) {
    const long long maps = 2LL * c * p.B;
    if (maps > MAX_POS / p.P || maps / 2 > SURF_MAX_GRID / 3) return -1;
    int64_t e = 0;
    if (ptb_edt_plan(dims, maps, D, H, W, 0, &e) != PTB_OK) return -1;
    if (edt_bytes) *edt_bytes = e;
    return up16(maps * p.P) + up16(4 * maps * p.P) + e;
}

static int surf_plan(int dims, long long B, long long D, long long H, long long W, int K, long long cap, SurfPlan& p) {
    if ((dims != 2 && dims != 3) || B < 1 || D < 1 || H < 1 || W < 1 || K < 1 || (dims == 2 && D != 1) || cap < 0) return PTB_EINVAL;
    if (D > MAX_POS || H > MAX_POS || W > MAX_POS || H * W > MAX_POS || D * H * W > MAX_POS) return PTB_EUNSUPPORTED;
    p.B = B; p.P = D * H * W;
    if (B > MAX_POS / p.P / 2 || K > MAX_POS / B) return PTB_EUNSUPPORTED;
    p.objects = B * K;
    // the sample kernel's geometry: a function of P alone
    long long seg = std::max<long long>(SURF_SEG_MIN, (p.P + SURF_MAX_SLOTS - 1) / SURF_MAX_SLOTS);
    seg = (seg + 15) & ~15LL;
    p.seg = seg;
    p.slots = (int)((p.P + seg - 1) / seg);
    const long long words[9] = {2, 2, SURF_MAX_TOL, 3, 3, 3, 3, 3, 3 * 256};
    long long o = 0;
    for (int i = 0; i < 9; ++i) { p.off_state[i] = o; o += up16(4 * words[i] * p.objects); }
    p.off_state[9] = o; o += up16(8LL * 2 * p.slots * p.objects);
    p.state_bytes = o;
    long long e = 0;
    const long long one = surf_chunk_bytes(p, dims, D, H, W, 1, &e);
    if (one < 0) return PTB_EUNSUPPORTED;
    p.min_bytes = p.state_bytes + one;
    p.chunk = 0;
    for (int c = std::min(K, SURF_MAX_CHUNK); c >= 1; --c) {
        const long long need = surf_chunk_bytes(p, dims, D, H, W, c, &e);
        if (need >= 0 && p.state_bytes + need <= cap) {
            p.chunk = c; p.edt_bytes = e;
            const long long maps = 2LL * c * B;
            p.off_border = p.state_bytes;
            p.off_dist = p.off_border + up16(maps * p.P);
            p.off_edt = p.off_dist + up16(4 * maps * p.P);
            p.bytes = p.state_bytes + need;
            break;
        }
    }
    return PTB_OK;                                                             // (chunk == 0: the cap is below min_bytes)
}

static SurfState surf_state(const SurfPlan& p, char* ws) {
    SurfState s;
    s.count = reinterpret_cast<unsigned*>(ws + p.off_state[0]);
    s.maxkey = reinterpret_cast<unsigned*>(ws + p.off_state[1]);
    s.tol = reinterpret_cast<unsigned*>(ws + p.off_state[2]);
    s.prefix = reinterpret_cast<unsigned*>(ws + p.off_state[3]);
    s.rank = reinterpret_cast<unsigned*>(ws + p.off_state[4]);
    s.below = reinterpret_cast<unsigned*>(ws + p.off_state[5]);
    s.le = reinterpret_cast<unsigned*>(ws + p.off_state[6]);
    s.upper = reinterpret_cast<unsigned*>(ws + p.off_state[7]);
    s.hist = reinterpret_cast<unsigned*>(ws + p.off_state[8]);
    s.partial = reinterpret_cast<double*>(ws + p.off_state[9]);
    return s;
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_surface_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int K, int64_t max_workspace_bytes, int* classes_per_chunk,
                                int64_t* workspace_bytes, int64_t* min_workspace_bytes, int* partial_sums_per_map) {
    SurfPlan p;
    if (int rc = surf_plan(dims, B, D, H, W, K, max_workspace_bytes, p)) return rc;
    if (min_workspace_bytes) *min_workspace_bytes = p.min_bytes;
    if (partial_sums_per_map) *partial_sums_per_map = p.slots;
    if (p.chunk == 0) return PTB_EINVAL;
    if (classes_per_chunk) *classes_per_chunk = p.chunk;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return PTB_OK;
}

extern "C" int ptb_surface_metrics(const void* pred, int pred_elem_bytes, const void* truth, int truth_elem_bytes, int dims, int64_t B, int64_t D, int64_t H,
                                   int64_t W, const int64_t* class_values, int K, int object_rule, int connectivity, const double* spacing, double percentile,
                                   const double* tolerances, int T, int64_t* surface_count, float* directed_hausdorff, float* hausdorff,
                                   float* directed_percentile, float* hausdorff_percentile, float* mean_surface_distance, float* assd, float* surface_dice,
                                   void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (!pred || !truth || !class_values || !tolerances || !workspace || bad_elem_bytes(pred_elem_bytes) || bad_elem_bytes(truth_elem_bytes)) return PTB_EINVAL;
    if (!surface_count || !directed_hausdorff || !hausdorff || !directed_percentile || !hausdorff_percentile || !mean_surface_distance || !assd || !surface_dice)
        return PTB_EINVAL;
    if (object_rule != PTB_SURFACE_CLASSES && object_rule != PTB_SURFACE_NOT_BACKGROUND) return PTB_EINVAL;
    if (object_rule == PTB_SURFACE_NOT_BACKGROUND && K != 1) return PTB_EINVAL;
    if (T < 1 || T > SURF_MAX_TOL || !(percentile >= 0.0 && percentile <= 100.0)) return PTB_EINVAL;
    const bool full = connectivity == (dims == 2 ? 8 : 26);
    if (!full && connectivity != (dims == 2 ? 4 : 6)) return PTB_EINVAL;
    const bool flt = spacing != nullptr;
    if (flt) {
        for (int k = 0; k < 3; ++k)
            if ((k > 0 || dims == 3) && !(spacing[k] > 0.0 && std::isfinite(spacing[k]))) return PTB_EINVAL;
    }
    for (int t = 0; t < T; ++t)
        if (!(tolerances[t] >= 0.0)) return PTB_EINVAL;
    SurfPlan p;
    if (int rc = surf_plan(dims, B, D, H, W, K, workspace_bytes, p)) return rc;
    if (p.chunk == 0 || !aligned16(workspace)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    const SurfState st = surf_state(p, ws);
    if (hipError_t e = hipMemsetAsync(ws, 0, (size_t)p.state_bytes, s); e != hipSuccess) { set_hip_error(e); return PTB_ELAUNCH; }

    SurfSampleArgs sa{};
    sa.st = st; sa.border = reinterpret_cast<unsigned char*>(ws + p.off_border); sa.dist = reinterpret_cast<unsigned*>(ws + p.off_dist);
    sa.P = p.P; sa.seg = p.seg; sa.B = (unsigned)B; sa.slots = (unsigned)p.slots; sa.K = K; sa.T = T; sa.flt = flt;
    for (int t = 0; t < T; ++t) {
        // unit spacing: the exact squared integer against floor(tol^2); with spacing: the float32 squared distance against tol^2 rounded
        // to float32.  Neither may reach the "no site" value.
        const double sq = tolerances[t] * tolerances[t];
        if (!flt) {
            sa.thr[t] = sq >= (double)(SURF_INT_INF - 1) ? SURF_INT_INF - 1 : (unsigned)std::floor(sq);
        } else {
            float f = sq >= 3.4028234663852886e38 ? 3.4028234663852886e38f : (float)sq;
            std::memcpy(&sa.thr[t], &f, 4);
        }
    }
    const double q = percentile / 100.0;
    const long long rows = D * H;
    const unsigned bpe = (unsigned)((rows + SURF_THREADS / 64 - 1) / (SURF_THREADS / 64));        // (bpe * B <= B * P: the plan's position limit)

    for (int k0 = 0; k0 < K; k0 += p.chunk) {
        const int C = std::min(p.chunk, K - k0);
        const long long maps = 2LL * C * B;
        for (int side = 0; side < 2; ++side) {
            const void* labels = side ? truth : pred;
            const int eb = side ? truth_elem_bytes : pred_elem_bytes;
            SurfBorderArgs ba{};
            ba.labels = labels; ba.border = reinterpret_cast<unsigned char*>(ws + p.off_border); ba.count = st.count;
            ba.P = p.P; ba.B = (unsigned)B; ba.bpe = bpe; ba.D = (int)D; ba.H = (int)H; ba.W = (int)W; ba.K = K; ba.k0 = k0; ba.C = C; ba.side = side;
            ba.full = full; ba.dims3 = dims == 3;
            for (int k = 0; k < C; ++k) {                                      // a value the element type cannot hold occurs nowhere
                const long long v = class_values[k0 + k];
                const bool held = holds(eb, v);
                ba.values[k] = v;
                if (object_rule == PTB_SURFACE_CLASSES) ba.modes[k] = held ? SURF_IN_EQ : SURF_IN_NONE;
                else ba.modes[k] = held ? SURF_IN_NE : SURF_IN_ALL;
            }
            ba.object_mode = object_rule == PTB_SURFACE_CLASSES ? SURF_IN_EQ : ba.modes[0];
            ba.object_value = class_values[0];
            // (the border maps of a chunk start at multiples of P: packed stores need P % 4 == 0, which W % 4 == 0 gives)
            const bool wide = W % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % std::min(4 * eb, 16) == 0;
            with_value<1, 2, 4, 8>(eb, [&](auto e) {
                using T_ = label_t<e()>;
                with_bool(wide, [&](auto w) {
                    hipLaunchKernelGGL((surf_border_kernel<T_, w()>), dim3(bpe * (unsigned)B), dim3(SURF_THREADS), 0, s, ba);
                });
            });
        }
        if (int rc = check_launch()) return rc;
        if (int rc = ptb_edt(ws + p.off_border, 1, dims, maps, D, H, W, PTB_EDT_SITES_EQUAL, 1, spacing, PTB_EDT_SQUARED, ws + p.off_dist,
                             flt ? PTB_EDT_OUT_F32 : PTB_EDT_OUT_I32, ws + p.off_edt, p.edt_bytes, stream))
            return rc;
        sa.k0 = k0; sa.C = C;
        const long long blocks = maps * p.slots;                               // (<= SURF_MAX_GRID: the plan chose the chunk so)
        SurfPickArgs pa{};
        pa.st = st; pa.q = q; pa.K = K; pa.k0 = k0; pa.C = C;
        const unsigned picks = (unsigned)(3LL * C * B);
        for (int pass = 0; pass < 4; ++pass) {
            sa.shift = 24 - 8 * pass;
            if (pass == 0) hipLaunchKernelGGL(surf_stats_kernel, dim3((unsigned)blocks), dim3(SURF_THREADS), 0, s, sa);
            else hipLaunchKernelGGL(surf_hist_kernel, dim3((unsigned)blocks), dim3(SURF_THREADS), 0, s, sa);
            pa.pass = pass;
            hipLaunchKernelGGL(surf_pick_kernel, dim3(picks), dim3(256), 0, s, pa);
        }
        hipLaunchKernelGGL(surf_upper_kernel, dim3((unsigned)blocks), dim3(SURF_THREADS), 0, s, sa);
        if (int rc = check_launch()) return rc;
    }
    SurfFinishArgs fa{};
    fa.st = st; fa.surface_count = reinterpret_cast<long long*>(surface_count); fa.directed_hausdorff = directed_hausdorff; fa.hausdorff = hausdorff;
    fa.directed_percentile = directed_percentile; fa.hausdorff_percentile = hausdorff_percentile; fa.mean_surface_distance = mean_surface_distance;
    fa.assd = assd; fa.surface_dice = surface_dice; fa.q = q; fa.objects = p.objects; fa.slots = (unsigned)p.slots; fa.T = T; fa.flt = flt;
    hipLaunchKernelGGL(surf_finish_kernel, dim3((unsigned)((p.objects + 63) / 64)), dim3(64), 0, s, fa);
    return check_launch();
}
