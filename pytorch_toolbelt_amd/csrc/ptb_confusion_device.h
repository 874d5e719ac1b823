// The counting tail shared by the confusion-matrix kernels (ptb_confusion.hip): a workgroup's private histogram of 32-bit counters in
// LDS, the per-lane fold of equal (target, pred) keys into one LDS add, and the exact flush into the caller's int64 matrix.
//
// A workgroup counts target rows r0 .. r0 + rows - 1 of the K x K matrix: cell (t, p) lives at hist[(t - r0) * K + p], rows * K <=
// CONF_HIST_MAX counters (64 KiB).  K <= 128 is one row block; above that blockIdx.y walks the row blocks and every block reads the maps
// again, dropping the positions of other rows.
// 32-BIT COUNTERS: a workgroup visits at most CONF_MAX_POS_PER_WG + one chunk positions (the host sizes gridDim.x for it), so neither a
// cell nor a lane's run length nor a lane's invalid count can wrap.
// KEYS: a lane keeps ONE open (key, length) pair for the whole kernel -- counting does not care where a position lies, so equal keys fold
// across loads and across trips of the grid-stride loop, and a constant map costs one LDS add per lane.  The range comparison comes
// first; a key is formed from values that passed it only, so no input can index outside the histogram.
#pragma once
#include <type_traits>

#include "ptb_common.h"

namespace ptb {

constexpr int CONF_THREADS = 256;
constexpr int CONF_HIST_MAX = 16384;                       // counters of a workgroup's histogram: 64 KiB of LDS
constexpr int CONF_MAX_K = 256;
constexpr long long CONF_MAX_POS_PER_WG = 1LL << 31;

extern __shared__ __attribute__((aligned(16))) unsigned conf_hist[];

struct ConfLane {
    int key;                // open run: cell index, -1 = not counted (ignored, out of range, another row block)
    unsigned len;
    unsigned invalid;       // positions out of [0, K) that were not ignored
};

// what every instance needs of the matrix: by value in the kernel argument
struct ConfMatrix {
    long long* out;         // [groups, K, K], added to
    long long* invalid;     // one counter
    long long ignore;
    int has_ignore;
    int K, rows;            // rows of a row block
    int g0;                 // first group (sample, or the pooled one) of this launch: group = g0 + blockIdx.z
};

// the 64-bit types compare as 64-bit, everything narrower as int
template <class T>
using conf_wide_t = std::conditional_t<sizeof(T) == 8, long long, int>;

struct ConfBlock {
    int K, r0, rows, cells;
};

__device__ __forceinline__ ConfBlock conf_begin(const ConfMatrix& m, ConfLane& s) {
    ConfBlock b;
    b.K = m.K;
    b.r0 = (int)blockIdx.y * m.rows;
    b.rows = min(m.rows, m.K - b.r0);
    b.cells = b.rows * m.K;
    for (int i = threadIdx.x; i < b.cells; i += CONF_THREADS) conf_hist[i] = 0;
    __syncthreads();
    s.key = -1; s.len = 0; s.invalid = 0;
    return b;
}

template <class WT, class WP>
__device__ __forceinline__ void conf_push(ConfLane& s, const ConfBlock& b, WT t, WP p, bool has_ignore, WT ignore) {
    using UT = std::make_unsigned_t<WT>;
    using UP = std::make_unsigned_t<WP>;
    const bool ign = has_ignore && t == ignore;
    const bool in = (UT)t < (UT)b.K && (UP)p < (UP)b.K;
    s.invalid += (unsigned)(!ign && !in);
    int key = -1;
    if (!ign && in) {
        const unsigned r = (unsigned)((int)t - b.r0);
        if (r < (unsigned)b.rows) key = (int)r * b.K + (int)p;
    }
    if (key != s.key) {
        if (s.key >= 0) atomicAdd(&conf_hist[s.key], s.len);
        s.key = key;
        s.len = 0;
    }
    s.len += 1;
}

// the open runs, then the workgroup's non-zero cells as 64-bit adds into the group's matrix; row block 0 reports the invalid positions
__device__ __forceinline__ void conf_finish(const ConfMatrix& m, const ConfBlock& b, ConfLane& s) {
    if (s.key >= 0) atomicAdd(&conf_hist[s.key], s.len);
    __syncthreads();
    unsigned long long* out = reinterpret_cast<unsigned long long*>(m.out) + ((long long)m.g0 + blockIdx.z) * m.K * m.K + (long long)b.r0 * m.K;
    for (int i = threadIdx.x; i < b.cells; i += CONF_THREADS) {
        const unsigned v = conf_hist[i];
        if (v) atomicAdd(out + i, (unsigned long long)v);
    }
    if (blockIdx.y == 0) {
        unsigned long long inv = s.invalid;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) inv += __shfl_xor(inv, d);
        if ((threadIdx.x & 63) == 0 && inv) atomicAdd(reinterpret_cast<unsigned long long*>(m.invalid), inv);
    }
}

}  // namespace ptb
