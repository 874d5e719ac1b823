// Exclusive scan of 32-bit counts into 64-bit offsets, as launches of their own: reduce tiles upwards, scan the top tile in one
// workgroup, scan tiles downwards with their base.  No workgroup waits for another one inside a launch ("run-length codec").
// Shared by ptb_rle.hip (segment counts -> output offsets) and ptb_components.hip (roots per chunk -> component numbers).
#pragma once
#include "ptb_common.h"

namespace ptb {

constexpr int SCAN_PER = 8, SCAN_TILE = 256 * SCAN_PER;
constexpr int SCAN_MAX_LEVELS = 4;             // SCAN_TILE^4 > 2^36 counts

// Sum of one tile of SCAN_TILE values -> sums[tile].
template <class IN>
__global__ __launch_bounds__(256) void scan_reduce_kernel(const IN* __restrict__ in, long long m, long long* __restrict__ sums) {
    __shared__ long long wsum[4];
    const long long i0 = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_PER;
    long long t = 0;
#pragma unroll
    for (int j = 0; j < SCAN_PER; ++j) t += i0 + j < m ? (long long)in[i0 + j] : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Exclusive scan of one tile, plus base[tile] when given.  `out` may be `in` (every lane reads its SCAN_PER values before it writes them).
template <class IN>
__global__ __launch_bounds__(256) void scan_tile_kernel(const IN* in, long long m, const long long* __restrict__ base, long long* out) {
    __shared__ long long wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i0 = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_PER;
    long long v[SCAN_PER], t = 0;
#pragma unroll
    for (int j = 0; j < SCAN_PER; ++j) {
        v[j] = i0 + j < m ? (long long)in[i0 + j] : 0;
        t += v[j];
    }
    long long inc = t;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long ex = inc - t + (base ? base[blockIdx.x] : 0);
#pragma unroll
    for (int w = 0; w < 3; ++w)
        if (w < wave) ex += wsum[w];
#pragma unroll
    for (int j = 0; j < SCAN_PER; ++j) {
        if (i0 + j < m) out[i0 + j] = ex;
        ex += v[j];
    }
}

// levels and tile counts of a scan over m values: cnt[l] sums at level l, the last level fits one tile
inline int scan_levels(long long m, long long* cnt) {
    int levels = 0;
    while (m > SCAN_TILE) {
        m = (m + SCAN_TILE - 1) / SCAN_TILE;
        cnt[levels++] = m;
    }
    return levels;
}

// out[i] = sum of counts[0 .. i - 1]; sums[l]: cnt[l] 64-bit words of workspace per level
inline void scan_exclusive(const unsigned* counts, long long m, int levels, const long long* cnt, long long* const* sums, long long* out, hipStream_t s) {
    auto tiles = [](long long k) { return dim3((unsigned)((k + SCAN_TILE - 1) / SCAN_TILE)); };
    if (levels == 0) {
        hipLaunchKernelGGL((scan_tile_kernel<unsigned>), dim3(1), dim3(256), 0, s, counts, m, (const long long*)nullptr, out);
        return;
    }
    hipLaunchKernelGGL((scan_reduce_kernel<unsigned>), tiles(m), dim3(256), 0, s, counts, m, sums[0]);
    for (int l = 1; l < levels; ++l)
        hipLaunchKernelGGL((scan_reduce_kernel<long long>), tiles(cnt[l - 1]), dim3(256), 0, s, (const long long*)sums[l - 1], cnt[l - 1], sums[l]);
    const int top = levels - 1;                                                              // (<= SCAN_TILE sums: one workgroup)
    hipLaunchKernelGGL((scan_tile_kernel<long long>), dim3(1), dim3(256), 0, s, (const long long*)sums[top], cnt[top], (const long long*)nullptr, sums[top]);
    for (int l = top - 1; l >= 0; --l)
        hipLaunchKernelGGL((scan_tile_kernel<long long>), tiles(cnt[l]), dim3(256), 0, s, (const long long*)sums[l], cnt[l], (const long long*)sums[l + 1], sums[l]);
    hipLaunchKernelGGL((scan_tile_kernel<unsigned>), tiles(m), dim3(256), 0, s, counts, m, (const long long*)sums[0], out);
}

}  // namespace ptb
