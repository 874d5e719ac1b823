// Run-length encoding and decoding of masks on the device (utils/rle.py of the reference: column-major `start + 1, length` pairs).
//
// ENCODE.  A boundary is a position p of the column-major pixel sequence f[p] = fg[p % H][p / H] with f[p] != f[p - 1] (f[-1] = f[N] = 0);
// an encoding is its boundaries in increasing order, every second one replaced by its distance from the one before.  The mask is read
// where it lies: row-major, each lane four neighbouring columns with one wide load per row, walking RLE_SEG rows down and comparing every
// pixel with the one above it.  The unit of bookkeeping is a SEGMENT: one column x RLE_SEG rows of one (slice, label).  Its boundary
// count lives at counts[((e * W) + x) * S + s] -- column-major order of segments, encodings one after the other -- so that ONE exclusive
// scan over the whole array gives every segment the place of its first boundary in the concatenated output, and an encoding e starts
// at the scanned value of its first segment (an even number: every encoding has an even boundary count).
//   ptb_rle_count:  rle_pass_kernel<.., WRITE = false> (counts) -> the scan, launches of its own (reduce tiles upwards, scan the top tile in
//                   one workgroup, scan tiles downwards with their base: no workgroup waits for another one inside a launch) ->
//                   rle_enc_offsets_kernel ([E + 1] 64-bit offsets for the caller's one D2H read).
//   ptb_rle_write:  rle_pass_kernel<.., WRITE = true> (the same walk; position + 1 of every boundary at its segment's offset) ->
//                   rle_lengths_kernel (odd entries: minus the entry before, 16 bytes per lane).
// No atomics, no transposed / boolean / per-label copy of the mask; the result is deterministic.
//
// DECODE.  Runs (any order, overlapping) are filled as ones into a linear column-major [W, H] byte buffer -- coalesced stores however
// long a vertical run is -- which a second kernel transposes into the row-major mask through 64 x 64 LDS tiles.  Runs are clamped to
// 0..N in the kernel, so runs that were never validated on the host store nothing out of bounds.
#include <algorithm>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_scan_device.h"

namespace ptb {

constexpr int RLE_SEG = 32;                    // rows of a segment
constexpr int RLE_LANES = 64;                  // lanes of a workgroup along x, four columns each
constexpr int RLE_COLS = 4 * RLE_LANES;        // columns of a work item
constexpr int RLE_WY = 4;                      // segments (waves) of a workgroup along y
constexpr int RLE_ROWS = RLE_SEG * RLE_WY;
constexpr int RLE_CHUNK = 8;                   // rows whose loads are in flight together
constexpr int RLE_MAX_LABELS = 16;             // labels of one launch (by-value kernel argument)
constexpr long long RLE_MAX_COUNTS = 1LL << 36;
constexpr long long RLE_MAX_PIXELS = 0x7fffffffLL - 1;
constexpr int FILL_SHORT = 16;                 // runs up to this length are stored by the lane that read them
constexpr int FILL_CHUNK = 16384;              // bytes of a long run that one wave stores before the next z-slice of the grid takes over

struct RleLabels {
    long long v[RLE_MAX_LABELS];
};

struct RleArgs {
    const void* mask;
    const unsigned* counts_in;      // WRITE: unused
    unsigned* counts;               // COUNT: out
    const long long* offsets;       // WRITE: in
    long long* out;                 // WRITE: out
    long long HW;
    int H, W, S, colblocks;
    int b0, k0, kc, Ktot;           // blockIdx.y = (slice - b0) * kc + (label - k0); encoding = slice * Ktot + label
    int any;                        // labels = None: foreground is mask != 0
    RleLabels labels;
};

template <class T, bool VEC>
__device__ __forceinline__ unsigned fg_bits(const T* row, int x, int W, bool any, bool rep, T c) {
    T v[4];
    if constexpr (VEC) {
        constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        __builtin_memcpy(v, __builtin_assume_aligned(row + x, A), sizeof(v));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = row[min(x + j, W - 1)];      // (columns past W are masked out by the caller)
    }
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) bits |= (unsigned)(any ? v[j] != (T)0 : (rep && v[j] == c)) << j;
    return bits;
}

// One lane: columns x .. x + 3, rows y0 .. y1 - 1 of one (slice, label).  WRITE = false: the number of boundaries of each of the four
// segments; WRITE = true: position + 1 of every boundary, from the segment's scanned offset on.
template <class T, bool VEC, bool WRITE>
__global__ __launch_bounds__(RLE_LANES * RLE_WY) void rle_pass_kernel(const RleArgs a) {
    const int cb = blockIdx.x % a.colblocks, rb = blockIdx.x / a.colblocks;
    const int x = cb * RLE_COLS + (int)threadIdx.x * 4, s = rb * RLE_WY + (int)threadIdx.y, y0 = s * RLE_SEG;
    if (x >= a.W || y0 >= a.H) return;
    const int y1 = min(y0 + RLE_SEG, a.H);
    const int bi = blockIdx.y / a.kc, kj = blockIdx.y - bi * a.kc;
    long long label = 0;
#pragma unroll
    for (int j = 0; j < RLE_MAX_LABELS; ++j)
        if (j == kj) label = a.labels.v[j];
    const bool any = a.any != 0;
    const T c = (T)label;
    const bool rep = (long long)c == label;                    // a label outside T's range occurs nowhere
    const T* m = reinterpret_cast<const T*>(a.mask) + (long long)(a.b0 + bi) * a.HW;
    const long long e = (long long)(a.b0 + bi) * a.Ktot + a.k0 + kj;
    const unsigned valid = x + 4 <= a.W ? 15u : (1u << (a.W - x)) - 1u;

    unsigned prev = 0;
    if (y0 > 0) {
        prev = fg_bits<T, VEC>(m + (long long)(y0 - 1) * a.W, x, a.W, any, rep, c);
    } else {                                                    // row 0 follows row H - 1 of the column before; p = 0 follows background
        const T* last = m + (long long)(a.H - 1) * a.W;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xp = x + j - 1;
            if (xp >= 0) {
                const T v = last[min(xp, a.W - 1)];
                prev |= (unsigned)(any ? v != (T)0 : (rep && v == c)) << j;
            }
        }
    }

    unsigned cnt[4] = {0, 0, 0, 0};
    long long off[4] = {0, 0, 0, 0};
    const long long seg0 = (e * a.W + x) * a.S + s;             // segment of column x; column x + j is j * S further
    if constexpr (WRITE) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((valid >> j) & 1u) off[j] = a.offsets[seg0 + (long long)j * a.S];
    }

#pragma unroll 1
    for (int y = y0; y < y1; y += RLE_CHUNK) {
        unsigned rows[RLE_CHUNK];
#pragma unroll
        for (int r = 0; r < RLE_CHUNK; ++r)                      // (rows past the segment load its last row again; they are not used)
            rows[r] = fg_bits<T, VEC>(m + (long long)min(y + r, y1 - 1) * a.W, x, a.W, any, rep, c);
#pragma unroll
        for (int r = 0; r < RLE_CHUNK; ++r) {
            if (y + r < y1) {
                const unsigned diff = (rows[r] ^ prev) & valid;
                prev = rows[r];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (WRITE) {
                        if ((diff >> j) & 1u) a.out[off[j]++] = (long long)(x + j) * a.H + (y + r) + 1;
                    } else {
                        cnt[j] += (diff >> j) & 1u;
                    }
                }
            }
        }
    }
    if (y1 == a.H && x + 4 >= a.W) {                            // a foreground last pixel closes its run at p = N
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x + j == a.W - 1 && ((prev >> j) & 1u)) {
                if constexpr (WRITE) a.out[off[j]++] = a.HW + 1;
                else cnt[j] += 1;
            }
        }
    }
    if constexpr (!WRITE) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((valid >> j) & 1u) a.counts[seg0 + (long long)j * a.S] = cnt[j];
    }
}

// enc[e] = first output entry of encoding e; enc[E] = the total
__global__ __launch_bounds__(256) void rle_enc_offsets_kernel(const long long* __restrict__ offsets, const unsigned* __restrict__ counts, long long n,
                                                              long long per_enc, long long E, long long* __restrict__ enc) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < E) enc[e] = offsets[e * per_enc];
    else if (e == E) enc[E] = offsets[n - 1] + counts[n - 1];
}

// out[2 i + 1] -= out[2 i]: an end position becomes a length
__global__ __launch_bounds__(256) void rle_lengths_kernel(long long* out, long long pairs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= pairs) return;
    const longlong2 v = *reinterpret_cast<const longlong2*>(out + 2 * i);
    out[2 * i + 1] = v.y - v.x;
}

// ---------------------------------------------------------------------------------------------------------- decode
// A wave takes 64 runs.  Short runs are stored by their own lane; a long run is broadcast and stored by the whole wave, 16 bytes per
// lane where the run covers an aligned 16-byte group; its FILL_CHUNK-byte chunks go round robin over gridDim.y.  Overlapping runs store
// the same ones: whichever store lands last, the byte is 1.
__global__ __launch_bounds__(256) void rle_fill_kernel(const long long* __restrict__ runs, long long pairs, long long N, unsigned char* __restrict__ lin) {
    const int lane = threadIdx.x & 63;
    const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + lane;
    const int z = blockIdx.y, Z = gridDim.y;
    long long lo = 0, hi = 0;
    if (r < pairs) {
        const longlong2 p = *reinterpret_cast<const longlong2*>(runs + 2 * r);
        lo = min(max(p.x, 1LL), N + 1) - 1;                    // clamped: nothing is stored outside 0 .. N - 1
        hi = lo + min(max(p.y, 0LL), N - lo);
    }
    const long long len = hi - lo;
    if (z == 0 && len <= FILL_SHORT)
        for (long long q = lo; q < hi; ++q) lin[q] = 1;
    unsigned long long todo = __ballot(len > FILL_SHORT);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const long long a = __shfl(lo, src), b = __shfl(hi, src), a16 = a & ~15LL;
        for (long long c0 = a16 + (long long)z * FILL_CHUNK; c0 < b; c0 += (long long)Z * FILL_CHUNK) {
            const long long c1 = min(c0 + FILL_CHUNK, b);
            for (long long q = c0 + lane * 16; q < c1; q += 64 * 16) {
                if (q >= a && q + 16 <= b) {
                    *reinterpret_cast<uint4*>(lin + q) = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
                } else {
                    const long long q1 = min(q + 16, b);
                    for (long long t = max(q, a); t < q1; ++t) lin[t] = 1;
                }
            }
        }
    }
}

// out[y][x] = lin[x * H + y] through a 64 x 64 tile (rows padded to 68 bytes: the transposed byte reads of a wave hit 64 banks)
__global__ __launch_bounds__(256) void rle_transpose_kernel(const unsigned char* __restrict__ lin, unsigned char* __restrict__ out, int H, int W, int tiles_x) {
    __shared__ unsigned char t[64][68];
    const int x0 = (blockIdx.x % tiles_x) * 64, y0 = (blockIdx.x / tiles_x) * 64;
    const int tx = threadIdx.x, ty = threadIdx.y;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int xx = x0 + ty + 4 * i, yy = y0 + tx;
        if (xx < W && yy < H) t[ty + 4 * i][tx] = lin[(long long)xx * H + yy];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int yy = y0 + ty + 4 * i, xx = x0 + tx;
        if (yy < H && xx < W) out[(long long)yy * W + xx] = t[tx][ty + 4 * i];
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
struct RlePlan {
    long long E, S, n;
    int levels;
    long long cnt[SCAN_MAX_LEVELS];
    long long off_enc, off_offsets, off_sums[SCAN_MAX_LEVELS], off_counts, bytes;
};

static int make_plan(int B, int K, int H, int W, RlePlan& p) {
    if (B < 1 || K < 0 || H < 1 || W < 1) return PTB_EINVAL;
    if ((long long)H * W > RLE_MAX_PIXELS) return PTB_EUNSUPPORTED;
    p.E = (long long)B * std::max(K, 1);
    p.S = (H + RLE_SEG - 1) / RLE_SEG;
    const long long per = (long long)W * p.S;
    if (per > RLE_MAX_COUNTS / p.E) return PTB_EUNSUPPORTED;
    p.n = p.E * per;
    p.levels = scan_levels(p.n, p.cnt);
    long long o = 0;
    p.off_enc = o; o += up16(8 * (p.E + 1));
    p.off_offsets = o; o += up16(8 * p.n);
    for (int l = 0; l < p.levels; ++l) { p.off_sums[l] = o; o += up16(8 * p.cnt[l]); }
    p.off_counts = o; o += up16(4 * p.n);
    p.bytes = o;
    return PTB_OK;
}

static int vec_bytes(int elem_bytes) { return std::min(4 * elem_bytes, 16); }

template <bool WRITE>
static int launch_pass(const void* mask, int elem_bytes, int B, int H, int W, const int64_t* labels, int K, const RlePlan& p, char* ws, long long* out,
                       hipStream_t s) {
    RleArgs a{};
    a.mask = mask; a.counts = reinterpret_cast<unsigned*>(ws + p.off_counts); a.offsets = reinterpret_cast<const long long*>(ws + p.off_offsets);
    a.out = out; a.HW = (long long)H * W; a.H = H; a.W = W; a.S = (int)p.S;
    a.colblocks = (W + RLE_COLS - 1) / RLE_COLS;
    a.Ktot = std::max(K, 1); a.any = K == 0;
    const long long blocks = (long long)a.colblocks * ((H + RLE_ROWS - 1) / RLE_ROWS);    // <= N / 128 + W / 256 + H / 128 + 1 < 2^31
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(mask) % vec_bytes(elem_bytes)) == 0;
    const dim3 block(RLE_LANES, RLE_WY);
    for (int k0 = 0; k0 < a.Ktot; k0 += RLE_MAX_LABELS) {
        a.k0 = k0; a.kc = std::min(RLE_MAX_LABELS, a.Ktot - k0);
        for (int j = 0; j < RLE_MAX_LABELS; ++j) a.labels.v[j] = K > 0 && j < a.kc ? labels[k0 + j] : 0;
        const int per_launch = 65535 / a.kc;                      // gridDim.y carries (slice, label)
        for (int b0 = 0; b0 < B; b0 += per_launch) {
            a.b0 = b0;
            const dim3 grid((unsigned)blocks, (unsigned)(std::min(per_launch, B - b0) * a.kc));
            with_value<1, 2, 4, 8>(elem_bytes, [&](auto eb) {
                using T = std::conditional_t<eb() == 1, unsigned char, std::conditional_t<eb() == 2, short, std::conditional_t<eb() == 4, int, long long>>>;
                with_bool(vec, [&](auto v) { hipLaunchKernelGGL((rle_pass_kernel<T, v(), WRITE>), grid, block, 0, s, a); });
            });
            if (int rc = check_launch()) return rc;
        }
    }
    return PTB_OK;
}

static bool bad_labels(int elem_bytes, const int64_t* labels, int K) {
    return bad_elem_bytes(elem_bytes) || (K > 0 && !labels);
}

}  // namespace ptb

using namespace ptb;

extern "C" int64_t ptb_rle_workspace_bytes(int B, int K, int H, int W) {
    RlePlan p;
    if (int rc = make_plan(B, K, H, W, p)) return rc;
    return p.bytes;
}

extern "C" int ptb_rle_count(const void* mask, int elem_bytes, int B, int H, int W, const int64_t* labels, int K, void* workspace,
                             int64_t workspace_bytes, ptb_stream_t stream) {
    if (!mask || !workspace || bad_labels(elem_bytes, labels, K)) return PTB_EINVAL;
    RlePlan p;
    if (int rc = make_plan(B, K, H, W, p)) return rc;
    if (workspace_bytes < p.bytes || !aligned16(workspace)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = launch_pass<false>(mask, elem_bytes, B, H, W, labels, K, p, ws, nullptr, s)) return rc;

    const unsigned* counts = reinterpret_cast<const unsigned*>(ws + p.off_counts);
    long long* offsets = reinterpret_cast<long long*>(ws + p.off_offsets);
    long long* sums[SCAN_MAX_LEVELS] = {};
    for (int l = 0; l < p.levels; ++l) sums[l] = reinterpret_cast<long long*>(ws + p.off_sums[l]);
    scan_exclusive(counts, p.n, p.levels, p.cnt, sums, offsets, s);                          // (ptb_scan_device.h)
    hipLaunchKernelGGL(rle_enc_offsets_kernel, dim3((unsigned)((p.E + 256) / 256)), dim3(256), 0, s, (const long long*)offsets, counts, p.n,
                       (long long)W * p.S, p.E, reinterpret_cast<long long*>(ws + p.off_enc));
    return check_launch();
}

extern "C" int ptb_rle_write(const void* mask, int elem_bytes, int B, int H, int W, const int64_t* labels, int K, void* workspace,
                             int64_t workspace_bytes, int64_t* out, int64_t total, ptb_stream_t stream) {
    if (!mask || !workspace || bad_labels(elem_bytes, labels, K) || total < 0 || (total & 1) || (total > 0 && !out)) return PTB_EINVAL;
    RlePlan p;
    if (int rc = make_plan(B, K, H, W, p)) return rc;
    if (workspace_bytes < p.bytes || !aligned16(workspace) || !aligned16(out)) return PTB_EINVAL;
    if (total / 2 > 0x7fffffffLL * 256) return PTB_EUNSUPPORTED;
    if (total == 0) return PTB_OK;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = launch_pass<true>(mask, elem_bytes, B, H, W, labels, K, p, reinterpret_cast<char*>(workspace), reinterpret_cast<long long*>(out), s)) return rc;
    const long long pairs = total / 2;
    hipLaunchKernelGGL(rle_lengths_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, reinterpret_cast<long long*>(out), pairs);
    return check_launch();
}

extern "C" int64_t ptb_rle_decode_workspace_bytes(int H, int W) {
    if (H < 1 || W < 1) return PTB_EINVAL;
    if ((long long)H * W > RLE_MAX_PIXELS) return PTB_EUNSUPPORTED;
    return up16((long long)H * W);
}

extern "C" int ptb_rle_decode(const int64_t* runs, int64_t pairs, int H, int W, uint8_t* mask, void* workspace, int64_t workspace_bytes,
                              ptb_stream_t stream) {
    if (!mask || !workspace || pairs < 0 || (pairs > 0 && !runs) || H < 1 || W < 1) return PTB_EINVAL;
    if ((long long)H * W > RLE_MAX_PIXELS) return PTB_EUNSUPPORTED;
    const long long N = (long long)H * W;
    if (workspace_bytes < up16(N) || !aligned16(workspace) || !aligned16(runs)) return PTB_EINVAL;
    const long long run_blocks = (pairs + 255) / 256;
    if (run_blocks > 0x7fffffffLL) return PTB_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    unsigned char* lin = reinterpret_cast<unsigned char*>(workspace);
    if (hipError_t e = hipMemsetAsync(lin, 0, (size_t)N, s); e != hipSuccess) { set_hip_error(e); return PTB_ELAUNCH; }
    if (pairs > 0) {
        // few runs: their long ones are spread over up to 64 z-slices, towards some 2048 workgroups in all
        const int Z = (int)std::min<long long>(64, std::max<long long>(1, 2048 / run_blocks));
        hipLaunchKernelGGL(rle_fill_kernel, dim3((unsigned)run_blocks, (unsigned)Z), dim3(256), 0, s, reinterpret_cast<const long long*>(runs), (long long)pairs, N, lin);
    }
    const int tiles_x = (W + 63) / 64;
    const long long tiles = (long long)tiles_x * ((H + 63) / 64);
    hipLaunchKernelGGL(rle_transpose_kernel, dim3((unsigned)tiles), dim3(64, 4), 0, s, (const unsigned char*)lin, mask, H, W, tiles_x);
    return check_launch();
}
