// Connected-component labelling of label maps on the device (utils/components.py; the reference has no counterpart).  Two neighbouring
// positions belong to one component iff they hold the same value and that value is not the background; neighbourhoods: 4 | 8 (2-D),
// 6 | 26 (3-D).  Block-based union-find (Komura; Playne & Hawick), every phase a launch of its own:
//   1. cc_local_kernel    a workgroup loads one tile (2-D: 16 x 64, 3-D: 4 x 8 x 32 positions, four neighbouring x per lane, one wide
//                         load) and labels it in LDS: a union-find whose parent is always a smaller tile-local index.  It writes
//                         parent[p] = global linear index of p's tile-local root, -1 at background.
//   2. cc_seam_kernel     positions on tile borders are united with their equal-valued backward neighbours in OTHER tiles: the
//                         lock-free atomicMin loop on the parent map.  The smaller root always wins, so at the end a component's root
//                         is its minimum linear index = its first position in row-major order, whatever order the atomics arrived in.
//   3. cc_flatten_kernel  every position follows its parents to the root and stores it (into the caller's cc map, or the second
//                         workspace map of remove_small); the roots of each chunk of 1024 consecutive positions are counted.
//   4. scan (ptb_scan_device.h, launches of its own) -> cc_rank_kernel (every root: its rank in row-major order, minus the scan value at
//      the start of its stack entry, + 1; count per entry) -> cc_relabel_kernel (cc = rank of the root).
//   remove_small: 1-3, then cc_area_kernel (areas at the root index) and cc_rewrite_kernel.   stats: cc_stats_*_kernel.
//
// WHY STALE READS ARE HARMLESS.  Within a launch the per-CU L1s and per-XCD L2s are not coherent, and no workgroup ever waits for
// another one: ordering between phases comes from launch boundaries only.  Inside the seam kernel every access to the parent map is an
// agent-scope atomic (atomicMin whose returned value is acted on; relaxed agent-scope loads), and correctness rests on ONE invariant:
//     a cell's parent only ever DECREASES, and every value it has ever held is a member of the cell's own component.
// It holds at the start (tile-local roots), and every write is atomicMin(&parent[a], b) with a and b in one component (two equal-valued
// neighbours, or a cell and something reached from it by parent links).  A stale or old value of a cell is therefore still a member of
// its component that lies at or above the current value: following it costs extra steps, never a wrong union.  A union ends only when
// atomicMin RETURNS a == the cell it was applied to, i.e. a was a root at the instant it was linked below b, or when both finds reach
// the same cell; otherwise it goes on from the returned (smaller) value.  After the last seam union has completed, the equal-valued
// neighbours of every seam share a root, and a root is the minimum of its component because links only point downwards.
// EVERY LOOP IS BOUNDED.  Parent chasing strictly decreases the index (a step that does not is treated as a failure), and every find /
// union carries a hard step cap on top.  A lane that exceeds it stops and raises err[entry]: that entry's count becomes -1 and
// remove_small leaves the entry as it was.  A logic error ends as a failed test, not as a hung device.
// AGGREGATION.  Areas and boxes are folded before anything touches global memory: runs of equal keys across the wave (cc_seg_len), then
// all keys of the workgroup's chunk in an LDS hash table, then ONE atomic per (workgroup, component) and statistic -- a map that is one
// component, or one that is mostly one component cut into short runs by noise, does not serialise on a single address.  All sums are
// integers: exact and independent of arrival order.
#include <algorithm>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_scan_device.h"

namespace ptb {

constexpr int CC_THREADS = 256;
constexpr int CC_TILE = 1024;                   // positions of a tile (phases 1, 2) and of a chunk (phases 3, 4; statistics)
constexpr int CC_LOCAL_CAP = 8 * CC_TILE;       // steps of one union inside a tile: both ends only move down, fewer than CC_TILE links each
constexpr int CC_CAP = 1 << 24;                 // steps of one union / find on the global map (its links are tile-local roots only)
constexpr int CC_SEAM_BLOCKS = 1 << 16;

template <bool DIM3>
struct CcTile {
    static constexpr int TZ = DIM3 ? 4 : 1, TY = DIM3 ? 8 : 16, TX = DIM3 ? 32 : 64;
    static_assert(TZ * TY * TX == CC_TILE && TX % 4 == 0, "a tile is CC_TILE positions, four per lane along x");
};

struct CcArgs {
    const void* labels;
    int* parent;
    int* err;                   // [B]: a step cap was exceeded in this entry
    long long bg;
    unsigned n, total;          // positions per entry, per call
    int D, H, W;
    int tz, ty, tx;             // tiles per entry
    int has_bg;
};

// f(dz, dy, dx) for every neighbour offset that precedes (0, 0, 0) in row-major order: faces only, or faces + edges + corners
template <bool DIM3, bool FULL, class F>
__device__ __forceinline__ void cc_backward(F&& f) {
#pragma unroll
    for (int dz = DIM3 ? -1 : 0; dz <= 0; ++dz) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const bool before = dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
                const bool face = (dz != 0) + (dy != 0) + (dx != 0) == 1;
                if (before && (FULL || face)) f(dz, dy, dx);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- union-find
// LDS form (workgroup scope) and global form (agent scope) of the same two loops.  Both return -1 / false when a step does not decrease
// the index or the cap is exceeded.
template <bool GLOBAL>
__device__ __forceinline__ int cc_load(const int* p) {
    if constexpr (GLOBAL) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool GLOBAL>
__device__ __forceinline__ int cc_min(int* p, int v) {
    if constexpr (GLOBAL) return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool GLOBAL>
__device__ __forceinline__ int cc_find(const int* L, int x, int& steps) {
    constexpr int CAP = GLOBAL ? CC_CAP : CC_LOCAL_CAP;
    for (; steps < CAP; ++steps) {
        const int p = cc_load<GLOBAL>(L + x);
        if (p == x) return x;
        if (p > x || p < 0) return -1;
        x = p;
    }
    return -1;
}

// unite the components of a and b; returns their common root, -1 on failure
template <bool GLOBAL>
__device__ __forceinline__ int cc_union(int* L, int a, int b) {
    constexpr int CAP = GLOBAL ? CC_CAP : CC_LOCAL_CAP;
    int steps = 0;
    for (; steps < CAP; ++steps) {
        a = cc_find<GLOBAL>(L, a, steps);
        b = cc_find<GLOBAL>(L, b, steps);
        if (a < 0 || b < 0) return -1;
        if (a == b) return a;
        if (a < b) { const int t = a; a = b; b = t; }           // a: the larger root
        const int old = cc_min<GLOBAL>(L + a, b);
        if (old == a) return b;                                   // a was a root when it was linked below b
        if (old > a || old < 0) return -1;
        a = old;                                                  // a had been linked meanwhile: go on from where it points
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------------------- phase 1
template <class T, bool WIDE, bool FULL, bool DIM3>
__global__ __launch_bounds__(CC_THREADS) void cc_local_kernel(const CcArgs a) {
    constexpr int TZ = CcTile<DIM3>::TZ, TY = CcTile<DIM3>::TY, TX = CcTile<DIM3>::TX, LX = TX / 4;
    __shared__ T sv[CC_TILE];
    __shared__ int par[CC_TILE];
    unsigned t = blockIdx.x;
    const int bx = (int)(t % (unsigned)a.tx); t /= (unsigned)a.tx;
    const int by = (int)(t % (unsigned)a.ty); t /= (unsigned)a.ty;
    const int bz = (int)(t % (unsigned)a.tz);
    const unsigned e = t / (unsigned)a.tz;
    const int lt = (int)threadIdx.x;
    const int lx = (lt % LX) * 4, ly = (lt / LX) % TY, lz = lt / (LX * TY), li = lt * 4;      // li = (lz * TY + ly) * TX + lx
    const int x = bx * TX + lx, y = by * TY + ly, z = bz * TZ + lz;
    const bool row_in = y < a.H && z < a.D;
    const unsigned g0 = e * a.n + ((unsigned)z * (unsigned)a.H + (unsigned)y) * (unsigned)a.W + (unsigned)x;   // (used only when in range)
    const T* lab = reinterpret_cast<const T*>(a.labels);
    const T bg = (T)a.bg;
    const bool has_bg = a.has_bg != 0 && (long long)bg == a.bg;               // a background outside the type occurs nowhere

    T v[4] = {(T)0, (T)0, (T)0, (T)0};
    if (row_in) {
        if constexpr (WIDE) {                                                  // W % 4 == 0 and an aligned base: x < W means x + 3 < W
            constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
            if (x < a.W) __builtin_memcpy(v, __builtin_assume_aligned(lab + g0, A), sizeof(v));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < a.W) v[j] = lab[g0 + j];
        }
    }
    bool fg[4];
    int p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        fg[j] = row_in && x + j < a.W && !(has_bg && v[j] == bg);
        const int jp = j > 0 ? j - 1 : 0;
        p[j] = !fg[j] ? -1 : (j > 0 && fg[jp] && v[j] == v[jp]) ? p[jp] : li + j;      // the lane's own runs are linked in registers
        sv[li + j] = v[j];
        par[li + j] = p[j];
    }
    __syncthreads();

    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cc_backward<DIM3, FULL>([&](int dz, int dy, int dx) {
            if (dz == 0 && dy == 0 && j > 0) return;                           // (the left neighbour inside the lane: linked above)
            const int nx = lx + j + dx, ny = ly + dy, nz = lz + dz;
            if (!fg[j] || nx < 0 || nx >= TX || ny < 0 || ny >= TY || nz < 0) return;     // other tiles: phase 2
            const int q = (nz * TY + ny) * TX + nx;
            if (cc_load<false>(par + q) >= 0 && sv[q] == v[j]) bad |= cc_union<false>(par, li + j, q) < 0;
        });
    }
    __syncthreads();

    int out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        out[j] = -1;
        if (fg[j]) {
            int steps = 0;
            const int r = cc_find<false>(par, li + j, steps);
            bad |= r < 0;
            const int rr = r < 0 ? li + j : r;
            const int rx = rr % TX, ry = (rr / TX) % TY, rz = rr / (TX * TY);
            out[j] = (int)(e * a.n + ((unsigned)(bz * TZ + rz) * (unsigned)a.H + (unsigned)(by * TY + ry)) * (unsigned)a.W + (unsigned)(bx * TX + rx));
        }
    }
    if (row_in) {
        if constexpr (WIDE) {
            if (x < a.W) *reinterpret_cast<int4*>(a.parent + g0) = make_int4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < a.W) a.parent[g0 + j] = out[j];
        }
    }
    if (bad) a.err[e] = 1;
}

// ---------------------------------------------------------------------------------------------------------- phase 2
template <class T, bool FULL, bool DIM3>
__global__ __launch_bounds__(CC_THREADS) void cc_seam_kernel(const CcArgs a) {
    constexpr int TZ = CcTile<DIM3>::TZ, TY = CcTile<DIM3>::TY, TX = CcTile<DIM3>::TX;
    const T* lab = reinterpret_cast<const T*>(a.labels);
    const T bg = (T)a.bg;
    const bool has_bg = a.has_bg != 0 && (long long)bg == a.bg;
    const unsigned W = (unsigned)a.W, H = (unsigned)a.H;
#pragma unroll 1
    for (unsigned long long pp = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x; pp < a.total; pp += (unsigned long long)gridDim.x * CC_THREADS) {
        const unsigned p = (unsigned)pp, e = p / a.n, r = p - e * a.n;
        const unsigned row = r / W;
        const int x = (int)(r - row * W), z = (int)(row / H), y = (int)(row - (unsigned)z * H);
        const int mx = x % TX, my = y % TY;
        if (!(mx == 0 || mx == TX - 1 || my == 0 || my == TY - 1 || (DIM3 && z % TZ == 0))) continue;
        const T v = lab[p];
        if (has_bg && v == bg) continue;
        bool bad = false;
        cc_backward<DIM3, FULL>([&](int dz, int dy, int dx) {
            const int nx = x + dx, ny = y + dy, nz = z + dz;
            if (nx < 0 || nx >= a.W || ny < 0 || ny >= a.H || nz < 0) return;
            if (nx / TX == x / TX && ny / TY == y / TY && nz / TZ == z / TZ) return;          // the same tile: phase 1
            const unsigned q = (unsigned)((long long)p + ((long long)dz * a.H + dy) * a.W + dx);
            if (lab[q] != v) return;
            // the first hops of both ends (their tile-local roots) are pulled down to the common root afterwards: the next union that
            // starts in either tile finds it in two steps
            const int la = cc_load<true>(a.parent + p), lb = cc_load<true>(a.parent + q);
            if (la < 0 || lb < 0 || la > (int)p || lb > (int)q) { bad = true; return; }
            const int root = cc_union<true>(a.parent, la, lb);
            if (root < 0) { bad = true; return; }
            if (root < la && cc_load<true>(a.parent + la) > root) cc_min<true>(a.parent + la, root);      // (a load first: the other border
            if (root < lb && cc_load<true>(a.parent + lb) > root) cc_min<true>(a.parent + lb, root);      //  positions of the tile find it done)
        });
        if (bad) a.err[e] = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------- chunks
// Phases 3 and 4 and the statistics walk chunks of CC_TILE consecutive positions of one entry; position j * 256 + thread of the chunk
// belongs to the lane in trip j, so a wave row is 64 consecutive positions.
struct CcChunkArgs {
    const int* parent;          // flatten: in; rank: out (rank at the root's position); area: the areas (unsigned)
    int* root;                  // flatten: out; rank / relabel: the cc map
    int* err;
    unsigned* counts;           // [chunks + 1]
    const long long* excl;      // [chunks + 1]
    long long* count;           // [B]
    unsigned n, cpe;            // positions, chunks per entry
};

struct CcChunk {
    unsigned e, base, valid;    // entry, first position, positions
};

__device__ __forceinline__ CcChunk cc_chunk(unsigned n, unsigned cpe) {
    CcChunk c;
    c.e = blockIdx.x / cpe;
    const unsigned k = blockIdx.x - c.e * cpe;
    c.base = c.e * n + k * CC_TILE;
    c.valid = min((unsigned)CC_TILE, n - k * CC_TILE);
    return c;
}

// A wave row of keys (64 consecutive positions; key < 0: nothing there).  For the first lane of every run of equal keys: the run's
// length.
__device__ __forceinline__ int cc_seg_len(int key, int lane, bool& leader) {
    const int prev = __shfl_up(key, 1);
    leader = lane == 0 || prev != key;
    const unsigned long long m = __ballot(leader);
    const unsigned long long above = lane == 63 ? 0ull : m >> (lane + 1);
    return above ? __ffsll((long long)above) : 64 - lane;
}

__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const CcChunkArgs a) {
    __shared__ unsigned wcount[4];
    const CcChunk c = cc_chunk(a.n, a.cpe);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned roots = 0;
    bool bad = false;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const unsigned i = (unsigned)j * CC_THREADS + threadIdx.x;
        const bool in = i < c.valid;
        const int q = in ? a.parent[c.base + i] : -1;
        // neighbouring lanes mostly share their first hop (a row run of a tile): the first lane of each run of equal hops chases
        bool leader;
        (void)cc_seg_len(q, lane, leader);
        int r = -1;
        if (leader && q >= 0) {
            int steps = 0;
            r = cc_find<true>(a.parent, q, steps);               // (the seam launch is complete: nothing writes the map any more)
            bad |= r < 0;
        }
        const unsigned long long m = __ballot(leader);
        const int src = 63 - __clzll((long long)(m & (~0ull >> (63 - lane))));
        r = __shfl(r, src);
        if (in) a.root[c.base + i] = q < 0 ? -1 : r;
        roots += (unsigned)__popcll(__ballot(in && q >= 0 && r == (int)(c.base + i)));
    }
    if (bad) a.err[c.e] = 1;
    if (a.counts) {
        if (lane == 0) wcount[wave] = roots;
        __syncthreads();
        if (threadIdx.x == 0) {
            a.counts[blockIdx.x] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
            if (blockIdx.x == 0) a.counts[gridDim.x] = 0;        // (the scan's last value is then the total)
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- phase 4
__global__ __launch_bounds__(CC_THREADS) void cc_rank_kernel(const CcChunkArgs a, int* rank) {
    __shared__ unsigned wcount[16];
    const CcChunk c = cc_chunk(a.n, a.cpe);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool is_root[4];
    unsigned below[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned i = (unsigned)j * CC_THREADS + threadIdx.x;
        is_root[j] = i < c.valid && a.root[c.base + i] == (int)(c.base + i);
        const unsigned long long m = __ballot(is_root[j]);
        below[j] = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcount[j * 4 + wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    const long long first = a.excl[(unsigned long long)c.e * a.cpe];
    const long long base = a.excl[blockIdx.x] - first;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned before = 0;
#pragma unroll
        for (int s = 0; s < 16; ++s)
            if (s < j * 4 + wave) before += wcount[s];
        if (is_root[j]) rank[c.base + (unsigned)j * CC_THREADS + threadIdx.x] = (int)(base + before + below[j] + 1);
    }
    if (threadIdx.x == 0 && blockIdx.x == c.e * a.cpe)
        a.count[c.e] = a.err[c.e] ? -1 : a.excl[(unsigned long long)(c.e + 1) * a.cpe] - first;
}

__global__ __launch_bounds__(CC_THREADS) void cc_relabel_kernel(int* cc, const int* __restrict__ rank, unsigned total) {
    const unsigned long long i = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= total) return;
    const int r = cc[i];
    cc[i] = r < 0 ? 0 : rank[r];
}

// ---------------------------------------------------------------------------------------------------------- remove_small
// The keys of a chunk are folded in an LDS table before anything touches global memory: open addressing with linear probing, CC_HASH
// slots for at most CC_TILE distinct keys, so a probe always ends at the key or at a free slot within CC_HASH steps.
constexpr int CC_HASH = CC_TILE;

__device__ __forceinline__ int cc_hash_slot(int* hkey, int key) {
    unsigned h = ((unsigned)key * 2654435761u) >> 22;
    static_assert(CC_HASH == 1 << 10, "the hash keeps 10 bits");
    for (int probe = 0; probe < CC_HASH; ++probe) {
        const int old = atomicCAS(hkey + h, -1, key);
        if (old == -1 || old == key) return (int)h;
        h = (h + 1) & (CC_HASH - 1);
    }
    return -1;
}

__global__ __launch_bounds__(CC_THREADS) void cc_area_kernel(const int* __restrict__ root, unsigned* area, unsigned n, unsigned cpe) {
    __shared__ int hkey[CC_HASH];
    __shared__ unsigned hcnt[CC_HASH];
    const CcChunk c = cc_chunk(n, cpe);
    const int lane = threadIdx.x & 63;
    for (int s = threadIdx.x; s < CC_HASH; s += CC_THREADS) { hkey[s] = -1; hcnt[s] = 0; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned i = (unsigned)j * CC_THREADS + threadIdx.x;
        const int key = i < c.valid ? root[c.base + i] : -1;
        bool leader;
        const int len = cc_seg_len(key, lane, leader);
        if (leader && key >= 0) {
            const int slot = cc_hash_slot(hkey, key);
            if (slot >= 0) atomicAdd(hcnt + slot, (unsigned)len);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < CC_HASH; s += CC_THREADS)      // one add per (workgroup, component)
        if (hkey[s] >= 0) atomicAdd(area + hkey[s], hcnt[s]);
}

template <class U>
__global__ __launch_bounds__(CC_THREADS) void cc_rewrite_kernel(const U* in, U* out, const int* __restrict__ root, const unsigned* __restrict__ area,
                                                                const int* __restrict__ err, unsigned n, unsigned total, long long min_area, U fill) {
    const unsigned long long i = (unsigned long long)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= total) return;
    const int r = root[i];
    const U v = in[i];
    const bool small = r >= 0 && (long long)area[r] < min_area && err[(unsigned)i / n] == 0;
    out[i] = small ? fill : v;
}

// ---------------------------------------------------------------------------------------------------------- statistics
struct CcStatsArgs {
    const int* cc;
    const void* values;
    long long* area;            // [nmax]
    long long* bbox;            // [nmax, 2 * dims]: minima, then maxima
    void* value;                // [nmax]
    unsigned n;
    int H, W, dims, nmax;
};

__global__ __launch_bounds__(CC_THREADS) void cc_stats_init_kernel(long long* area, long long* bbox, int nmax, int dims) {
    const int c = blockIdx.x * CC_THREADS + threadIdx.x;
    if (c >= nmax) return;
    area[c] = 0;
    for (int d = 0; d < dims; ++d) {
        bbox[(long long)c * 2 * dims + d] = 0x7fffffffffffffffLL;
        bbox[(long long)c * 2 * dims + dims + d] = -1;
    }
}

// The box of positions s .. s + len - 1 (consecutive in row-major order): once the range passes a row end it holds x = W - 1 and
// x = 0; once it passes a slice end it holds y = H - 1 and y = 0.
__device__ __forceinline__ void cc_range_box(unsigned s, unsigned len, unsigned H, unsigned W, int (&lo)[3], int (&hi)[3]) {
    const unsigned t = s + len - 1;
    const unsigned row_s = s / W, row_t = t / W;
    const unsigned zs = row_s / H, zt = row_t / H;
    lo[0] = (int)zs; hi[0] = (int)zt;
    lo[1] = zs == zt ? (int)(row_s - zs * H) : 0; hi[1] = zs == zt ? (int)(row_t - zt * H) : (int)H - 1;
    lo[2] = row_s == row_t ? (int)(s - row_s * W) : 0; hi[2] = row_s == row_t ? (int)(t - row_t * W) : (int)W - 1;
}

template <int VB>
__global__ __launch_bounds__(CC_THREADS) void cc_stats_kernel(const CcStatsArgs a, unsigned cpe) {
    __shared__ int hkey[CC_HASH];
    __shared__ unsigned hcnt[CC_HASH];
    __shared__ int hlo[3][CC_HASH], hhi[3][CC_HASH];
    const CcChunk c = cc_chunk(a.n, cpe);
    const int lane = threadIdx.x & 63;
    for (int s = threadIdx.x; s < CC_HASH; s += CC_THREADS) {
        hkey[s] = -1; hcnt[s] = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) { hlo[d][s] = 0x7fffffff; hhi[d][s] = -1; }
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const unsigned i = (unsigned)j * CC_THREADS + threadIdx.x;
        const int key = i < c.valid ? a.cc[c.base + i] : -1;
        bool leader;
        const int len = cc_seg_len(key, lane, leader);
        if (leader && key >= 1 && key <= a.nmax) {              // components numbered above nmax are left out
            const int slot = cc_hash_slot(hkey, key);
            if (slot >= 0) {
                int lo[3], hi[3];
                cc_range_box(c.base + i, (unsigned)len, (unsigned)a.H, (unsigned)a.W, lo, hi);
                atomicAdd(hcnt + slot, (unsigned)len);
#pragma unroll
                for (int d = 0; d < 3; ++d) { atomicMin(&hlo[d][slot], lo[d]); atomicMax(&hhi[d][slot], hi[d]); }
            }
            if constexpr (VB > 0) {                              // every position of a component holds the same class: any store is the value
                using V = std::conditional_t<VB == 1, unsigned char, std::conditional_t<VB == 2, unsigned short, std::conditional_t<VB == 4, unsigned, unsigned long long>>>;
                reinterpret_cast<V*>(a.value)[key - 1] = reinterpret_cast<const V*>(a.values)[c.base + i];
            }
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < CC_HASH; s += CC_THREADS) {   // one set of 64-bit atomics per (workgroup, component)
        if (hkey[s] < 1) continue;
        const long long row = hkey[s] - 1;
        atomicAdd(reinterpret_cast<unsigned long long*>(a.area + row), (unsigned long long)hcnt[s]);
        long long* b = a.bbox + row * 2 * a.dims;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int col = d - (3 - a.dims);                   // (2-D: z is not a column)
            if (col >= 0) {
                __hip_atomic_fetch_min(b + col, (long long)hlo[d][s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_max(b + a.dims + col, (long long)hhi[d][s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// maxima become exclusive; rows without a position are all zero
__global__ __launch_bounds__(CC_THREADS) void cc_stats_finish_kernel(const long long* __restrict__ area, long long* bbox, int nmax, int dims) {
    const int c = blockIdx.x * CC_THREADS + threadIdx.x;
    if (c >= nmax) return;
    const bool none = area[c] == 0;
    for (int d = 0; d < dims; ++d) {
        long long* lo = bbox + (long long)c * 2 * dims + d;
        long long* hi = lo + dims;
        *lo = none ? 0 : *lo;
        *hi = none ? 0 : *hi + 1;
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
struct CcPlan {
    int dims, D, H, W, TZ, TY, TX, tz, ty, tx;
    long long B, n, total, tiles, cpe, chunks;
    int levels;
    long long cnt[SCAN_MAX_LEVELS];
    long long off_err, off_parent, off_counts, off_excl, off_sums[SCAN_MAX_LEVELS], label_bytes;
    long long off_root, remove_bytes;
};

static int cc_plan(int dims, long long B, long long D, long long H, long long W, CcPlan& p) {
    if ((dims != 2 && dims != 3) || B < 1 || D < 1 || H < 1 || W < 1 || (dims == 2 && D != 1)) return PTB_EINVAL;
    if (D > MAX_POS || H > MAX_POS || W > MAX_POS || H * W > MAX_POS || D * H * W > MAX_POS || B > MAX_POS / (D * H * W)) return PTB_EUNSUPPORTED;
    p.dims = dims; p.D = (int)D; p.H = (int)H; p.W = (int)W; p.B = B;
    p.TZ = dims == 3 ? CcTile<true>::TZ : CcTile<false>::TZ;
    p.TY = dims == 3 ? CcTile<true>::TY : CcTile<false>::TY;
    p.TX = dims == 3 ? CcTile<true>::TX : CcTile<false>::TX;
    p.tz = (p.D + p.TZ - 1) / p.TZ; p.ty = (p.H + p.TY - 1) / p.TY; p.tx = (p.W + p.TX - 1) / p.TX;
    p.n = D * H * W; p.total = B * p.n;
    p.tiles = B * p.tz * p.ty * p.tx;
    p.cpe = (p.n + CC_TILE - 1) / CC_TILE;
    p.chunks = B * p.cpe;
    if (p.tiles > MAX_POS || p.chunks > MAX_POS) return PTB_EUNSUPPORTED;
    p.levels = scan_levels(p.chunks + 1, p.cnt);
    long long o = 0;
    p.off_err = o; o += up16(4 * B);
    p.off_parent = o; o += up16(4 * p.total);
    p.off_root = o; p.remove_bytes = o + up16(4 * p.total);
    p.off_counts = o; o += up16(4 * (p.chunks + 1));
    p.off_excl = o; o += up16(8 * (p.chunks + 1));
    for (int l = 0; l < p.levels; ++l) { p.off_sums[l] = o; o += up16(8 * p.cnt[l]); }
    p.label_bytes = o;
    return PTB_OK;
}

static bool cc_bad_conn(int dims, int c) { return dims == 2 ? (c != 4 && c != 8) : (c != 6 && c != 26); }

// phases 1 - 3: the roots of every position into `root`; the roots per chunk into counts when given
static int cc_roots(const void* labels, int elem_bytes, const CcPlan& p, int connectivity, int has_bg, long long bg, char* ws, int* root, unsigned* counts,
                    hipStream_t s) {
    CcArgs a{};
    a.labels = labels; a.parent = reinterpret_cast<int*>(ws + p.off_parent); a.err = reinterpret_cast<int*>(ws + p.off_err);
    a.bg = bg; a.has_bg = has_bg != 0; a.n = (unsigned)p.n; a.total = (unsigned)p.total; a.D = p.D; a.H = p.H; a.W = p.W; a.tz = p.tz; a.ty = p.ty; a.tx = p.tx;
    if (hipError_t e = hipMemsetAsync(a.err, 0, (size_t)up16(4 * p.B), s); e != hipSuccess) { set_hip_error(e); return PTB_ELAUNCH; }
    const bool full = connectivity == 8 || connectivity == 26;
    const bool wide = p.W % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % std::min(4 * elem_bytes, 16) == 0;
    const unsigned seam_blocks = (unsigned)std::min<long long>((p.total + CC_THREADS - 1) / CC_THREADS, CC_SEAM_BLOCKS);
    with_value<1, 2, 4, 8>(elem_bytes, [&](auto eb) {
        using T = label_t<eb()>;
        with_bool(p.dims == 3, [&](auto d3) {
            with_bool(full, [&](auto f) {
                with_bool(wide, [&](auto w) {
                    hipLaunchKernelGGL((cc_local_kernel<T, w(), f(), d3()>), dim3((unsigned)p.tiles), dim3(CC_THREADS), 0, s, a);
                });
                hipLaunchKernelGGL((cc_seam_kernel<T, f(), d3()>), dim3(seam_blocks), dim3(CC_THREADS), 0, s, a);
            });
        });
    });
    CcChunkArgs c{};
    c.parent = a.parent; c.root = root; c.err = a.err; c.counts = counts; c.n = a.n; c.cpe = (unsigned)p.cpe;
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)p.chunks), dim3(CC_THREADS), 0, s, c);
    return check_launch();
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_cc_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int* tile, int64_t* tiles, int64_t* chunks, int* scan_levels,
                           int64_t* label_workspace_bytes, int64_t* remove_workspace_bytes) {
    CcPlan p;
    if (int rc = cc_plan(dims, B, D, H, W, p)) return rc;
    if (tile) { tile[0] = p.TZ; tile[1] = p.TY; tile[2] = p.TX; }
    if (tiles) *tiles = p.tiles;
    if (chunks) *chunks = p.chunks;
    if (scan_levels) *scan_levels = p.levels;
    if (label_workspace_bytes) *label_workspace_bytes = p.label_bytes;
    if (remove_workspace_bytes) *remove_workspace_bytes = p.remove_bytes;
    return PTB_OK;
}

extern "C" int ptb_cc_label(const void* labels, int elem_bytes, int dims, int64_t B, int64_t D, int64_t H, int64_t W, int connectivity, int has_background,
                            int64_t background, int32_t* cc, int64_t* count, void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (!labels || !cc || !count || !workspace || bad_elem_bytes(elem_bytes) || (dims != 2 && dims != 3) || cc_bad_conn(dims, connectivity)) return PTB_EINVAL;
    CcPlan p;
    if (int rc = cc_plan(dims, B, D, H, W, p)) return rc;
    if (workspace_bytes < p.label_bytes || !aligned16(workspace) || !aligned16(cc)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    unsigned* counts = reinterpret_cast<unsigned*>(ws + p.off_counts);
    long long* excl = reinterpret_cast<long long*>(ws + p.off_excl);
    if (int rc = cc_roots(labels, elem_bytes, p, connectivity, has_background, background, ws, cc, counts, s)) return rc;
    long long* sums[SCAN_MAX_LEVELS] = {};
    for (int l = 0; l < p.levels; ++l) sums[l] = reinterpret_cast<long long*>(ws + p.off_sums[l]);
    scan_exclusive(counts, p.chunks + 1, p.levels, p.cnt, sums, excl, s);
    CcChunkArgs c{};
    c.root = cc; c.err = reinterpret_cast<int*>(ws + p.off_err); c.excl = excl; c.count = reinterpret_cast<long long*>(count);
    c.n = (unsigned)p.n; c.cpe = (unsigned)p.cpe;
    int* rank = reinterpret_cast<int*>(ws + p.off_parent);                 // (the parent map is not read again)
    hipLaunchKernelGGL(cc_rank_kernel, dim3((unsigned)p.chunks), dim3(CC_THREADS), 0, s, c, rank);
    hipLaunchKernelGGL(cc_relabel_kernel, dim3((unsigned)((p.total + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, s, cc, (const int*)rank, (unsigned)p.total);
    return check_launch();
}

extern "C" int ptb_cc_remove_small(const void* labels, int elem_bytes, int dims, int64_t B, int64_t D, int64_t H, int64_t W, int connectivity,
                                   int has_background, int64_t background, int64_t min_area, int64_t fill, void* out, void* workspace,
                                   int64_t workspace_bytes, ptb_stream_t stream) {
    if (!labels || !out || !workspace || bad_elem_bytes(elem_bytes) || (dims != 2 && dims != 3) || cc_bad_conn(dims, connectivity)) return PTB_EINVAL;
    CcPlan p;
    if (int rc = cc_plan(dims, B, D, H, W, p)) return rc;
    if (workspace_bytes < p.remove_bytes || !aligned16(workspace)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    int* root = reinterpret_cast<int*>(ws + p.off_root);
    if (int rc = cc_roots(labels, elem_bytes, p, connectivity, has_background, background, ws, root, nullptr, s)) return rc;
    unsigned* area = reinterpret_cast<unsigned*>(ws + p.off_parent);       // (the parent map is not read again; an area is < 2^31)
    if (hipError_t e = hipMemsetAsync(area, 0, (size_t)(4 * p.total), s); e != hipSuccess) { set_hip_error(e); return PTB_ELAUNCH; }
    hipLaunchKernelGGL(cc_area_kernel, dim3((unsigned)p.chunks), dim3(CC_THREADS), 0, s, (const int*)root, area, (unsigned)p.n, (unsigned)p.cpe);
    const dim3 grid((unsigned)((p.total + CC_THREADS - 1) / CC_THREADS));
    const int* err = reinterpret_cast<const int*>(ws + p.off_err);
    with_value<1, 2, 4, 8>(elem_bytes, [&](auto eb) {
        using U = std::make_unsigned_t<label_t<eb()>>;
        hipLaunchKernelGGL((cc_rewrite_kernel<U>), grid, dim3(CC_THREADS), 0, s, reinterpret_cast<const U*>(labels), reinterpret_cast<U*>(out), (const int*)root,
                           (const unsigned*)area, err, (unsigned)p.n, (unsigned)p.total, (long long)min_area, (U)fill);
    });
    return check_launch();
}

extern "C" int ptb_cc_stats(const int32_t* cc, int dims, int64_t D, int64_t H, int64_t W, int64_t max_components, const void* values, int values_elem_bytes,
                            int64_t* area, int64_t* bbox, void* value, ptb_stream_t stream) {
    if (!cc || !area || !bbox || max_components < 1 || (values != nullptr) != (value != nullptr) || (values && bad_elem_bytes(values_elem_bytes))) return PTB_EINVAL;
    CcPlan p;
    if (int rc = cc_plan(dims, 1, D, H, W, p)) return rc;
    if (max_components > MAX_POS) return PTB_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    CcStatsArgs a{};
    a.cc = cc; a.values = values; a.area = reinterpret_cast<long long*>(area); a.bbox = reinterpret_cast<long long*>(bbox); a.value = value;
    a.n = (unsigned)p.n; a.H = p.H; a.W = p.W; a.dims = dims; a.nmax = (int)max_components;
    const dim3 rows((unsigned)((max_components + CC_THREADS - 1) / CC_THREADS));
    if (value) {
        if (hipError_t e = hipMemsetAsync(value, 0, (size_t)(max_components * values_elem_bytes), s); e != hipSuccess) { set_hip_error(e); return PTB_ELAUNCH; }
    }
    hipLaunchKernelGGL(cc_stats_init_kernel, rows, dim3(CC_THREADS), 0, s, a.area, a.bbox, a.nmax, dims);
    with_value<0, 1, 2, 4, 8>(values ? values_elem_bytes : 0, [&](auto vb) {
        hipLaunchKernelGGL((cc_stats_kernel<vb()>), dim3((unsigned)p.chunks), dim3(CC_THREADS), 0, s, a, (unsigned)p.cpe);
    });
    hipLaunchKernelGGL(cc_stats_finish_kernel, rows, dim3(CC_THREADS), 0, s, (const long long*)a.area, a.bbox, a.nmax, dims);
    return check_launch();
}
