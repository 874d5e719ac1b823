// Nearest-site feature transform of label maps and the label expansion built on it (utils/nearest.py; the reference has no
// counterpart).  The passes are those of the distance transform (edt_row_pass and edt_line_pass of ptb_edt_common.h, with FEAT),
// carrying next to every squared distance the FEATURE: the linear index, within the stack entry, of the site that distance is measured
// to; -1 where there is none.  Which site that is among several at the same distance, THE TIE RULE, is stated with the passes.
//   1. ft_row_kernel     the row pass: two maps, the 1-D squared distance and the feature of the nearer site of the row.
//   2. ft_line_kernel    the envelope pass along H, then along D for dims = 3.  The feature maps ping-pong like the distance maps: a pass
//                        never reads a map it writes.  The last pass stores the distance only where somebody asked for it.
//   3. ft_gather_kernel  expand_labels: a lane per four positions; an unlabelled position takes markers[entry + feature] if it is within
//                        the distance and inside the mask, else the background.
#include <algorithm>
#include <cmath>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_edt_common.h"

namespace ptb {

// ---------------------------------------------------------------------------------------------------------- row pass
struct FtRowArgs {
    const void* labels;
    int* map;                   // [rows, W]: the squared distance along the row: int32, or float32 bits with spacing
    int* feat;                  // [rows, W]: the nearest site of the row as an index within the entry, or -1
    long long value;
    double sx;
    unsigned rows, rows_per_entry;
    int W, mode;
};

template <class T, bool WIDE, bool FLT>
__global__ __launch_bounds__(EDT_ROW_THREADS) void ft_row_kernel(const FtRowArgs a) {
    edt_row_pass<T, WIDE, FLT, true>(a);
}

// ---------------------------------------------------------------------------------------------------------- line passes
struct FtLineArgs {
    const void* in;             // the distance map of the previous axis
    void* out;                  // the distance map of this axis; NULL on a last pass whose distances nobody reads
    const int* fin;             // the feature map of the previous axis
    int* fout;                  // the feature map of this axis
    int* s;                     // stack: the vertex of every parabola of the envelope ...
    int* t;                     // ... and the first index at which it is the lowest; both [outer][height][inner]
    double sp;                  // spacing along this axis
    unsigned n, inner, bpo;     // extent of the axis; neighbouring lines per outer group; workgroups per outer group
};

template <bool FLT>
__global__ __launch_bounds__(EDT_LINE_THREADS) void ft_line_kernel(const FtLineArgs a) {
    using V = typename EdtValue<FLT>::V;
    V* out = reinterpret_cast<V*>(a.out);
    edt_line_pass<FLT, true>(a, [&](unsigned p, V d, int f) {
        if (out) out[p] = d;
        a.fout[p] = f;
    });
}

// ---------------------------------------------------------------------------------------------------------- label expansion
struct FtGatherArgs {
    const void* markers;
    void* out;                  // markers' element type
    const int* feat;            // the final feature map
    const int* dist;            // the final squared distances (int32, or float32 bits): read with has_max only
    const unsigned char* mask;  // or NULL
    long long background;
    double max_f;               // has_max: the largest squared distance a label crosses, float32 maps ...
    int max_i;                  // ... and int32 maps
    unsigned total, per_entry;
    int has_max, flt, all_labelled;
};

template <class T, bool WIDE>
__global__ __launch_bounds__(256) void ft_gather_kernel(const FtGatherArgs a) {
    const unsigned p0 = (blockIdx.x * 256u + threadIdx.x) * 4u;                // (total <= 2^31 - 2: p0 + 3 fits 32 bits)
    if (p0 >= a.total) return;
    const T* markers = reinterpret_cast<const T*>(a.markers);
    T* out = reinterpret_cast<T*>(a.out);
    const T bg = (T)a.background;
    T m[4] = {bg, bg, bg, bg};
    int f[4] = {-1, -1, -1, -1}, d[4] = {0, 0, 0, 0};
    unsigned char k[4] = {1, 1, 1, 1};
    if constexpr (WIDE) {                                                      // total % 4 == 0 and aligned bases: all four positions exist
        constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        __builtin_memcpy(m, __builtin_assume_aligned(markers + p0, A), sizeof(m));
        __builtin_memcpy(f, __builtin_assume_aligned(a.feat + p0, 16), sizeof(f));
        if (a.has_max) __builtin_memcpy(d, __builtin_assume_aligned(a.dist + p0, 16), sizeof(d));
        if (a.mask) __builtin_memcpy(k, __builtin_assume_aligned(a.mask + p0, 4), sizeof(k));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < a.total) {
                m[j] = markers[p0 + j];
                f[j] = a.feat[p0 + j];
                if (a.has_max) d[j] = a.dist[p0 + j];
                if (a.mask) k[j] = a.mask[p0 + j];
            }
    }
    unsigned e0 = p0 - p0 % a.per_entry;                                       // the first position of p0's entry
    T r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (p0 + j - e0 >= a.per_entry) e0 += a.per_entry;                     // (at most once per position)
        r[j] = m[j];
        if (a.all_labelled || m[j] != bg) continue;
        const bool near = !a.has_max || (a.flt ? (double)__int_as_float(d[j]) <= a.max_f : d[j] <= a.max_i);
        if (f[j] >= 0 && near && k[j] != 0) r[j] = markers[e0 + (unsigned)f[j]];       // 0 <= feature < per_entry: inside the entry
    }
    if constexpr (WIDE) {
        constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
        __builtin_memcpy(__builtin_assume_aligned(out + p0, A), r, sizeof(r));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < a.total) out[p0 + j] = r[j];
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
// The maps of a call, 4 bytes per position each.  Distances: the row pass writes d0, the pass along H d1, the pass along D d0 again;
// features likewise f0, f1, f0.  The map the LAST pass writes is the caller's tensor where there is one (index_out, squared_out), and is
// not written at all for distances nobody reads; the others and the two stack words lie in the workspace.
struct FtPlan {
    int dims, D, H, W;
    long long B, total;
    bool final_dist;
    long long off_s, off_t, off_d[2], off_f[2], bytes;         // an offset of -1: not in the workspace
};

static int ft_plan(int dims, long long B, long long D, long long H, long long W, int flags, FtPlan& p) {
    if (int rc = edt_check_shape(dims, B, D, H, W)) return rc;
    constexpr int ALL = PTB_NEAREST_INDEX | PTB_NEAREST_SQUARED | PTB_NEAREST_GATHER | PTB_NEAREST_MAX_SQ;
    if ((flags & ~ALL) || !(flags & (PTB_NEAREST_INDEX | PTB_NEAREST_SQUARED | PTB_NEAREST_GATHER))) return PTB_EINVAL;      // asks for nothing
    if ((flags & PTB_NEAREST_MAX_SQ) && !(flags & PTB_NEAREST_GATHER)) return PTB_EINVAL;
    p.dims = dims; p.D = (int)D; p.H = (int)H; p.W = (int)W; p.B = B; p.total = B * D * H * W;
    p.final_dist = (flags & PTB_NEAREST_SQUARED) || (flags & PTB_NEAREST_MAX_SQ);
    const long long map = up16(4 * p.total);
    const int last = dims == 2 ? 1 : 0;                                        // the map of each pair that the last pass writes
    long long o = 0;
    p.off_s = o; o += map;
    p.off_t = o; o += map;
    for (int k = 0; k < 2; ++k) {
        const bool callers = k == last && (flags & PTB_NEAREST_SQUARED), unused = k == last && dims == 2 && !p.final_dist;
        p.off_d[k] = callers || unused ? -1 : o;
        if (p.off_d[k] >= 0) o += map;
    }
    for (int k = 0; k < 2; ++k) {
        p.off_f[k] = k == last && (flags & PTB_NEAREST_INDEX) ? -1 : o;
        if (p.off_f[k] >= 0) o += map;
    }
    p.bytes = o;
    return PTB_OK;
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_nearest_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int flags, int64_t* workspace_bytes) {
    FtPlan p;
    if (int rc = ft_plan(dims, B, D, H, W, flags, p)) return rc;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return PTB_OK;
}

extern "C" int ptb_nearest(const void* labels, int elem_bytes, int dims, int64_t B, int64_t D, int64_t H, int64_t W, int site_rule, int64_t value,
                           const double* spacing, int flags, int32_t* index_out, void* squared_out, void* gather_out, const void* mask, double max_sq,
                           void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (!labels || !workspace || bad_elem_bytes(elem_bytes)) return PTB_EINVAL;
    if (site_rule != PTB_EDT_SITES_EQUAL && site_rule != PTB_EDT_SITES_NOT_EQUAL) return PTB_EINVAL;
    if (spacing && !edt_spacing_ok(spacing, dims)) return PTB_EINVAL;
    FtPlan p;
    if (int rc = ft_plan(dims, B, D, H, W, flags, p)) return rc;
    const bool gather = flags & PTB_NEAREST_GATHER, has_max = flags & PTB_NEAREST_MAX_SQ;
    if (((flags & PTB_NEAREST_INDEX) != 0) != (index_out != nullptr) || ((flags & PTB_NEAREST_SQUARED) != 0) != (squared_out != nullptr)) return PTB_EINVAL;
    if (gather != (gather_out != nullptr) || (mask && !gather)) return PTB_EINVAL;
    if (gather && site_rule != PTB_EDT_SITES_NOT_EQUAL) return PTB_EINVAL;     // the labelled positions are the sites; value is the background
    if (has_max && !(max_sq >= 0.0)) return PTB_EINVAL;
    if (workspace_bytes < p.bytes || !aligned16(workspace) || !aligned16(index_out) || !aligned16(squared_out) || !aligned16(gather_out)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const bool flt = spacing != nullptr;
    const bool held = holds(elem_bytes, value);                                // a value the element type cannot hold occurs nowhere
    const int mode = held ? (site_rule == PTB_EDT_SITES_EQUAL ? EDT_SITE_EQ : EDT_SITE_NE) : (site_rule == PTB_EDT_SITES_EQUAL ? EDT_SITE_NONE : EDT_SITE_ALL);
    const int last = p.dims == 2 ? 1 : 0;
    int *d[2], *f[2];
    for (int k = 0; k < 2; ++k) {
        d[k] = p.off_d[k] >= 0 ? reinterpret_cast<int*>(ws + p.off_d[k]) : k == last ? reinterpret_cast<int*>(squared_out) : nullptr;
        f[k] = p.off_f[k] >= 0 ? reinterpret_cast<int*>(ws + p.off_f[k]) : index_out;
    }

    FtRowArgs r{};
    r.labels = labels; r.map = d[0]; r.feat = f[0]; r.value = value; r.sx = flt ? spacing[2] : 1.0;
    r.rows = (unsigned)(p.B * p.D * p.H); r.rows_per_entry = (unsigned)(p.D * p.H); r.W = p.W; r.mode = mode;
    const bool wide = p.W % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % std::min(4 * elem_bytes, 16) == 0;
    const unsigned row_blocks = (r.rows + EDT_ROW_THREADS / 64 - 1) / (EDT_ROW_THREADS / 64);
    with_value<1, 2, 4, 8>(elem_bytes, [&](auto eb) {
        using T = label_t<eb()>;
        with_bool(wide, [&](auto w) {
            with_bool(flt, [&](auto fl) {
                hipLaunchKernelGGL((ft_row_kernel<T, w(), fl()>), dim3(row_blocks), dim3(EDT_ROW_THREADS), 0, st, r);
            });
        });
    });
    auto line = [&](int from, unsigned outer, unsigned n, unsigned inner, double sp, bool is_last) {
        FtLineArgs a{};
        a.in = d[from]; a.fin = f[from]; a.fout = f[from ^ 1];
        a.out = is_last && !p.final_dist ? nullptr : d[from ^ 1];
        a.s = reinterpret_cast<int*>(ws + p.off_s); a.t = reinterpret_cast<int*>(ws + p.off_t); a.sp = sp;
        a.n = n; a.inner = inner; a.bpo = (inner + EDT_LINE_THREADS - 1) / EDT_LINE_THREADS;
        with_bool(flt, [&](auto fl) {
            hipLaunchKernelGGL((ft_line_kernel<fl()>), dim3(outer * a.bpo), dim3(EDT_LINE_THREADS), 0, st, a);
        });
    };
    line(0, (unsigned)(p.B * p.D), (unsigned)p.H, (unsigned)p.W, flt ? spacing[1] : 1.0, p.dims == 2);
    if (p.dims == 3) line(1, (unsigned)p.B, (unsigned)p.D, (unsigned)(p.H * p.W), flt ? spacing[0] : 1.0, true);

    if (gather) {
        FtGatherArgs g{};
        g.markers = labels; g.out = gather_out; g.feat = f[last]; g.dist = has_max ? d[last] : nullptr;
        g.mask = reinterpret_cast<const unsigned char*>(mask); g.background = value;
        g.max_f = max_sq; g.max_i = max_sq >= 2147483647.0 ? 0x7fffffff : (int)max_sq;
        g.total = (unsigned)p.total; g.per_entry = (unsigned)((long long)p.D * p.H * p.W);
        g.has_max = has_max; g.flt = flt; g.all_labelled = !held;
        const bool gwide = p.total % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % std::min(4 * elem_bytes, 16) == 0 &&
                           reinterpret_cast<uintptr_t>(mask) % 4 == 0;
        const unsigned blocks = (unsigned)((p.total + 1023) / 1024);
        with_value<1, 2, 4, 8>(elem_bytes, [&](auto eb) {
            using T = label_t<eb()>;
            with_bool(gwide, [&](auto w) {
                hipLaunchKernelGGL((ft_gather_kernel<T, w()>), dim3(blocks), dim3(256), 0, st, g);
            });
        });
    }
    return check_launch();
}
