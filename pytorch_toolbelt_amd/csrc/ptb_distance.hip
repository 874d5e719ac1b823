// Exact Euclidean distance transform of label maps on the device (utils/distance.py; the reference has no counterpart).  The transform
// is separable, one launch per axis:
//   1. edt_row_kernel    the row pass along W: the 1-D squared distance to the nearest site of the row.
//   2. edt_line_kernel   the envelope pass along H, then along D for dims = 3.  The last pass writes the final form: the int32, sqrtf of its
//                        float32 conversion, or on the second run of a signed call the difference with what the first run left in `out`.
// The passes, the argument of their exactness and the bounds of their loops: ptb_edt_common.h (edt_row_pass, edt_line_pass), shared
// with the feature transform (ptb_nearest.hip).
#include <algorithm>
#include <cmath>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_edt_common.h"

namespace ptb {

// ---------------------------------------------------------------------------------------------------------- row pass
struct EdtRowArgs {
    const void* labels;
    int* map;                   // [rows, W]: int32, or float32 bits with spacing
    long long value;
    double sx;
    unsigned rows;
    int W, mode;
};

template <class T, bool WIDE, bool FLT>
__global__ __launch_bounds__(EDT_ROW_THREADS) void edt_row_kernel(const EdtRowArgs a) {
    edt_row_pass<T, WIDE, FLT, false>(a);
}

// ---------------------------------------------------------------------------------------------------------- line passes
struct EdtLineArgs {
    const void* in;             // the map of the previous axis
    void* out;                  // the map of this axis; on the last pass the result
    int* s;                     // stack: the vertex of every parabola of the envelope ...
    int* t;                     // ... and the first index at which it is the lowest; both [outer][height][inner]
    double sp;                  // spacing along this axis
    unsigned n, inner, bpo;     // extent of the axis; neighbouring lines per outer group; workgroups per outer group
    int root, second, out_i32;  // last pass only: take the root; subtract what out holds; write int32
};

template <bool FLT, bool LAST>
__global__ __launch_bounds__(EDT_LINE_THREADS) void edt_line_kernel(const EdtLineArgs a) {
    using V = typename EdtValue<FLT>::V;
    edt_line_pass<FLT, false>(a, [&](unsigned p, V d, int) {
        if constexpr (!LAST) {
            reinterpret_cast<V*>(a.out)[p] = d;
        } else if (a.out_i32) {                                                // (unit spacing only: V is int)
            int r = (int)d;
            if (a.second) r -= reinterpret_cast<const int*>(a.out)[p];         // exactly one of the two terms is non-zero
            reinterpret_cast<int*>(a.out)[p] = r;
        } else {
            float r;
            if constexpr (FLT) r = d;
            else r = d == EDT_INF ? INFINITY : (float)d;
            if (a.root) r = sqrtf(r);
            if (a.second) r -= reinterpret_cast<const float*>(a.out)[p];
            reinterpret_cast<float*>(a.out)[p] = r;
        }
    });
}

// ---------------------------------------------------------------------------------------------------------- host side
struct EdtPlan {
    int dims, D, H, W;
    long long B, total;
    long long off_map, off_s, off_t, off_map2, bytes;
};

static int edt_plan(int dims, long long B, long long D, long long H, long long W, bool is_signed, EdtPlan& p) {
    if (int rc = edt_check_shape(dims, B, D, H, W)) return rc;
    p.dims = dims; p.D = (int)D; p.H = (int)H; p.W = (int)W; p.B = B; p.total = B * D * H * W;
    const long long map = up16(4 * p.total);
    long long o = 0;
    p.off_map = o; o += map;
    p.off_s = o; o += map;
    p.off_t = o; o += map;
    p.off_map2 = o;
    if (is_signed && dims == 3) o += map;
    p.bytes = o;
    return PTB_OK;
}

// one run of the passes; first: the map the row pass writes
static void edt_run(const void* labels, int elem_bytes, const EdtPlan& p, int mode, long long value, const double* sp, bool root, bool second, bool out_i32,
                    void* out, int* first, char* ws, hipStream_t s) {
    const bool flt = sp != nullptr;
    int* map = reinterpret_cast<int*>(ws + p.off_map);
    EdtRowArgs r{};
    r.labels = labels; r.map = first; r.value = value; r.sx = flt ? sp[2] : 1.0; r.rows = (unsigned)(p.B * p.D * p.H); r.W = p.W; r.mode = mode;
    const bool wide = p.W % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % std::min(4 * elem_bytes, 16) == 0;
    const unsigned row_blocks = (r.rows + EDT_ROW_THREADS / 64 - 1) / (EDT_ROW_THREADS / 64);
    with_value<1, 2, 4, 8>(elem_bytes, [&](auto eb) {
        using T = label_t<eb()>;
        with_bool(wide, [&](auto w) {
            with_bool(flt, [&](auto f) {
                hipLaunchKernelGGL((edt_row_kernel<T, w(), f()>), dim3(row_blocks), dim3(EDT_ROW_THREADS), 0, s, r);
            });
        });
    });
    auto line = [&](const void* in, void* to, unsigned outer, unsigned n, unsigned inner, double spacing, bool last) {
        EdtLineArgs a{};
        a.in = in; a.out = to; a.s = reinterpret_cast<int*>(ws + p.off_s); a.t = reinterpret_cast<int*>(ws + p.off_t); a.sp = spacing;
        a.n = n; a.inner = inner; a.bpo = (inner + EDT_LINE_THREADS - 1) / EDT_LINE_THREADS;
        a.root = root; a.second = second; a.out_i32 = out_i32;
        with_bool(flt, [&](auto f) {
            with_bool(last, [&](auto la) {
                hipLaunchKernelGGL((edt_line_kernel<f(), la()>), dim3(outer * a.bpo), dim3(EDT_LINE_THREADS), 0, s, a);
            });
        });
    };
    if (p.dims == 2) {
        line(first, out, (unsigned)p.B, (unsigned)p.H, (unsigned)p.W, flt ? sp[1] : 1.0, true);
    } else {
        line(first, map, (unsigned)(p.B * p.D), (unsigned)p.H, (unsigned)p.W, flt ? sp[1] : 1.0, false);
        line(map, out, (unsigned)p.B, (unsigned)p.D, (unsigned)(p.H * p.W), flt ? sp[0] : 1.0, true);
    }
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_edt_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int is_signed, int64_t* workspace_bytes) {
    EdtPlan p;
    if (int rc = edt_plan(dims, B, D, H, W, is_signed != 0, p)) return rc;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return PTB_OK;
}

extern "C" int ptb_edt(const void* labels, int elem_bytes, int dims, int64_t B, int64_t D, int64_t H, int64_t W, int site_rule, int64_t value,
                       const double* spacing, int flags, void* out, int out_kind, void* workspace, int64_t workspace_bytes, ptb_stream_t stream) {
    if (!labels || !out || !workspace || bad_elem_bytes(elem_bytes)) return PTB_EINVAL;
    if ((site_rule != PTB_EDT_SITES_EQUAL && site_rule != PTB_EDT_SITES_NOT_EQUAL) || (flags & ~(PTB_EDT_SQUARED | PTB_EDT_SIGNED))) return PTB_EINVAL;
    if (out_kind != PTB_EDT_OUT_F32 && out_kind != PTB_EDT_OUT_I32) return PTB_EINVAL;
    if (out_kind == PTB_EDT_OUT_I32 && (!(flags & PTB_EDT_SQUARED) || spacing)) return PTB_EINVAL;
    if (spacing && !edt_spacing_ok(spacing, dims)) return PTB_EINVAL;
    const bool is_signed = (flags & PTB_EDT_SIGNED) != 0;
    EdtPlan p;
    if (int rc = edt_plan(dims, B, D, H, W, is_signed, p)) return rc;
    if (workspace_bytes < p.bytes || !aligned16(workspace) || !aligned16(out)) return PTB_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    // a value the element type cannot hold occurs nowhere
    const int mode = holds(elem_bytes, value) ? (site_rule == PTB_EDT_SITES_EQUAL ? EDT_SITE_EQ : EDT_SITE_NE)
                                                  : (site_rule == PTB_EDT_SITES_EQUAL ? EDT_SITE_NONE : EDT_SITE_ALL);
    const bool root = !(flags & PTB_EDT_SQUARED), out_i32 = out_kind == PTB_EDT_OUT_I32;
    // the row pass writes the map the first line pass reads: 2-D: workspace -> out; 3-D: out -> workspace -> out
    int* first = p.dims == 2 ? reinterpret_cast<int*>(ws + p.off_map) : reinterpret_cast<int*>(out);
    edt_run(labels, elem_bytes, p, mode, value, spacing, root, false, out_i32, out, first, ws, s);
    if (is_signed) {                                                           // the distances to the other set, minus what out holds
        if (p.dims == 3) first = reinterpret_cast<int*>(ws + p.off_map2);
        edt_run(labels, elem_bytes, p, mode ^ 1, value, spacing, root, true, out_i32, out, first, ws, s);
    }
    return check_launch();
}
