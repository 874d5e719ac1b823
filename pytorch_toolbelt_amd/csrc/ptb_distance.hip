// Exact Euclidean distance transform of label maps on the device (utils/distance.py; the reference has no counterpart).  The transform
// is separable, one launch per axis:
//   1. edt_row_kernel    a wave walks one row along W in chunks of 256 positions (four neighbouring x per lane, one wide load), forward
//                        with the index of the last site carried in a register -- the nearest site to the left inside a chunk is a
//                        wave max-scan of `is_site ? x : -1` -- and then backward with the mirror image (min-scan of `is_site ? x :
//                        BIG`).  The forward walk leaves the left index in the map, the backward walk recognises sites by L[x] == x (the
//                        labels are read once) and writes the 1-D squared distance: int32, or float32 (sx * dx)^2 with spacing, or the
//                        "infinite" sentinel in a row without a site.  The carry starts afresh in every row: a wave owns one row.
//   2. edt_line_kernel   along H, then along D for dims = 3: the lower envelope of the parabolas f(j) + (i - j)^2 of every line
//                        (Meijster, Roerdink & Hesselink 2000).  One lane per line, the 64 lanes of a wave on 64 neighbouring lines, so
//                        every load and store of the wave is a contiguous row segment although the line itself is strided.  The
//                        envelope's stack (vertex index s, start t of its interval) lies in the workspace, laid out [height][line]
//                        like the map itself -- it is NOT a private array: no scratch -- and its top entry is kept in registers, so the
//                        stack is written at a push and read at a pop only.  Sentinel values push nothing; a line that ends with an
//                        empty stack is written as the sentinel.  The last pass writes the final form: the int32, sqrtf of its float32
//                        conversion, or on the second run of a signed call the difference with what the first run left in `out`.
// EXACTNESS.  With unit spacing everything is int32.  Under the limit D^2 + H^2 + W^2 <= 2^31 - 2 every g(i) + (x - i)^2 that is
// evaluated is at most that sum (g holds the squared offsets of the axes already done, x and i lie on the current axis).  The
// separator Sep(i, u) = ((g(u) + u^2) - (g(i) + i^2)) div (2 (u - i)), i < u, is evaluated only after the pop loop has ended with
// f(t, i) <= f(t, u) at the start t >= 0 of i's interval: (t - i)^2 + g(i) <= (t - u)^2 + g(u) is the same as
// (g(u) + u^2) - (g(i) + i^2) >= 2 t (u - i) >= 0.  So the numerator is non-negative, it is the difference of two values in
// [0, 2^31 - 2] and fits, C's division is the floor, and Sep >= t: starts grow with the height.  No 64-bit expression is needed.
// With spacing the maps are float32 and every parabola and separator is evaluated in double from exact integer offsets: the only
// roundings are the one store per pass and the root, and the choice between two parabolas is exact with respect to the stored values.
// EVERY LOOP IS BOUNDED.  The build and query loops run over the extent of the axis; the pop loop lowers the stack height each trip.
// No workgroup waits for another one and there are no atomics: the result is a function of the input alone.
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
    const unsigned row = blockIdx.x * (EDT_ROW_THREADS / 64) + (unsigned)wave_id();
    if (row >= a.rows) return;                                                 // (whole waves leave; nothing below synchronises workgroups)
    const int lane = threadIdx.x & 63;
    const int W = a.W;
    const T* lab = reinterpret_cast<const T*>(a.labels) + (size_t)row * (size_t)W;
    int* map = a.map + (size_t)row * (size_t)W;
    const T val = (T)a.value;
    const int chunks = (W + EDT_CHUNK - 1) / EDT_CHUNK;

    int carry = -1;                                                            // the last site at or before the chunk: none yet in this row
#pragma unroll 1
    for (int c = 0; c < chunks; ++c) {
        const int x = c * EDT_CHUNK + lane * 4;
        T v[4] = {(T)0, (T)0, (T)0, (T)0};
        if constexpr (WIDE) {                                                  // W % 4 == 0 and an aligned base: x < W means x + 3 < W
            constexpr int A = sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16;
            if (x < W) __builtin_memcpy(v, __builtin_assume_aligned(lab + x, A), sizeof(v));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < W) v[j] = lab[x + j];
        }
        int p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool site = x + j < W && (a.mode == EDT_SITE_EQ ? v[j] == val : a.mode == EDT_SITE_NE ? v[j] != val : a.mode == EDT_SITE_ALL);
            const int m = site ? x + j : -1;
            p[j] = j > 0 ? max(p[j > 0 ? j - 1 : 0], m) : m;
        }
        const int inc = edt_scan_max(p[3], lane);
        int exc = __shfl_up(inc, 1);
        if (lane == 0) exc = -1;
        const int before = max(carry, exc);
        int L[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) L[j] = max(before, p[j]);
        if constexpr (WIDE) {
            if (x < W) *reinterpret_cast<int4*>(map + x) = make_int4(L[0], L[1], L[2], L[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < W) map[x + j] = L[j];
        }
        carry = max(carry, __shfl(inc, 63));
    }

    carry = EDT_BIG;                                                           // the first site at or behind the chunk: none yet
#pragma unroll 1
    for (int c = chunks - 1; c >= 0; --c) {
        const int x = c * EDT_CHUNK + lane * 4;
        int L[4] = {-1, -1, -1, -1};
        if constexpr (WIDE) {
            if (x < W) {
                const int4 l = *reinterpret_cast<const int4*>(map + x);        // (written by this lane itself in the forward walk)
                L[0] = l.x; L[1] = l.y; L[2] = l.z; L[3] = l.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < W) L[j] = map[x + j];
        }
        int s[4];
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            const int m = (x + j < W && L[j] == x + j) ? x + j : EDT_BIG;      // a site is its own nearest site to the left
            s[j] = j < 3 ? min(s[j < 3 ? j + 1 : 3], m) : m;
        }
        const int inc = edt_scan_min_rev(s[0], lane);
        int exc = __shfl_down(inc, 1);
        if (lane == 63) exc = EDT_BIG;
        const int behind = min(carry, exc);
        int out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int R = min(behind, s[j]);
            const int dl = L[j] >= 0 ? x + j - L[j] : EDT_BIG;
            const int dr = R < EDT_BIG ? R - (x + j) : EDT_BIG;
            const int d = min(dl, dr);
            if constexpr (FLT) {
                const double t = a.sx * (double)d;
                out[j] = __float_as_int(d == EDT_BIG ? INFINITY : (float)(t * t));
            } else {
                out[j] = d == EDT_BIG ? EDT_INF : d * d;                       // d < W <= 46340
            }
        }
        if constexpr (WIDE) {
            if (x < W) *reinterpret_cast<int4*>(map + x) = make_int4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < W) map[x + j] = out[j];
        }
        carry = min(carry, __shfl(inc, 0));
    }
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
    using X = EdtValue<FLT>;
    using V = typename X::V;
    const unsigned o = blockIdx.x / a.bpo;
    const unsigned l = (blockIdx.x - o * a.bpo) * EDT_LINE_THREADS + threadIdx.x;
    if (l >= a.inner) return;
    const unsigned inner = a.inner;
    const int n = (int)a.n;
    const unsigned base = o * a.n * inner + l;                                 // position k of the line: base + k * inner (< 2^31)
    const V* in = reinterpret_cast<const V*>(a.in);

    // the envelope: entries 0 .. q - 1 of the stack are in memory, entry q is (s, t, g)
    int q = -1, s = 0, t = 0;
    V g = (V)0;
    V next = in[base];
#pragma unroll 1
    for (int u = 0; u < n; ++u) {
        const V gu = next;
        if (u + 1 < n) next = in[base + (unsigned)(u + 1) * inner];
        if (X::none(gu)) continue;                                             // no site in the rest of the axes: no parabola
        while (q >= 0 && X::at(t, s, g, a.sp) > X::at(t, u, gu, a.sp)) {      // (each trip lowers q)
            if (--q >= 0) {
                s = a.s[base + (unsigned)q * inner];
                t = a.t[base + (unsigned)q * inner];
                g = in[base + (unsigned)s * inner];
            }
        }
        if (q < 0) {
            q = 0; s = u; t = 0; g = gu;
        } else {
            int w = X::first(s, u, g, gu, a.sp, n);
            if (FLT && w <= t) w = t + 1;                                      // (starts stay strictly increasing whatever the rounding)
            if (w < n) {
                a.s[base + (unsigned)q * inner] = s;
                a.t[base + (unsigned)q * inner] = t;
                ++q; s = u; t = w; g = gu;
            }
        }
    }

#pragma unroll 1
    for (int u = n - 1; u >= 0; --u) {
        const unsigned p = base + (unsigned)u * inner;
        V d;
        if (q < 0) {
            if constexpr (FLT) d = INFINITY;
            else d = EDT_INF;
        } else {
            d = X::store(X::at(u, s, g, a.sp));
            if (u == t && q > 0) {                                             // (t of entry 0 is 0: the stack lasts for the whole line)
                --q;
                s = a.s[base + (unsigned)q * inner];
                t = a.t[base + (unsigned)q * inner];
                g = in[base + (unsigned)s * inner];
            }
        }
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
    }
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
    const long long map = edt_up16(4 * p.total);
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
        using T = edt_label_t<eb()>;
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
    if (!labels || !out || !workspace || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)) return PTB_EINVAL;
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
    const int mode = edt_holds(elem_bytes, value) ? (site_rule == PTB_EDT_SITES_EQUAL ? EDT_SITE_EQ : EDT_SITE_NE)
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
