// Nearest-site feature transform of label maps and the label expansion built on it (utils/nearest.py; the reference has no
// counterpart).  The passes are those of the distance transform (ptb_distance.hip, whose scans and parabola arithmetic are shared
// through ptb_edt_common.h), carrying next to every squared distance the FEATURE: the linear index, within the stack entry, of the site
// that distance is measured to; -1 where there is none.
//   1. ft_row_kernel     the two walks of edt_row_kernel.  The backward walk knows the nearest site on either side, L and R, and writes
//                        two maps: the 1-D squared distance as before, and the feature row * W + (dl <= dr ? L : R).
//   2. ft_line_kernel    the envelope pass of edt_line_kernel along H, then along D for dims = 3.  The query walk knows the vertex s of
//                        the parabola that is lowest at every position and copies the feature the previous pass left at s -- one gather
//                        load per position, taken before the pop.  The feature maps ping-pong like the distance maps: a pass never
//                        reads a map it writes.  The last pass stores the distance only where somebody asked for it.
//   3. ft_gather_kernel  expand_labels: a lane per four positions; an unlabelled position takes markers[entry + feature] if it is within
//                        the distance and inside the mask, else the background.
// THE TIE RULE.  Among the sites at the minimum distance the one with the SMALLEST LINEAR INDEX is returned.  Every pass prefers the
// smaller coordinate of its axis on a tie -- the row pass by dl <= dr; the envelope because a parabola is popped only when it is
// strictly higher at the start of its interval and the next one takes over at 1 + floor(intersection), so where two are equal the
// earlier vertex holds -- and the axes are passed from the fastest to the slowest: the last comparison, which overrides the others,
// is on the coordinate that weighs most in the linear index.  With spacing the maps are float32 and the rule holds with respect to
// the stored values: bit for bit wherever those are exact.
// EVERY LOOP IS BOUNDED by the extent of its axis (the pop loop lowers the stack height each trip).  No workgroup waits for another
// one and there are no atomics: the result is a function of the inputs alone.
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
    const unsigned row = blockIdx.x * (EDT_ROW_THREADS / 64) + (unsigned)wave_id();
    if (row >= a.rows) return;                                                 // (whole waves leave; nothing below synchronises workgroups)
    const int lane = threadIdx.x & 63;
    const int W = a.W;
    const T* lab = reinterpret_cast<const T*>(a.labels) + (size_t)row * (size_t)W;
    int* map = a.map + (size_t)row * (size_t)W;
    int* feat = a.feat + (size_t)row * (size_t)W;
    const int row_base = (int)(row % a.rows_per_entry) * W;                    // (an entry has fewer than 2^31 positions)
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
        int out[4], f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int R = min(behind, s[j]);
            const int dl = L[j] >= 0 ? x + j - L[j] : EDT_BIG;
            const int dr = R < EDT_BIG ? R - (x + j) : EDT_BIG;
            const int d = min(dl, dr);
            f[j] = d == EDT_BIG ? -1 : row_base + (dl <= dr ? L[j] : R);       // the left site on a tie: the smaller index
            if constexpr (FLT) {
                const double t = a.sx * (double)d;
                out[j] = __float_as_int(d == EDT_BIG ? INFINITY : (float)(t * t));
            } else {
                out[j] = d == EDT_BIG ? EDT_INF : d * d;                       // d < W <= 46340
            }
        }
        if constexpr (WIDE) {
            if (x < W) {
                *reinterpret_cast<int4*>(map + x) = make_int4(out[0], out[1], out[2], out[3]);
                *reinterpret_cast<int4*>(feat + x) = make_int4(f[0], f[1], f[2], f[3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < W) {
                    map[x + j] = out[j];
                    feat[x + j] = f[j];
                }
        }
        carry = min(carry, __shfl(inc, 0));
    }
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
    using X = EdtValue<FLT>;
    using V = typename X::V;
    const unsigned o = blockIdx.x / a.bpo;
    const unsigned l = (blockIdx.x - o * a.bpo) * EDT_LINE_THREADS + threadIdx.x;
    if (l >= a.inner) return;
    const unsigned inner = a.inner;
    const int n = (int)a.n;
    const unsigned base = o * a.n * inner + l;                                 // position k of the line: base + k * inner (< 2^31)
    const V* in = reinterpret_cast<const V*>(a.in);
    V* out = reinterpret_cast<V*>(a.out);

    // the envelope: entries 0 .. q - 1 of the stack are in memory, entry q is (s, t, g)
    int q = -1, s = 0, t = 0;
    V g = (V)0;
    V next = in[base];
#pragma unroll 1
    for (int u = 0; u < n; ++u) {
        const V gu = next;
        if (u + 1 < n) next = in[base + (unsigned)(u + 1) * inner];
        if (X::none(gu)) continue;                                             // no site in the rest of the axes: no parabola
        while (q >= 0 && X::at(t, s, g, a.sp) > X::at(t, u, gu, a.sp)) {      // (each trip lowers q; equal: the earlier vertex stays)
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
        int f = -1;
        if (q < 0) {
            if constexpr (FLT) d = INFINITY;
            else d = EDT_INF;
        } else {
            d = X::store(X::at(u, s, g, a.sp));
            f = a.fin[base + (unsigned)s * inner];                             // the site the winning vertex measures to (s: before the pop)
            if (u == t && q > 0) {                                             // (t of entry 0 is 0: the stack lasts for the whole line)
                --q;
                s = a.s[base + (unsigned)q * inner];
                t = a.t[base + (unsigned)q * inner];
                g = in[base + (unsigned)s * inner];
            }
        }
        if (out) out[p] = d;
        a.fout[p] = f;
    }
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
    const long long map = edt_up16(4 * p.total);
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
    if (!labels || !workspace || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)) return PTB_EINVAL;
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
    const bool holds = edt_holds(elem_bytes, value);                           // a value the element type cannot hold occurs nowhere
    const int mode = holds ? (site_rule == PTB_EDT_SITES_EQUAL ? EDT_SITE_EQ : EDT_SITE_NE) : (site_rule == PTB_EDT_SITES_EQUAL ? EDT_SITE_NONE : EDT_SITE_ALL);
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
        using T = edt_label_t<eb()>;
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
        g.has_max = has_max; g.flt = flt; g.all_labelled = !holds;
        const bool gwide = p.total % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % std::min(4 * elem_bytes, 16) == 0 &&
                           reinterpret_cast<uintptr_t>(mask) % 4 == 0;
        const unsigned blocks = (unsigned)((p.total + 1023) / 1024);
        with_value<1, 2, 4, 8>(elem_bytes, [&](auto eb) {
            using T = edt_label_t<eb()>;
            with_bool(gwide, [&](auto w) {
                hipLaunchKernelGGL((ft_gather_kernel<T, w()>), dim3(blocks), dim3(256), 0, st, g);
            });
        });
    }
    return check_launch();
}
