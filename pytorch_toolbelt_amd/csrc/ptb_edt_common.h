// What the distance transform (ptb_distance.hip) and the feature transform (ptb_nearest.hip) share: the sentinels and limits, the two
// wave scans, the arithmetic of a parabola of the lower envelope in its int32 and float32 forms, THE TWO PASSES THEMSELVES (edt_row_pass,
// edt_line_pass: with FEAT they carry the feature next to every distance), and the host-side checks of a shape.  Device pieces are
// forced inline, host pieces are static: each translation unit compiles its own copy.
// EXACTNESS.  With unit spacing everything is int32.  Under the limit D^2 + H^2 + W^2 <= 2^31 - 2 every g(i) + (x - i)^2 that is
// evaluated is at most that sum (g holds the squared offsets of the axes already done, x and i lie on the current axis).  The
// separator Sep(i, u) = ((g(u) + u^2) - (g(i) + i^2)) div (2 (u - i)), i < u, is evaluated only after the pop loop has ended with
// f(t, i) <= f(t, u) at the start t >= 0 of i's interval: (t - i)^2 + g(i) <= (t - u)^2 + g(u) is the same as
// (g(u) + u^2) - (g(i) + i^2) >= 2 t (u - i) >= 0.  So the numerator is non-negative, it is the difference of two values in
// [0, 2^31 - 2] and fits, C's division is the floor, and Sep >= t: starts grow with the height.  No 64-bit expression is needed.
// With spacing the maps are float32 and every parabola and separator is evaluated in double from exact integer offsets: the only
// roundings are the one store per pass and the root, and the choice between two parabolas is exact with respect to the stored values;
// the guard `FLT && w <= t` keeps the starts strictly increasing whatever the rounding of a separator.
// THE TIE RULE.  Among the sites at the minimum distance the one with the SMALLEST LINEAR INDEX is the feature.  Every pass prefers the
// smaller coordinate of its axis on a tie -- the row pass by dl <= dr; the envelope because a parabola is popped only when it is
// strictly higher at the start of its interval and the next one takes over at 1 + floor(intersection), so where two are equal the
// earlier vertex holds -- and the axes are passed from the fastest to the slowest: the last comparison, which overrides the others,
// is on the coordinate that weighs most in the linear index.  With spacing the rule holds with respect to the stored values: bit for
// bit wherever those are exact.
// EVERY LOOP IS BOUNDED.  The walks, the build and the query loops run over the extent of their axis; the pop loop lowers the stack
// height each trip.  No workgroup waits for another one and there are no atomics: the result is a function of the input alone.
#pragma once

#include <cmath>

#include "ptb_common.h"

namespace ptb {

constexpr int EDT_ROW_THREADS = 256;            // four waves, a row each
constexpr int EDT_CHUNK = 256;                  // positions of a row a wave handles per trip: 64 lanes x 4
constexpr int EDT_LINE_THREADS = 64;            // one wave per workgroup: a single 2-D image has only W lines, spread them over the CUs
constexpr int EDT_INF = 0x7fffffff;             // the int32 sentinel
constexpr int EDT_BIG = 0x3fffffff;             // "no site to the right" (an index never reaches it)

enum { EDT_SITE_EQ = 0, EDT_SITE_NE = 1, EDT_SITE_NONE = 2, EDT_SITE_ALL = 3 };

__device__ __forceinline__ int edt_scan_max(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v = max(v, t);
    }
    return v;
}

__device__ __forceinline__ int edt_scan_min_rev(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_down(v, d);
        if (lane + d < 64) v = min(v, t);
    }
    return v;
}

template <bool FLT>
struct EdtValue;

template <>
struct EdtValue<false> {
    using V = int;
    using E = int;              // a parabola's value while it is compared
    static __device__ __forceinline__ bool none(int g) { return g == EDT_INF; }
    static __device__ __forceinline__ int at(int x, int i, int g, double) { return (x - i) * (x - i) + g; }
    // the first index at which the parabola of u lies below that of i < u, given that it does not at the start of i's interval
    static __device__ __forceinline__ int first(int i, int u, int gi, int gu, double, int) { return 1 + ((gu + u * u) - (gi + i * i)) / (2 * (u - i)); }
    static __device__ __forceinline__ int store(int e) { return e; }
};

template <>
struct EdtValue<true> {
    using V = float;
    using E = double;
    static __device__ __forceinline__ bool none(float g) { return g == INFINITY; }
    static __device__ __forceinline__ double at(int x, int i, float g, double sp) {
        const double d = sp * (double)(x - i);
        return d * d + (double)g;
    }
    static __device__ __forceinline__ int first(int i, int u, float gi, float gu, double sp, int n) {
        const double du = sp * (double)u, di = sp * (double)i;
        const double x = ((du * du + (double)gu) - (di * di + (double)gi)) / (2.0 * sp * sp * (double)(u - i));
        if (!(x < (double)n)) return n;                                        // never the lowest inside the line
        return 1 + (int)floor(x < -1.0 ? -1.0 : x);
    }
    static __device__ __forceinline__ float store(double e) { return (float)e; }
};

// ---------------------------------------------------------------------------------------------------------- row pass
// A wave walks one row along W in chunks of 256 positions (four neighbouring x per lane, one wide load), forward with the index of the
// last site carried in a register -- the nearest site to the left inside a chunk is a wave max-scan of `is_site ? x : -1` -- and then
// backward with the mirror image (min-scan of `is_site ? x : BIG`).  The forward walk leaves the left index in the map, the backward
// walk recognises sites by L[x] == x (the labels are read once), knows the nearest site on either side, L and R, and writes the 1-D
// squared distance: int32, or float32 (sx * dx)^2 with spacing, or the "infinite" sentinel in a row without a site; with FEAT also
// the feature row * W + (dl <= dr ? L : R).  The carry starts afresh in every row: a wave owns one row.
// Args is the kernel's own argument struct, so that each kernel keeps its layout: labels, map, value, sx, rows, W, mode, and with FEAT
// feat ([rows, W]: the nearest site of the row as an index within the entry, or -1) and rows_per_entry.
template <class T, bool WIDE, bool FLT, bool FEAT, class Args>
__device__ __forceinline__ void edt_row_pass(const Args& a) {
    const unsigned row = blockIdx.x * (EDT_ROW_THREADS / 64) + (unsigned)wave_id();
    if (row >= a.rows) return;                                                 // (whole waves leave; nothing below synchronises workgroups)
    const int lane = threadIdx.x & 63;
    const int W = a.W;
    const T* lab = reinterpret_cast<const T*>(a.labels) + (size_t)row * (size_t)W;
    int* map = a.map + (size_t)row * (size_t)W;
    int* feat = nullptr;
    int row_base = 0;
    if constexpr (FEAT) {
        feat = a.feat + (size_t)row * (size_t)W;
        row_base = (int)(row % a.rows_per_entry) * W;                          // (an entry has fewer than 2^31 positions)
    }
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
                if constexpr (FEAT) *reinterpret_cast<int4*>(feat + x) = make_int4(f[0], f[1], f[2], f[3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < W) {
                    map[x + j] = out[j];
                    if constexpr (FEAT) feat[x + j] = f[j];
                }
        }
        carry = min(carry, __shfl(inc, 0));
    }
}

// ---------------------------------------------------------------------------------------------------------- line passes
// Along H, then along D for dims = 3: the lower envelope of the parabolas f(j) + (i - j)^2 of every line (Meijster, Roerdink &
// Hesselink 2000).  One lane per line, the 64 lanes of a wave on 64 neighbouring lines, so every load and store of the wave is a
// contiguous row segment although the line itself is strided.  The envelope's stack (vertex index s, start t of its interval) lies in
// the workspace, laid out [height][line] like the map itself -- it is NOT a private array: no scratch -- and its top entry is kept in
// registers, so the stack is written at a push and read at a pop only.  Sentinel values push nothing; a line that ends with an empty
// stack gets the sentinel.  The query walk knows the vertex s of the parabola that is lowest at every position: with FEAT it copies the
// feature the previous pass left at s -- one gather load per position, taken before the pop.  store(p, d, f) writes position p: its
// squared distance d in the type of the maps and its feature f (-1 without FEAT, or where there is no site).  Args is the kernel's own
// argument struct: in (the distance map of the previous axis), s, t (the stack), sp, n, inner, bpo, and with FEAT fin (its feature map).
template <bool FLT, bool FEAT, class Args, class Store>
__device__ __forceinline__ void edt_line_pass(const Args& a, Store&& store) {
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
            if constexpr (FEAT) f = a.fin[base + (unsigned)s * inner];         // the site the winning vertex measures to (s: before the pop)
            if (u == t && q > 0) {                                             // (t of entry 0 is 0: the stack lasts for the whole line)
                --q;
                s = a.s[base + (unsigned)q * inner];
                t = a.t[base + (unsigned)q * inner];
                g = in[base + (unsigned)s * inner];
            }
        }
        store(p, d, f);
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
// the shape of a call: check_shape, and the limit of the int32 arithmetic on the sum of the squared extents
static inline int edt_check_shape(int dims, long long B, long long D, long long H, long long W) {
    if (int rc = check_shape(dims, B, D, H, W)) return rc;
    if ((dims == 3 ? D * D : 0) + H * H + W * W > MAX_POS) return PTB_EUNSUPPORTED;           // (each extent is < 2^31 here: no overflow in 64 bits)
    return PTB_OK;
}

static inline bool edt_spacing_ok(const double* spacing, int dims) {
    for (int k = 0; k < 3; ++k)
        if ((k > 0 || dims == 3) && !(spacing[k] > 0.0 && std::isfinite(spacing[k]))) return false;
    return true;
}

}  // namespace ptb
