// What the distance transform (ptb_distance.hip) and the feature transform (ptb_nearest.hip) share: the sentinels and limits, the two
// wave scans of the row passes, the arithmetic of a parabola of the lower envelope in its int32 and float32 forms, and the host-side
// checks of a shape.  Device pieces are forced inline, host pieces are static: each translation unit compiles its own copy.
#pragma once

#include <cmath>
#include <type_traits>

#include "ptb_common.h"

namespace ptb {

constexpr int EDT_ROW_THREADS = 256;            // four waves, a row each
constexpr int EDT_CHUNK = 256;                  // positions of a row a wave handles per trip: 64 lanes x 4
constexpr int EDT_LINE_THREADS = 64;            // one wave per workgroup: a single 2-D image has only W lines, spread them over the CUs
constexpr int EDT_INF = 0x7fffffff;             // the int32 sentinel
constexpr int EDT_BIG = 0x3fffffff;             // "no site to the right" (an index never reaches it)
constexpr long long EDT_MAX_POS = 0x7fffffffLL - 1;

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

// ---------------------------------------------------------------------------------------------------------- host side
static inline long long edt_up16(long long v) { return (v + 15) & ~15LL; }

// the shape of a call: PTB_EINVAL for what is no shape, PTB_EUNSUPPORTED above the limits
static inline int edt_check_shape(int dims, long long B, long long D, long long H, long long W) {
    if ((dims != 2 && dims != 3) || B < 1 || D < 1 || H < 1 || W < 1 || (dims == 2 && D != 1)) return PTB_EINVAL;
    if (D > EDT_MAX_POS || H > EDT_MAX_POS || W > EDT_MAX_POS || H * W > EDT_MAX_POS || D * H * W > EDT_MAX_POS || B > EDT_MAX_POS / (D * H * W)) return PTB_EUNSUPPORTED;
    if ((dims == 3 ? D * D : 0) + H * H + W * W > EDT_MAX_POS) return PTB_EUNSUPPORTED;       // (each extent is < 2^31 here: no overflow in 64 bits)
    return PTB_OK;
}

template <int EB>
using edt_label_t = std::conditional_t<EB == 1, unsigned char, std::conditional_t<EB == 2, short, std::conditional_t<EB == 4, int, long long>>>;

static inline bool edt_holds(int elem_bytes, long long v) {
    switch (elem_bytes) {
        case 1: return v >= 0 && v <= 255;
        case 2: return v >= -32768 && v <= 32767;
        case 4: return v >= -2147483648LL && v <= 2147483647LL;
        default: return true;
    }
}

static inline bool edt_spacing_ok(const double* spacing, int dims) {
    for (int k = 0; k < 3; ++k)
        if ((k > 0 || dims == 3) && !(spacing[k] > 0.0 && std::isfinite(spacing[k]))) return false;
    return true;
}

}  // namespace ptb
