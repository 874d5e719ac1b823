// Device helpers of the merge + crop kernels, shared by the 2-D (ptb_edges.hip) and 3-D (ptb_volume_edges.hip) loop edges.
#pragma once
#include "ptb_view_device.h"

namespace ptb {

// numpy / torch float -> uint8 cast as x86-64 performs it: truncate toward zero to int32, keep the low byte
// (values outside the int32 range, NaN and infinities give 0).  In [0, 256) this is the plain truncation of
// ImageSlicer.merge / README.md:225 (quirk Q6).
__device__ __forceinline__ uint8_t cast_u8(float v) {
    if (!(fabsf(v) < 2147483648.0f)) return 0;
    return (uint8_t)((int)v & 255);
}

// 4 consecutive source floats of one row; `vec` (uniform): the window is 16 B aligned in the accumulator
__device__ __forceinline__ void load_px4(const float* p, int nv, bool vec, float* o) {
    if (!p) { o[0] = o[1] = o[2] = o[3] = 1.0f; return; }  // norm == NULL: the image is already normalised
    if (vec && nv == 4) {
        const float4 t = ld16<true>(p);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
        for (int m = 0; m < 4; ++m) o[m] = m < nv ? p[m] : 1.0f;
    }
}

__device__ __forceinline__ void store_f32x4(float* p, const float* v, int nv) {
    if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) out_store4(p, make_float4(v[0], v[1], v[2], v[3]));
    else for (int m = 0; m < nv; ++m) p[m] = v[m];
}
__device__ __forceinline__ void store_u8x4(uint8_t* p, const uint8_t* v, int nv) {
    if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0)
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    else for (int m = 0; m < nv; ++m) p[m] = v[m];
}

}  // namespace ptb
