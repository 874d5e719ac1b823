// The cast and store rules of the merge+crop outputs (PTB_CROP_* kinds), shared by ptb_merge_crop.hip and the deferred slab merge of
// ptb_volume_bands.hip.
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

__device__ __forceinline__ void store_f32x4(float* p, const float* v, int nv) {
    if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) out_store4(p, make_float4(v[0], v[1], v[2], v[3]));
    else for (int m = 0; m < nv; ++m) p[m] = v[m];
}
__device__ __forceinline__ void store_u8x4(uint8_t* p, const uint8_t* v, int nv) {
    if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0)
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    else for (int m = 0; m < nv; ++m) p[m] = v[m];
}

// nv (<= 4) consecutive output elements starting at element `o`, converted to KIND; one 16 / 8 / 4 B store when aligned
template <int KIND>
__device__ __forceinline__ void store_out(void* out, long long o, const float* v, int nv) {
    if constexpr (KIND == PTB_CROP_F32) {
        store_f32x4(static_cast<float*>(out) + o, v, nv);
    } else if constexpr (KIND == PTB_CROP_U8) {
        uint8_t b[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) b[m] = cast_u8(v[m]);
        store_u8x4(static_cast<uint8_t*>(out) + o, b, nv);
    } else {
        constexpr int OUT = KIND == PTB_CROP_F16 ? PTB_F16 : PTB_BF16;
        unsigned short* p = static_cast<unsigned short*>(out) + o;
        unsigned short b[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) b[m] = half_bits<OUT>(v[m]);
        if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
            typedef unsigned int u2 __attribute__((ext_vector_type(2)));
            *reinterpret_cast<u2*>(p) = u2{(unsigned)b[0] | ((unsigned)b[1] << 16), (unsigned)b[2] | ((unsigned)b[3] << 16)};
        } else {
            for (int m = 0; m < nv; ++m) p[m] = b[m];
        }
    }
}

}  // namespace ptb
