// The source taps of one axis of a linear resize, shared by the 2-D resize kernels (ptb_resample.hip) and the 3-D ones
// (ptb_volume_resample.hip): ATen's area_pixel_compute_source_index / compute_source_index_and_lambda, evaluated in fp32 like torch's GPU
// kernels.  scale = n_in / n_out, or (n_in - 1) / (n_out - 1) with align_corners (0 when n_out == 1).
#pragma once
#include "ptb_common.h"

namespace ptb {

struct Taps { int i0, i1; float l0, l1; };

// (__host__ too: a launcher that sizes an LDS window from the taps evaluates this very function, not a copy of it)
template <int ALIGN = -1>   // -1: run-time align_corners; 0 / 1: compile-time (no branch in the unrolled tap code)
__host__ __device__ __forceinline__ Taps taps(int dst, float scale, int n_in, bool align_corners) {
    float src;
    if (ALIGN < 0 ? align_corners : (ALIGN == 1)) {
        src = scale * (float)dst;
    } else {
        src = scale * ((float)dst + 0.5f) - 0.5f;
        src = src < 0.f ? 0.f : src;
    }
    Taps t;
    t.i0 = min((int)src, n_in - 1);
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
    t.l0 = 1.f - t.l1;
    return t;
}

}  // namespace ptb
