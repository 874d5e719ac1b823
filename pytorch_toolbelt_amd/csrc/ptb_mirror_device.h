// Device-side pieces of the 3-D mirror TTA shared by ptb_volume_tta.hip (reduce / accumulate per tile) and ptb_volume_bands.hip (the
// deferred slab merge): where view `m` keeps a voxel, and the per-voxel de-augmentation over the views.
#pragma once
#include "ptb_view_device.h"

namespace ptb {

// Element offset, inside one [D, H, W] plane, of the PIX source elements view `m` puts at output (z, y, x .. x + PIX - 1): the
// first of them in memory order (a W-flipped run is read from there and reversed).
template <int PIX>
__device__ __forceinline__ long long mirror_src(int m, int z, int y, int x, int D, int H, int W) {
    const int sz = (m & 4) ? D - 1 - z : z;
    const int sy = (m & 2) ? H - 1 - y : y;
    const int sx = (m & 1) ? W - PIX - x : x;
    return ((long long)sz * H + sy) * W + sx;
}

__device__ __forceinline__ float4 rev4(const float4 t) { return make_float4(t.w, t.z, t.y, t.x); }

// The per-voxel de-augmentation shared by ptb_volume_mirror_reduce, ptb_volume_mirror_accumulate and the deferred slab merge: the PIX
// (4 or 1) outputs at (z, y, x..) of one (tile, channel) = post(sum_v pre(unflip_v(view v))), summed in fp32 in view order with
// __fadd_rn (red_pre / red_post / div_views of the 2-D TTA kernels).  `src` + `plane` = view 0 of this tile and channel,
// `view_stride` = B * C * D * H * W.  All loads are issued before the sum.
template <int LD, int OPK, int PIX>
__device__ __forceinline__ float4 mirror_reduce_voxels(const void* __restrict__ src, long long plane, long long view_stride, int nv,
                                                       int masks, int op, float divisor, int z, int y, int x, int D, int H, int W) {
    float4 v[MAX_VIEWS];
#pragma unroll
    for (int k = 0; k < MAX_VIEWS; ++k) {
        v[k] = make_float4(1.f, 1.f, 1.f, 1.f);
        if (k < nv) {
            const int m = (masks >> (3 * k)) & 7;
            const long long off = plane + k * view_stride + mirror_src<PIX>(m, z, y, x, D, H, W);
            if constexpr (PIX == 4) {
                const float4 t = ld4<LD>(static_cast<const float*>(src), off);
                v[k] = (m & 1) ? rev4(t) : t;
            } else {
                v[k].x = widen<ld_dtype<LD>()>(src, off);
            }
        }
    }
    float4 s = make_float4(red_pre<OPK>(v[0].x, op), red_pre<OPK>(v[0].y, op), red_pre<OPK>(v[0].z, op), red_pre<OPK>(v[0].w, op));
#pragma unroll
    for (int k = 1; k < MAX_VIEWS; ++k) {
        if (k < nv) {
            s.x = __fadd_rn(s.x, red_pre<OPK>(v[k].x, op));
            if constexpr (PIX == 4) {
                s.y = __fadd_rn(s.y, red_pre<OPK>(v[k].y, op));
                s.z = __fadd_rn(s.z, red_pre<OPK>(v[k].z, op));
                s.w = __fadd_rn(s.w, red_pre<OPK>(v[k].w, op));
            }
        }
    }
    return make_float4(red_post<OPK>(s.x, op, divisor), red_post<OPK>(s.y, op, divisor), red_post<OPK>(s.z, op, divisor),
                       red_post<OPK>(s.w, op, divisor));
}

}  // namespace ptb
