// ptb_volume_channels_last.hip -- the 3-D mirror TTA and slab merge kernels on channels-last model outputs (PTB_SRC_CHANNELS_LAST on a
// 5-D batch), gfx950 / MI355X.
//
// A 3-D model in torch.channels_last_3d returns [V*B, d, h, w, C] memory: the C channels of a voxel lie next to each other.  These kernels
// do what volume_mirror_reduce_kernel / volume_mirror_accumulate_kernel (ptb_volume_tta.hip) and volume_gather_kernel
// (ptb_volume_bands.hip) do and write what they write -- dense planar output, planar fp32 accumulators, the PTB_CROP_* results -- but read
// such a source where it lies, so the [V*B, C, d, h, w] copy never exists.
//
// Work division (the 2-D design of ptb_channels_last.hip): a mirror view permutes VOXELS, and here a voxel is one contiguous run of C
// elements, so nothing is transposed or reversed inside a lane.  A lane owns one output voxel and handles its channels four at a time:
// one 16-byte load per view for four fp32 channels, 8 bytes for four half channels, when C is a multiple of 4 and the tile pointers are
// aligned; element loads of the same four channels otherwise.  Consecutive lanes take consecutive x, so a W-flip reads a descending
// but still contiguous span, and the planar weight / volume / norm / cdhw-result accesses are coalesced 4-byte accesses per channel
// plane.  Weight and normaliser are touched once per voxel, not once per channel.  C, masks, reduction, extents and the result layout are
// run-time values.  No LDS, no scratch, no atomics.
//
// Per voxel and channel the arithmetic is the planar kernels': views summed in view order with __fadd_rn through red_pre / red_post /
// the divisor, the reduced value of a half-precision source rounded to its type (round_src1), then tile * window rounded and added in
// integration order (no contraction) -- bit-identical results.
#include "ptb_crop_device.h"
#include "ptb_dispatch.h"
#include "ptb_mirror_device.h"
#include "ptb_volume_device.h"

namespace ptb {

namespace {

constexpr int CL3_BLOCK = 256;
constexpr int CL3_GRID_X = 8192;  // workgroups over the voxels of one tile (grid-stride beyond), as the planar mirror kernels
constexpr int CL3_NC = 4;         // channels a lane handles at a time

// channels c0 .. c0+3 of the voxel whose channel c0 is element `off` of `base`; channels >= nc stay 1 (never stored)
template <int LD, bool VEC>
__device__ __forceinline__ float4 cl3_load(const void* base, long long off, int nc) {
    if constexpr (VEC) {
        return ld4<LD>(static_cast<const float*>(base), off);
    } else {
        float4 v = make_float4(1.f, 1.f, 1.f, 1.f);
        v.x = widen<ld_dtype<LD>()>(base, off);
        if (nc > 1) v.y = widen<ld_dtype<LD>()>(base, off + 1);
        if (nc > 2) v.z = widen<ld_dtype<LD>()>(base, off + 2);
        if (nc > 3) v.w = widen<ld_dtype<LD>()>(base, off + 3);
        return v;
    }
}

// mirror_reduce_voxels for channels c0 .. c0+3 of output voxel (z, y, x) of one tile: `off0` = element offset of view 0 of the tile in
// `src`, `view_stride` = B * C * D * H * W.  All loads are issued before the sum.
template <int LD, int OPK, bool VEC>
__device__ __forceinline__ float4 cl3_reduce_vox(const void* __restrict__ src, long long off0, long long view_stride, int nv, int masks, int op,
                                                 float divisor, int z, int y, int x, int D, int H, int W, int C, int c0, int nc) {
    float4 v[MAX_VIEWS];
#pragma unroll
    for (int k = 0; k < MAX_VIEWS; ++k) {
        v[k] = make_float4(1.f, 1.f, 1.f, 1.f);
        if (k < nv) {
            const int m = (masks >> (3 * k)) & 7;
            v[k] = cl3_load<LD, VEC>(src, off0 + k * view_stride + mirror_src<1>(m, z, y, x, D, H, W) * C + c0, nc);
        }
    }
    float4 s = make_float4(red_pre<OPK>(v[0].x, op), red_pre<OPK>(v[0].y, op), red_pre<OPK>(v[0].z, op), red_pre<OPK>(v[0].w, op));
#pragma unroll
    for (int k = 1; k < MAX_VIEWS; ++k) {
        if (k < nv) {
            s.x = __fadd_rn(s.x, red_pre<OPK>(v[k].x, op));
            s.y = __fadd_rn(s.y, red_pre<OPK>(v[k].y, op));
            s.z = __fadd_rn(s.z, red_pre<OPK>(v[k].z, op));
            s.w = __fadd_rn(s.w, red_pre<OPK>(v[k].w, op));
        }
    }
    return make_float4(red_post<OPK>(s.x, op, divisor), red_post<OPK>(s.y, op, divisor), red_post<OPK>(s.z, op, divisor),
                       red_post<OPK>(s.w, op, divisor));
}

template <int LD>
__device__ __forceinline__ float4 cl3_round(const float4 r) {
    return make_float4(round_src1<LD>(r.x), round_src1<LD>(r.y), round_src1<LD>(r.z), round_src1<LD>(r.w));
}

// voxel index inside a [D, H, W] plane -> (z, y, x)
__device__ __forceinline__ void cl3_zyx(int u, int H, int W, int& z, int& y, int& x) {
    const int row = u / W;
    x = u - row * W;
    z = row / H;
    y = row - z * H;
}

// one element of the source type at element offset `o` of `dst`
template <int LD>
__device__ __forceinline__ void cl3_store_src(void* dst, long long o, float v) {
    constexpr int OUT = ld_dtype<LD>();
    if constexpr (OUT == PTB_F32) static_cast<float*>(dst)[o] = v;
    else static_cast<unsigned short*>(dst)[o] = half_bits<OUT>(v);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ de-augment + reduce (volume_mirror_reduce_kernel)
// out[b] = reduce_v(unflip_v(src[v * B + b])), dense [B, C, D, H, W] in the source type.  blockIdx.y walks the tiles b.
template <int LD, int OPK, bool VEC>
__global__ __launch_bounds__(CL3_BLOCK) void cl3_reduce_kernel(const MirrorArgs a) {
    const int plane = a.D * a.H * a.W;
    const long long tile_elems = (long long)a.C * plane;
    const void* __restrict__ src = a.src;
    void* __restrict__ dst = a.dst;
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        const long long off0 = b * tile_elems;
        for (int u = blockIdx.x * CL3_BLOCK + threadIdx.x; u < plane; u += gridDim.x * CL3_BLOCK) {
            int z, y, x;
            cl3_zyx(u, a.H, a.W, z, y, x);
            for (int c0 = 0; c0 < a.C; c0 += CL3_NC) {
                const int nc = min(CL3_NC, a.C - c0);
                const float4 r = cl3_reduce_vox<LD, OPK, VEC>(src, off0, a.view_stride, a.nv, a.masks, a.op, a.divisor, z, y, x, a.D, a.H, a.W,
                                                              a.C, c0, nc);
                const long long o = off0 + (long long)c0 * plane + u;
                cl3_store_src<LD>(dst, o, r.x);
                if (nc > 1) cl3_store_src<LD>(dst, o + plane, r.y);
                if (nc > 2) cl3_store_src<LD>(dst, o + 2LL * plane, r.z);
                if (nc > 3) cl3_store_src<LD>(dst, o + 3LL * plane, r.w);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ fused blend (volume_mirror_accumulate_kernel)
// One tile per launch: a tile never overlaps itself, so a launch owns its accumulator region and stream order gives the sequential
// fp32 order.  One workgroup walks all channels of its voxels; weight and norm are touched once per voxel.
template <int LD, int OPK, bool VEC>
__global__ __launch_bounds__(CL3_BLOCK) void cl3_accum_kernel(const MirrorAccArgs a) {
    const int tplane = a.d * a.h * a.w;
    const long long vplane = (long long)a.D * a.H * a.W;
    const float* __restrict__ weight = a.weight;
    const void* __restrict__ tiles = a.tiles;
    float* __restrict__ norm = a.norm;
    for (int u = blockIdx.x * CL3_BLOCK + threadIdx.x; u < tplane; u += gridDim.x * CL3_BLOCK) {
        int z, y, x;
        cl3_zyx(u, a.h, a.w, z, y, x);
        const long long voff = ((long long)(a.z0 + z) * a.H + (a.y0 + y)) * a.W + a.x0 + x;
        const float wv = weight[u];
        const float n0 = norm[voff];
        for (int c0 = 0; c0 < a.C; c0 += CL3_NC) {
            const int nc = min(CL3_NC, a.C - c0);
            // every load of the group -- the views and the four accumulator planes -- is issued before its first store: one round trip
            const float4 t = cl3_round<LD>(cl3_reduce_vox<LD, OPK, VEC>(tiles, a.tile_off, a.view_stride, a.nv, a.masks, a.op, a.divisor, z, y, x,
                                                                        a.d, a.h, a.w, a.C, c0, nc));
            float* vp = a.volume + c0 * vplane + voff;
            float4 v = make_float4(vp[0], 0.f, 0.f, 0.f);
            if (nc > 1) v.y = vp[vplane];
            if (nc > 2) v.z = vp[2 * vplane];
            if (nc > 3) v.w = vp[3 * vplane];
            vp[0] = __fadd_rn(v.x, __fmul_rn(t.x, wv));
            if (nc > 1) vp[vplane] = __fadd_rn(v.y, __fmul_rn(t.y, wv));
            if (nc > 2) vp[2 * vplane] = __fadd_rn(v.z, __fmul_rn(t.z, wv));
            if (nc > 3) vp[3 * vplane] = __fadd_rn(v.w, __fmul_rn(t.w, wv));
        }
        norm[voff] = __fadd_rn(n0, wv);
    }
}

// ------------------------------------------------------------------------------------------------ deferred slab merge (volume_gather_kernel)
namespace {

// The four channels c0 .. c0+3 of a voxel are ready: store them (cast and layout of ptb_merge_crop.hip), or fold them, in channel order,
// into the running argmax (first maximum wins; NaN counts as the maximum, like numpy / torch argmax)
template <int KIND>
__device__ __forceinline__ void cl3_emit(const VolArgs& a, long long vox, int c0, int nc, const float4 q4, float& best, int& arg) {
    const float q[4] = {q4.x, q4.y, q4.z, q4.w};
    if constexpr (vb_argmax<KIND>()) {
#pragma unroll
        for (int m = 0; m < CL3_NC; ++m) {
            const bool take = m < nc && (c0 + m == 0 ? true : (q[m] > best || (q[m] != q[m] && best == best)));
            best = take ? q[m] : best;
            arg = take ? c0 + m : arg;
        }
    } else if (a.layout == 0 || a.C == 1) {
        const long long oplane = (long long)a.OD * a.OH * a.OW;
#pragma unroll
        for (int m = 0; m < CL3_NC; ++m) {
            if (m < nc) {
                const float one[4] = {q[m], 0.f, 0.f, 0.f};
                store_out<KIND>(a.out, (c0 + m) * oplane + vox, one, 1);
            }
        }
    } else {
        store_out<KIND>(a.out, vox * a.C + c0, q, nc);     // "dhwc": the group's channels lie together
    }
}

template <int KIND>
__device__ __forceinline__ void cl3_emit_argmax(const VolArgs& a, long long vox, int arg) {
    if constexpr (KIND == PTB_CROP_ARGMAX_U8) static_cast<uint8_t*>(a.out)[vox] = (uint8_t)arg;
    else if constexpr (KIND == PTB_CROP_ARGMAX_I64) static_cast<long long*>(a.out)[vox] = arg;
}

// voxel u of an item (x fastest, then y, then z) -> offsets from the item's origin
__device__ __forceinline__ void cl3_unit(int u, int nx, int ny, int& dz, int& dy, int& dx) {
    const int row = u / nx;
    dx = u - row * nx;
    dz = row / ny;
    dy = row - dz * ny;
}

// No TTA.  NT = the item's tile count rounded up to 1, 2, 4 or 8: a fixed unrolled set of loads per lane and channel group, all issued
// before the dependent add chain; the padding entries load tile 0 again and are left out of the sums by a select, never by a branch.
template <int LD, bool VEC, int KIND, int NT>
__device__ __forceinline__ void cl3_gather_plain(const VolArgs& a, const VolTiles& t, const VolItem* it, int ntiles) {
    const int nx = it->nx, ny = it->ny, nz = it->nz, x0 = it->x0, y0 = it->y0, z0 = it->z0;
    const int units = nz * ny * nx;
    const void* src[NT];
    int lx[NT], ly[NT], lz[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const unsigned long long cv = it->cover[k];
        src[k] = t.src[(int)(cv & 0xffffu)];
        lx[k] = (int)((cv >> 16) & 0xffffu);
        ly[k] = (int)((cv >> 32) & 0xffffu);
        lz[k] = (int)(cv >> 48);
    }
    for (int u = threadIdx.x; u < units; u += VB_BLOCK) {
        int dz, dy, dx;
        cl3_unit(u, nx, ny, dz, dy, dx);
        const VolPos p = vol_pos(a, z0 + dz, y0 + dy, x0 + dx, 1);
        if (p.cnt <= 0) continue;                     // the 4-aligned hull of the window in x: nothing to store
        long long off[NT];
        float wt[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const int vo = ((lz[k] + dz) * a.h + ly[k] + dy) * a.w + lx[k] + dx;
            wt[k] = a.weight[vo];
            off[k] = (long long)vo * a.C;
        }
        float n = 0.f;
#pragma unroll
        for (int k = 0; k < NT; ++k) n = k < ntiles ? __fadd_rn(n, wt[k]) : n;
        float best = 0.f;
        int arg = 0;
        for (int c0 = 0; c0 < a.C; c0 += CL3_NC) {
            const int nc = min(CL3_NC, a.C - c0);
            float4 v[NT];
#pragma unroll
            for (int k = 0; k < NT; ++k) v[k] = cl3_load<LD, VEC>(src[k], off[k] + c0, nc);
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const bool on = k < ntiles;
                s.x = on ? __fadd_rn(s.x, __fmul_rn(v[k].x, wt[k])) : s.x; s.y = on ? __fadd_rn(s.y, __fmul_rn(v[k].y, wt[k])) : s.y;
                s.z = on ? __fadd_rn(s.z, __fmul_rn(v[k].z, wt[k])) : s.z; s.w = on ? __fadd_rn(s.w, __fmul_rn(v[k].w, wt[k])) : s.w;
            }
            cl3_emit<KIND>(a, p.vox, c0, nc, make_float4(__fdiv_rn(s.x, n), __fdiv_rn(s.y, n), __fdiv_rn(s.z, n), __fdiv_rn(s.w, n)), best, arg);
        }
        cl3_emit_argmax<KIND>(a, p.vox, arg);
    }
}

// Mirror TTA.  Per covering tile the V views are un-flipped and reduced by cl3_reduce_vox (its loads issued before its sum), rounded to
// the source type and blended; tiles are walked in a loop, the views are the unrolled set.
template <int LD, int OPK, bool VEC, int KIND>
__device__ __forceinline__ void cl3_gather_tta(const VolArgs& a, const VolTiles& t, const VolItem* it, int ntiles) {
    const int nx = it->nx, ny = it->ny, nz = it->nz, x0 = it->x0, y0 = it->y0, z0 = it->z0;
    const int units = nz * ny * nx;
    for (int u = threadIdx.x; u < units; u += VB_BLOCK) {
        int dz, dy, dx;
        cl3_unit(u, nx, ny, dz, dy, dx);
        const VolPos p = vol_pos(a, z0 + dz, y0 + dy, x0 + dx, 1);
        if (p.cnt <= 0) continue;
        float n = 0.f;
        for (int k = 0; k < ntiles; ++k) {
            const unsigned long long cv = it->cover[k];
            n = __fadd_rn(n, a.weight[(((int)(cv >> 48) + dz) * a.h + (int)((cv >> 32) & 0xffffu) + dy) * a.w + (int)((cv >> 16) & 0xffffu) + dx]);
        }
        float best = 0.f;
        int arg = 0;
        for (int c0 = 0; c0 < a.C; c0 += CL3_NC) {
            const int nc = min(CL3_NC, a.C - c0);
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < ntiles; ++k) {
                const unsigned long long cv = it->cover[k];
                const int slot = (int)(cv & 0xffffu);
                const int tz = (int)(cv >> 48) + dz, ty = (int)((cv >> 32) & 0xffffu) + dy, tx = (int)((cv >> 16) & 0xffffu) + dx;
                const float4 r = cl3_round<LD>(cl3_reduce_vox<LD, OPK, VEC>(t.src[slot], 0, t.vs[slot], a.nv, a.masks, a.op, a.divisor, tz, ty, tx,
                                                                            a.d, a.h, a.w, a.C, c0, nc));
                const float wv = a.weight[(tz * a.h + ty) * a.w + tx];
                s.x = __fadd_rn(s.x, __fmul_rn(r.x, wv)); s.y = __fadd_rn(s.y, __fmul_rn(r.y, wv));
                s.z = __fadd_rn(s.z, __fmul_rn(r.z, wv)); s.w = __fadd_rn(s.w, __fmul_rn(r.w, wv));
            }
            cl3_emit<KIND>(a, p.vox, c0, nc, make_float4(__fdiv_rn(s.x, n), __fdiv_rn(s.y, n), __fdiv_rn(s.z, n), __fdiv_rn(s.w, n)), best, arg);
        }
        cl3_emit_argmax<KIND>(a, p.vox, arg);
    }
}

// voxels nobody covers: what volume / norm_mask hold there is 0 and 0, and the plain merge divides them (gather_empty)
template <int KIND>
__device__ __forceinline__ void cl3_gather_empty(const VolArgs& a, const VolItem* it) {
    const int nx = it->nx, ny = it->ny, nz = it->nz;
    const int units = nz * ny * nx;
    const float zero = __int_as_float(it->zero);
    for (int u = threadIdx.x; u < units; u += VB_BLOCK) {
        int dz, dy, dx;
        cl3_unit(u, nx, ny, dz, dy, dx);
        const VolPos p = vol_pos(a, it->z0 + dz, it->y0 + dy, it->x0 + dx, 1);
        if (p.cnt <= 0) continue;
        float best = 0.f;
        int arg = 0;
        for (int c0 = 0; c0 < a.C; c0 += CL3_NC) {
            const float r = __fdiv_rn(zero, zero);
            cl3_emit<KIND>(a, p.vox, c0, min(CL3_NC, a.C - c0), make_float4(r, r, r, r), best, arg);
        }
        cl3_emit_argmax<KIND>(a, p.vox, arg);
    }
}

}  // namespace

// LD: 1 = fp32, 2 = fp16, 3 = bf16 sources; MODE: 0 = plain tiles, 1 = mirror TTA with a linear reduction, 2 = with a non-linear one;
// VEC: 16- / 8-byte | element loads; KIND: PTB_CROP_*.  One workgroup per work item of the plan's table.
template <int LD, int MODE, bool VEC, int KIND>
__global__ __launch_bounds__(VB_BLOCK) void cl3_gather_kernel(const VolArgs a, const VolTiles t) {
    const VolItem* it = a.items + blockIdx.x;
    const int ntiles = it->ntiles;
    if (ntiles == 0) {
        cl3_gather_empty<KIND>(a, it);
    } else if constexpr (MODE == 0) {
        if (ntiles > 4) cl3_gather_plain<LD, VEC, KIND, 8>(a, t, it, ntiles);
        else if (ntiles > 2) cl3_gather_plain<LD, VEC, KIND, 4>(a, t, it, ntiles);
        else if (ntiles == 2) cl3_gather_plain<LD, VEC, KIND, 2>(a, t, it, ntiles);
        else cl3_gather_plain<LD, VEC, KIND, 1>(a, t, it, ntiles);
    } else {
        cl3_gather_tta<LD, MODE - 1, VEC, KIND>(a, t, it, ntiles);
    }
}

// ------------------------------------------------------------------------------------------------ dispatch
// four channels per load: C a multiple of 4 (then every voxel of an aligned tile is aligned), 16- / 8-byte aligned tiles, view strides on
// the same grid, and the force-scalar switch off.  (cl_vec_ok of the 2-D unit does not look at that switch: known, and left as it is.)
static bool cl3_vec_ok(int dtype, int C, const void* p, long long stride0, long long stride1) {
    const uintptr_t mask = dtype == PTB_F32 ? 15u : 7u;
    return !g_force_scalar && C % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & mask) == 0 && stride0 % 4 == 0 && stride1 % 4 == 0;
}

static dim3 cl3_grid(long long voxels, long long tiles) {
    const long long gx = (voxels + CL3_BLOCK - 1) / CL3_BLOCK;
    return dim3((unsigned)(gx < CL3_GRID_X ? gx : CL3_GRID_X), (unsigned)(tiles < 65535 ? tiles : 65535));
}

// (linear | non-linear reduction) x source dtype x (vector | element loads): 12 instances
template <class F>
static void with_cl3_instance(int dtype, int op, bool vec, F&& f) {
    with_src_dtype(dtype, [&](auto ld) { with_reduction(op, [&](auto opk) { with_bool(vec, [&](auto v) { f(ld, opk, v); }); }); });
}

void cl3_launch_reduce(const MirrorArgs& a, int dtype, hipStream_t s) {
    const long long plane = (long long)a.D * a.H * a.W;
    const dim3 grid = cl3_grid(plane, a.B);
    const bool vec = cl3_vec_ok(dtype, a.C, a.src, a.view_stride, 0);
    with_cl3_instance(dtype, a.op, vec, [&](auto ld, auto opk, auto v) {
        hipLaunchKernelGGL((cl3_reduce_kernel<ld(), opk(), v()>), grid, dim3(CL3_BLOCK), 0, s, a); });
}

void cl3_launch_accum(const MirrorAccArgs& a, int dtype, hipStream_t s) {
    const dim3 grid = cl3_grid((long long)a.d * a.h * a.w, 1);
    const bool vec = cl3_vec_ok(dtype, a.C, a.tiles, a.view_stride, a.tile_off);
    with_cl3_instance(dtype, a.op, vec, [&](auto ld, auto opk, auto v) {
        hipLaunchKernelGGL((cl3_accum_kernel<ld(), opk(), v()>), grid, dim3(CL3_BLOCK), 0, s, a); });
}

void cl3_launch_gather(const VolArgs& a, const VolTiles& t, int n_tiles, int dtype, int mode, int kind, int n_items, hipStream_t s) {
    bool vec = true;
    for (int k = 0; k < n_tiles; ++k) vec = vec && cl3_vec_ok(dtype, a.C, t.src[k], t.vs[k], 0);
    const dim3 grid((unsigned)n_items), block(VB_BLOCK);
    with_src_dtype(dtype, [&](auto ld) { with_value<0, 1, 2>(mode, [&](auto m) { with_bool(vec, [&](auto v) {
        with_crop_kind(kind, [&](auto k) {
            hipLaunchKernelGGL((cl3_gather_kernel<ld(), m(), v(), k()>), grid, block, 0, s, a, t); }); }); }); });
}

}  // namespace ptb
